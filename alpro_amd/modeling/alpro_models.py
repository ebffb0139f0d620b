"""ALPRO model API on the MI355X kernels.

Drop-in for the reference's src/modeling/alpro_models.py: same class names
(AlproBaseModel :19, AlproForPretrain :58, Prompter :389, AlproForSequenceClassification :633,
AlproForVideoTextRetrieval :727), constructor signatures `(config, video_enc_cfg, input_format)`,
`forward(batch) -> dict` keys, `forward_inference`, `build_text_prompts`, `get_pseudo_labels`,
`load_separate_ckpt`, and the state_dict key layout.

Encoders run in libalpro_hip.so (alpro_amd.modeling.timesformer.vit / xbert).  The heads are
(B x 256)-sized: their Linear layers go through alpro_gemm in exact fp32 mode on the fp32 masters
(keeps VTC logits within 1e-3 of the reference even when the encoders run in bf16), the remaining
(B x B) loss arithmetic is plain device-side torch.  Differences from the reference, all
value-preserving: hard negatives are drawn with ONE batched torch.multinomial per direction instead
of 2B `.item()` host syncs (alpro_models.py:301-313); Horovod is replaced by alpro_amd.dist (RCCL).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from alpro_amd import dist as hvd
from alpro_amd import hip
from alpro_amd.modeling.timesformer.vit import TimeSformer  # noqa: F401  (resolved via video_enc_cfg['cls'])
from alpro_amd.modeling.xbert import BertForMaskedLM, BertModel

_VISUAL_CLASSES = {"TimeSformer": TimeSformer}


def _rows_ok(M, N, K):
    """shapes alpro_gemm_rows_f32 takes (include/alpro_hip.h): few rows, N % 16 == 0, K % 64 == 0"""
    return M <= 512 and N % 16 == 0 and K % 64 == 0


def _linear32(x, lin):
    """nn.Linear on fp32 rows through alpro_gemm's exact fp32 MFMA path (heads only)."""
    x = x.contiguous().float()
    return _Linear32.apply(x, lin.weight, lin.bias)


class _Linear32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        K = x.shape[1]
        if K % 32 != 0:
            raise RuntimeError("head Linear in_features must be a multiple of 32")
        if _rows_ok(x.shape[0], w.shape[0], K):   # a handful of rows: the skinny fp32 kernel (11-35 us) instead of a 128 x 128-tile launch (60-140 us)
            return hip.gemm_rows(x, w.detach().contiguous(), bias=None if b is None else b.detach())
        return hip.gemm(x, w.detach().contiguous(), bias=None if b is None else b.detach(), out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        # tiny (B x 256 x 768) products: dX = g W, dW = g^T X, db = sum g -- NT GEMMs on transposed copies
        dx = None
        if ctx.needs_input_grad[0]:
            wt = w.detach().t().contiguous()
            if _rows_ok(g.shape[0], wt.shape[0], 64):   # (contraction dim zero-padded to the skinny kernel's 64-granule: mpm_head's 1000 classes)
                dx = hip.gemm_rows(_pad_k(g, 64), _pad_k(wt, 64))
            else:
                dx = hip.gemm(_pad_k(g), _pad_k(wt), out_dtype=torch.float32)
        dw = hip.gemm(_pad_k(g.t().contiguous()), _pad_k(x.t().contiguous()), out_dtype=torch.float32) if ctx.needs_input_grad[1] else None
        db = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


class _FusionOutputs(torch.autograd.Function):
    """What the heads read out of the 4B-sequence fusion output (B positives, 2B hard negatives, B MLM pairs; alpro_models.py:283,331-338,
    366-371,215-218): the 3B [CLS] rows (ITM head), the MLM pairs' text rows (LM head) and the positives' patch rows (MPM head), as three
    contiguous tensors.  As plain slices each of them costs autograd a full-size zero tensor (186 MB at B = 64) plus an accumulation add when
    the pieces meet again (1.3 GB of traffic, ~0.5 ms per step); here the backward zero-fills the gradient ONCE and copies the three pieces in."""

    @staticmethod
    def forward(ctx, fused, b, txt_len):
        ctx.shape, ctx.b, ctx.txt_len = fused.shape, b, txt_len
        return fused[:3 * b, 0, :].contiguous(), fused[3 * b:, :txt_len].contiguous(), fused[:b, txt_len + 1:].contiguous()

    @staticmethod
    def backward(ctx, d_cls, d_mlm, d_vis):
        b, Lt = ctx.b, ctx.txt_len
        d = torch.zeros(ctx.shape, dtype=torch.float32, device=(d_cls if d_cls is not None else d_mlm if d_mlm is not None else d_vis).device)
        if d_cls is not None:
            d[:3 * b, 0, :] = d_cls
        if d_mlm is not None:
            d[3 * b:, :Lt] = d_mlm
        if d_vis is not None:
            d[:b, Lt + 1:] = d_vis
        return d, None, None


def _pad_k(t, granule=32):
    """Zero-pad the contraction dim to a multiple of 32 (alpro_gemm's K granule in fp32; 64: alpro_gemm_rows_f32's)."""
    k = t.shape[1]
    r = (-k) % granule
    return t if r == 0 else F.pad(t, (0, r))


class _VtcLoss(torch.autograd.Function):
    """alpro_vtc_loss as an autograd node: (v, t, gathered v, gathered t, temp) -> (loss, sim_v2t, sim_t2v); the similarity
    matrices are outputs for the hard-negative mining and the Prompter's score dict, gradients flow through the loss only (the
    reference differentiates nothing else through them: alpro_models.py:287-306 runs under no_grad)."""

    @staticmethod
    def forward(ctx, v, t, gv, gt, temp, col0):
        v, t, gv, gt = (x.contiguous().float() for x in (v, t, gv, gt))
        temp32 = temp.detach().reshape(1).float().contiguous()
        loss, sim_v2t, sim_t2v, lse = hip.vtc_loss_fwd(v, t, gv, gt, temp32, col0)
        ctx.save_for_backward(v, t, gv, gt, temp32, sim_v2t, sim_t2v, lse)
        ctx.col0 = col0
        ctx.mark_non_differentiable(sim_v2t, sim_t2v)
        ctx.set_materialize_grads(False)
        return loss, sim_v2t, sim_t2v

    @staticmethod
    def backward(ctx, dloss, _d1, _d2):
        if dloss is None:
            return (None,) * 6
        v, t, gv, gt, temp32, sim_v2t, sim_t2v, lse = ctx.saved_tensors
        dv, dt, dgv, dgt, dtemp = hip.vtc_loss_bwd(v, t, gv, gt, temp32, ctx.col0, sim_v2t, sim_t2v, lse, dloss, want_dtemp=ctx.needs_input_grad[4])
        return dv, dt, dgv, dgt, dtemp, None


class _VtcLossIds(torch.autograd.Function):
    """alpro_vtc_loss_ids as an autograd node: _VtcLoss with the pairs' video ids (ids (B,), gathered gids (G,), int64) -- every column that
    carries the row's id is a positive and the target is uniform over them.  The ids take no gradient."""

    @staticmethod
    def forward(ctx, v, t, gv, gt, temp, col0, ids, gids):
        v, t, gv, gt = (x.contiguous().float() for x in (v, t, gv, gt))
        temp32 = temp.detach().reshape(1).float().contiguous()
        ids, gids = ids.detach().contiguous(), gids.detach().contiguous()
        loss, sim_v2t, sim_t2v, lse = hip.vtc_loss_ids_fwd(v, t, gv, gt, temp32, ids, gids, col0)
        ctx.save_for_backward(v, t, gv, gt, temp32, sim_v2t, sim_t2v, lse, ids, gids)
        ctx.col0 = col0
        ctx.mark_non_differentiable(sim_v2t, sim_t2v)
        ctx.set_materialize_grads(False)
        return loss, sim_v2t, sim_t2v

    @staticmethod
    def backward(ctx, dloss, _d1, _d2):
        if dloss is None:
            return (None,) * 8
        v, t, gv, gt, temp32, sim_v2t, sim_t2v, lse, ids, gids = ctx.saved_tensors
        dv, dt, dgv, dgt, dtemp = hip.vtc_loss_ids_bwd(v, t, gv, gt, temp32, ids, gids, ctx.col0, sim_v2t, sim_t2v, lse, dloss,
                                                       want_dtemp=ctx.needs_input_grad[4])
        return dv, dt, dgv, dgt, dtemp, None, None, None


class AlproBaseModel(nn.Module):
    def __init__(self, config=None, input_format='RGB', video_enc_cfg=None, temp=0.07):
        super().__init__()
        self.temp = nn.Parameter(torch.ones([]) * temp)
        self.bert_config = config
        visual_model_cls = _VISUAL_CLASSES[video_enc_cfg['cls']]
        self.visual_encoder = visual_model_cls(model_cfg=video_enc_cfg, input_format=input_format, cross_attention_config=config)
        self.text_encoder = BertForMaskedLM.from_pretrained('bert-base-uncased', config=self.bert_config)
        embed_dim = 256
        vision_width = 768
        text_width = self.bert_config.hidden_size
        self.vision_proj = nn.Linear(vision_width, embed_dim)
        self.text_proj = nn.Linear(text_width, embed_dim)
        self.itc_token_type = self.bert_config.itc_token_type
        self.itm_head = nn.Linear(text_width, 2)

    def load_separate_ckpt(self, visual_weights_path=None, bert_weights_path=None):
        if visual_weights_path:
            self.visual_encoder.load_state_dict(visual_weights_path)

    # ---- shared pieces ---------------------------------------------------------------------------
    def _forward_visual_embeds(self, visual_inputs):
        """(B, T, C, H, W) -> (B, 1 + N, 768) (alpro_models.py:186-194)."""
        return self.visual_encoder.forward_features(visual_inputs.transpose(1, 2), return_all_tokens=True)

    def _text_embeds(self, input_ids, attention_mask):
        return self.text_encoder.bert(input_ids, attention_mask=attention_mask, return_dict=True, mode='text').last_hidden_state

    def _fusion(self, embeds, attention_mask):
        return self.text_encoder.bert(encoder_embeds=embeds, attention_mask=attention_mask, return_dict=True, mode='fusion').last_hidden_state

    def _video_feat(self, video_embeds):
        assert self.itc_token_type == 'cls', 'Support CLS tokens for ITC only, find {}.'.format(self.itc_token_type)
        return F.normalize(_linear32(video_embeds[:, 0, :], self.vision_proj), dim=-1)

    def _text_feat(self, text_embeds):
        return F.normalize(_linear32(text_embeds[:, 0, :], self.text_proj), dim=-1)

    def _vtc(self, video_feat, text_feat, ids=None):
        """In-batch video-text contrastive loss over the gathered features (alpro_models.py:109-128).  ids: the batch key `video_ids`, (B,) int64
        -- every gathered pair of the row's video is then a positive (the reference's FIXME, dataset_video_retrieval.py:101)."""
        b = video_feat.shape[0]
        gathered_video_feats = hvd.allgather(video_feat)
        gathered_text_feats = hvd.allgather(text_feat)
        b_start = b * hvd.local_rank()   # targets: eye(b) at columns [b_start, b_start + b) of the gathered similarity (:121-123)
        if ids is None:
            loss, sim_v2t, sim_t2v = _VtcLoss.apply(video_feat, text_feat, gathered_video_feats, gathered_text_feats, self.temp, b_start)
        else:
            ids = ids.to(device=video_feat.device, dtype=torch.long).reshape(b)
            loss, sim_v2t, sim_t2v = _VtcLossIds.apply(video_feat, text_feat, gathered_video_feats, gathered_text_feats, self.temp, b_start,
                                                       ids, hvd.allgather(ids))
        return loss, sim_v2t, sim_t2v, b_start

    @staticmethod
    def _sample_negatives(sim_v2t, sim_t2v, bs):
        """One hard negative video per text and one hard negative text per video, drawn from the softmax of the rank's own
        similarity block with the positives masked out (alpro_models.py:287-306)."""
        local_rank = hvd.local_rank()
        b_start, b_end = bs * local_rank, bs * (local_rank + 1)
        with torch.no_grad():
            weights_v2t = sim_v2t[:, b_start:b_end].detach().clone()
            weights_t2v = sim_t2v[:, b_start:b_end].detach().clone()
            weights_v2t.fill_diagonal_(-np.inf)
            weights_t2v.fill_diagonal_(-np.inf)
            weights_v2t = F.softmax(weights_v2t, dim=1)
            weights_t2v = F.softmax(weights_t2v, dim=1)
            neg_video = torch.multinomial(weights_t2v, 1).view(-1)  # a negative video for each text
            neg_text = torch.multinomial(weights_v2t, 1).view(-1)   # a negative text for each video
        return neg_video, neg_text

    @staticmethod
    def _sample_negatives_ids(sim_v2t, sim_t2v, bs, ids):
        """_sample_negatives where no pair of the row's own video can be drawn: the columns whose id equals the row's (ids (bs,) int64; a negative
        id equals nothing) are masked beside the diagonal.  A row that would lose every column (all local pairs from one video) keeps the
        diagonal-only mask.  With distinct ids the weights, and so the draws under one seed, are _sample_negatives'."""
        local_rank = hvd.local_rank()
        b_start, b_end = bs * local_rank, bs * (local_rank + 1)
        with torch.no_grad():
            ids = ids.reshape(bs).to(sim_v2t.device)
            eye = torch.eye(bs, dtype=torch.bool, device=ids.device)
            same = ((ids[:, None] == ids[None, :]) & (ids[:, None] >= 0)) | eye
            mask = torch.where(same.all(dim=1, keepdim=True), eye, same)
            weights_v2t = sim_v2t[:, b_start:b_end].detach().masked_fill(mask, -np.inf)
            weights_t2v = sim_t2v[:, b_start:b_end].detach().masked_fill(mask, -np.inf)
            weights_v2t = F.softmax(weights_v2t, dim=1)
            weights_t2v = F.softmax(weights_t2v, dim=1)
            neg_video = torch.multinomial(weights_t2v, 1).view(-1)  # a negative video for each text
            neg_text = torch.multinomial(weights_v2t, 1).view(-1)   # a negative text for each video
        return neg_video, neg_text

    def _vtm(self, text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v, cls_only=False, ids=None):
        """Video-text matching with in-batch hard negatives (alpro_models.py:269-344 / 800-872).
        cls_only: the caller reads nothing but the ITM logits (the retrieval model, alpro_models.py:800-872) -- the last fusion layer's row-wise tail then
        runs on the 3B [CLS] rows alone (BertLayer.forward_train rows=...; ALPRO_FUSION_TAIL_ROWS=0: every row) and `pos` is not returned."""
        device = text_embeds.device
        bs = text_embeds.shape[0]
        if ids is None:
            neg_video, neg_text = self._sample_negatives(sim_v2t, sim_t2v, bs)
        else:
            neg_video, neg_text = self._sample_negatives_ids(sim_v2t, sim_t2v, bs, ids)
        # positives and the 2B negatives as ONE 3B-sequence fusion batch (the reference makes two calls, :278 and :325; the
        # rows are independent, so the results are the same and the GEMM tiles are fuller)
        text_embeds_all = torch.cat([text_embeds, text_embeds, text_embeds[neg_text]], dim=0)
        text_atts_all = torch.cat([text_atts, text_atts, text_atts[neg_text]], dim=0)
        video_embeds_all = torch.cat([video_embeds, video_embeds[neg_video], video_embeds], dim=0)
        video_atts_all = torch.cat([video_atts, video_atts, video_atts], dim=0)
        bert = self.text_encoder.bert if hasattr(self.text_encoder, "bert") else self.text_encoder
        if cls_only and os.environ.get("ALPRO_FUSION_TAIL_ROWS", "1") != "0" and text_embeds.is_cuda:
            seq_len = text_embeds_all.shape[1] + video_embeds_all.shape[1]
            rows = torch.arange(3 * bs, device=device, dtype=torch.long) * seq_len
            vl_embeddings = bert(encoder_embeds=torch.cat([text_embeds_all, video_embeds_all], dim=1), attention_mask=torch.cat([text_atts_all, video_atts_all], dim=1),
                                 return_dict=True, mode='fusion', out_rows=rows).last_hidden_state
            pos = None
        else:
            both = self._fusion(torch.cat([text_embeds_all, video_embeds_all], dim=1), torch.cat([text_atts_all, video_atts_all], dim=1))
            pos, neg = both[:bs], both[bs:]
            vl_embeddings = torch.cat([pos[:, 0, :], neg[:, 0, :]], dim=0)
        vtm_logits = _linear32(vl_embeddings, self.itm_head)
        vtm_labels = torch.cat([torch.ones(bs, dtype=torch.long, device=device), torch.zeros(2 * bs, dtype=torch.long, device=device)], dim=0)   # built on the device: a pageable .to(device) makes the host wait for the launch stream
        vtm_loss = F.cross_entropy(vtm_logits, vtm_labels)
        return vtm_loss, vtm_logits, vtm_labels, pos


class AlproForPretrain(AlproBaseModel):
    def __init__(self, config, video_enc_cfg, input_format='RGB'):
        super().__init__(config, input_format=input_format, video_enc_cfg=video_enc_cfg)
        self.prompter = Prompter(config, video_enc_cfg)  # frozen teacher for pseudo labels
        self.use_mask_prob = 0
        self.batch_encoder_passes = True  # one 4B fusion pass / one 2B text pass instead of the reference's 3 / 2 calls
        # Round 6 (third session): the LAST fusion layer's row-wise tail (attention-output dense, LayerNorms, FFN) only on the rows the heads read -- the 3B
        # [CLS] rows, the MLM pairs' text rows, the positives' patch rows: 239 of every 948 rows of the 4B x 237 batch; nothing else of that layer's output
        # reaches a loss (alpro_models.py:283,331-338,366-371,215-218), forward or backward.  ALPRO_FUSION_TAIL_ROWS=0: every row, as before (A/B).
        self.fusion_tail_rows = os.environ.get("ALPRO_FUSION_TAIL_ROWS", "1") != "0"
        self._out_rows_cache = {}
        self.mpm_head = nn.Sequential(nn.Linear(config.hidden_size, config.hidden_size * 2), nn.ReLU(True),
                                      nn.Linear(config.hidden_size * 2, self.prompter.entity_num))

    def build_text_prompts(self, prompts):
        self.prompter.build_text_prompts(prompts)

    def _fusion_out_rows(self, b, txt_len, seq_len, device):
        """Flat row indices (into the 4B x seq_len rows of the fusion batch: positives | negative videos | negative texts | MLM pairs) of what the heads
        read: row 0 of the first 3B sequences (ITM), rows 0..txt_len-1 of the MLM pairs (LM head), rows txt_len+1.. of the positives (MPM: the patch
        tokens behind the video [CLS]).  Built once per geometry, on the device."""
        key = (b, txt_len, seq_len, str(device))
        idx = self._out_rows_cache.get(key)
        if idx is None:
            ar = lambda n: torch.arange(n, device=device, dtype=torch.long)
            cls_ = ar(3 * b) * seq_len
            mlm = ((3 * b + ar(b))[:, None] * seq_len + ar(txt_len)[None, :]).reshape(-1)
            vis = (ar(b)[:, None] * seq_len + (txt_len + 1 + ar(seq_len - txt_len - 1))[None, :]).reshape(-1)
            idx = self._out_rows_cache[key] = torch.cat([cls_, mlm, vis]).contiguous()
        return idx

    def get_pseudo_labels(self, batch):
        return self.prompter.get_pseudo_labels(batch)

    def forward(self, batch):
        with torch.no_grad():
            self.temp.clamp_(0.001, 0.5)
        visual_inputs = batch['visual_inputs']
        use_mpm = 'mpm_mask' in batch
        device = visual_inputs.device
        b = visual_inputs.shape[0]
        ids = batch.get('video_ids')   # optional (B,) int64: pairs of one video are positives of each other and never each other's hard negatives
        batched = 'mlm_labels' in batch and self.batch_encoder_passes
        from alpro_amd import config as rt
        text_side = rt.text_side_stream(device) if batched else None
        if text_side is not None:
            ev_inputs = torch.cuda.current_stream(device).record_event()   # everything the text pass reads (ids, masks, this step's operand mirrors) is older
        if use_mpm and np.random.uniform() < self.use_mask_prob:
            total = self._forward_visual_embeds(torch.cat([visual_inputs, batch['context_visual_inputs']], dim=0))
            video_embeds = total[:b]
        else:
            video_embeds = self._forward_visual_embeds(visual_inputs)
        text_atts = batch['text_input_mask']
        both = None
        if text_side is not None:
            # the 2B-caption text pass on its side stream (alpro_amd.config, ALPRO_TEXT_STREAM): queued BEHIND the visual encoder's launches on the host
            # (the visual anchor is the older autograd node, so the text backward still runs first and BERT's gradients can go on the wire early) but
            # ordered only behind `ev_inputs` on the device -- it runs beside the visual forward
            text_side.wait_event(ev_inputs)
            with torch.cuda.stream(text_side):
                both = self._text_embeds(torch.cat([batch['text_input_ids'], batch['mlm_text_input_ids']], dim=0), torch.cat([text_atts, text_atts], dim=0))
        pseudo = p_side = None
        if use_mpm:
            p_side = rt.prompter_side_stream(device)
            if p_side is not None:   # (alpro_amd.config, ALPRO_PROMPTER_STREAM) behind the visual forward, beside what the launch stream does from here on
                p_side.wait_stream(torch.cuda.current_stream(device))
                with torch.cuda.stream(p_side):
                    pseudo = self.get_pseudo_labels(batch)
        video_feat = self._video_feat(video_embeds)
        video_atts = torch.ones(video_embeds.size()[:-1], dtype=torch.long, device=device)
        pos_patch_rows = None
        if batched:
            # Same sequences through the same weights as the reference's three fusion calls (positive pairs :278, 2B negatives
            # :325, MLM pairs :360) and two text-encoder calls (:99, :354), but as ONE 4B-sequence fusion batch and ONE
            # 2B-caption text batch: every row of a BERT layer is independent of the batch it sits in, and M = 4B*237 fills
            # the 256x256 GEMM tiles far better than 3 launches at B / 2B / B.
            if both is None:
                both = self._text_embeds(torch.cat([batch['text_input_ids'], batch['mlm_text_input_ids']], dim=0), torch.cat([text_atts, text_atts], dim=0))
            else:
                torch.cuda.current_stream(device).wait_stream(text_side)
                both.record_stream(torch.cuda.current_stream(device))   # allocated on the side stream, read (and possibly outlived) on this one
            text_feat = self._text_feat(both[:b])
            if ids is None:
                vtc_loss, sim_v2t, sim_t2v, _ = self._vtc(video_feat, text_feat)
                neg_video, neg_text = self._sample_negatives(sim_v2t, sim_t2v, b)
            else:
                vtc_loss, sim_v2t, sim_t2v, _ = self._vtc(video_feat, text_feat, ids=ids)
                neg_video, neg_text = self._sample_negatives_ids(sim_v2t, sim_t2v, b, ids)
            ta_all = torch.cat([text_atts, text_atts, text_atts[neg_text], text_atts], dim=0)
            va_all = torch.cat([video_atts] * 4, dim=0)
            # sequence s of the 4B fusion batch = [text pool row ti[s] ; video pool row vi[s]] over the pools (both = [captions ; masked captions],
            # video_embeds): positives, negative videos, negative texts, MLM pairs -- the rows the reference's cats hold, never materialised by torch
            ar = torch.arange(b, device=device)
            ti = torch.cat([ar, ar, neg_text, ar + b])
            vi = torch.cat([ar, neg_video, ar, ar])
            txt_len, seq_len = text_atts.shape[1], text_atts.shape[1] + video_embeds.shape[1]
            rows = self._fusion_out_rows(b, txt_len, seq_len, device) if (use_mpm and self.fusion_tail_rows) else None
            fused = self.text_encoder.bert(encoder_embeds_parts=(both, video_embeds, ti, vi), attention_mask=torch.cat([ta_all, va_all], dim=1), return_dict=True,
                                           mode='fusion', out_rows=rows).last_hidden_state
            if rows is not None:
                # `fused` holds only the rows the heads read, in this order (see _fusion_out_rows): 3B [CLS] rows | B x txt_len MLM text rows | B x N patch rows
                n_cls, n_mlm = 3 * b, b * txt_len
                cls_rows, mlm_rows = fused[:n_cls], fused[n_cls:n_cls + n_mlm].view(b, txt_len, -1)
                pos_patch_rows = fused[n_cls + n_mlm:].view(b, -1, fused.shape[-1])
                encoder_outputs_pos = None
            elif use_mpm:
                cls_rows, mlm_rows, pos_patch_rows = _FusionOutputs.apply(fused, b, txt_len)
                encoder_outputs_pos = None
            else:
                encoder_outputs_pos, neg, mlm_out = fused[:b], fused[b:3 * b], fused[3 * b:]
                cls_rows, mlm_rows, pos_patch_rows = torch.cat([encoder_outputs_pos[:, 0, :], neg[:, 0, :]], dim=0), mlm_out[:, :txt_len], None
            vtm_logits = _linear32(cls_rows, self.itm_head)
            # built on the device: `.to(device)` of a pageable host tensor makes the host wait for everything queued on the launch stream (both encoders'
            # forwards), after which the device idles until the next launches arrive (tools/sync_probe.py found this one; the reference has the same line, :327)
            vtm_labels = torch.cat([torch.ones(b, dtype=torch.long, device=device), torch.zeros(2 * b, dtype=torch.long, device=device)], dim=0)
            vtm_loss = F.cross_entropy(vtm_logits, vtm_labels)
            mlm_labels = batch['mlm_labels']
            mlm_logits, mlm_loss = self.text_encoder.cls.predictions.forward_with_loss(mlm_rows, mlm_labels)
        else:
            text_embeds = self._text_embeds(batch['text_input_ids'], text_atts)
            text_feat = self._text_feat(text_embeds)
            if ids is None:
                vtc_loss, sim_v2t, sim_t2v, _ = self._vtc(video_feat, text_feat)
                vtm_loss, vtm_logits, vtm_labels, encoder_outputs_pos = self._vtm(text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v)
            else:
                vtc_loss, sim_v2t, sim_t2v, _ = self._vtc(video_feat, text_feat, ids=ids)
                vtm_loss, vtm_logits, vtm_labels, encoder_outputs_pos = self._vtm(text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v, ids=ids)
            if 'mlm_labels' in batch:
                mlm_loss, mlm_logits, mlm_labels = self.compute_mlm(batch['mlm_text_input_ids'], text_atts, video_embeds, video_atts, batch['mlm_labels'])
            else:
                mlm_logits = mlm_loss = mlm_labels = None
        if use_mpm:
            if pseudo is None:
                mpm_labels, ignore_masks = self.get_pseudo_labels(batch)
            else:
                torch.cuda.current_stream(device).wait_stream(p_side)
                mpm_labels, ignore_masks = pseudo
                for t_ in pseudo:
                    t_.record_stream(torch.cuda.current_stream(device))
            mpm_loss, mpm_logits = self.compute_mpm_with_encoder_out(encoder_outputs_pos, text_atts, mpm_labels, ignore_masks, batch['mpm_mask'], visual_output=pos_patch_rows)
        else:
            mpm_loss = mpm_logits = mpm_labels = None
        return dict(itc_loss=vtc_loss, mlm_scores=mlm_logits, mlm_loss=mlm_loss, mlm_labels=mlm_labels, itm_scores=vtm_logits,
                    itm_loss=vtm_loss, itm_labels=vtm_labels, mpm_loss=mpm_loss, mpm_logits=mpm_logits, mpm_labels=mpm_labels)

    def _forward_text_feats(self, batch):
        text_embeds = self._text_embeds(batch['text_input_ids'], batch['text_input_mask'])
        return text_embeds, self._text_feat(text_embeds)

    def compute_vtm(self, text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v, return_encoder_out=False):
        loss, logits, labels, pos = self._vtm(text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v)
        return loss, logits, labels, (pos if return_encoder_out else None)

    def compute_mlm(self, input_ids, text_input_mask, video_embeds, video_atts, mlm_labels):
        """alpro_models.py:346-373."""
        text_embeds = self._text_embeds(input_ids, text_input_mask)
        out = self._fusion(torch.cat([text_embeds, video_embeds], dim=1), torch.cat([text_input_mask, video_atts], dim=1))
        txt_len = text_input_mask.shape[1]
        mlm_logits, mlm_loss = self.text_encoder.cls.predictions.forward_with_loss(out[:, :txt_len], mlm_labels)
        return mlm_loss, mlm_logits, mlm_labels

    def compute_mpm_with_encoder_out(self, encoder_outputs, text_atts, soft_labels, ignore_masks, patch_masks, visual_output=None):
        """alpro_models.py:209-232 (encoder_outputs: last_hidden_state tensor of the positive fusion pass; visual_output: its patch rows
        [:, txt_len + 1:] when the caller has cut them out already)."""
        if visual_output is None:
            hidden = encoder_outputs.last_hidden_state if hasattr(encoder_outputs, "last_hidden_state") else encoder_outputs
            txt_len = text_atts.shape[1]
            visual_output = hidden[:, txt_len + 1:]
        bsz = patch_masks.shape[0]
        inv = (1 - patch_masks.view(bsz, -1)).unsqueeze(-1)
        num_masked = torch.sum(inv.squeeze(-1), dim=-1, keepdim=True)
        emb = torch.sum(inv * visual_output, dim=1) / num_masked
        h = F.relu(_linear32(emb, self.mpm_head[0]))
        mpm_logits = _linear32(h, self.mpm_head[2])
        ce = -torch.sum(F.log_softmax(mpm_logits, dim=1) * soft_labels, dim=1)
        ce = torch.where(ignore_masks, torch.zeros_like(ce), ce)
        return torch.sum(ce) / (bsz - torch.sum(ignore_masks)), mpm_logits

    def load_separate_ckpt(self, visual_weights_path=None, bert_weights_path=None, prompter_weights_path=None):
        if visual_weights_path:
            self.visual_encoder.load_state_dict(visual_weights_path)
        if prompter_weights_path is not None:
            self.prompter.load_pretrained_weights_without_prompts(prompter_weights_path)


class Prompter(AlproBaseModel):
    def __init__(self, config, video_enc_cfg, input_format='RGB'):
        super().__init__(config, input_format=input_format, video_enc_cfg=video_enc_cfg)
        self.entity_num = config.num_entities
        self.register_buffer("video_prompt_feat", torch.rand(self.entity_num, 256))
        self.register_buffer("image_prompt_feat", torch.rand(self.entity_num, 256))
        self.prompt_initialized = False
        self.ignore_threshold = 0.2

    def load_pretrained_weights_without_prompts(self, ckpt_path):
        sd = torch.load(ckpt_path, map_location='cpu')
        self.load_state_dict({k: v for k, v in sd.items() if 'prompt_feat' not in k}, strict=False)

    def _prompt_feats(self, enc, step_size=10000):
        feats = []
        ids, mask = enc.input_ids, enc.attention_mask
        dev = self.temp.device
        for s in range(0, ids.shape[0], step_size):
            emb = self._text_embeds(ids[s:s + step_size].to(dev), mask[s:s + step_size].to(dev))
            feats.append(self._text_feat(emb))
        feat = torch.cat(feats, dim=0)
        n_templates = int(feat.shape[0] / self.entity_num)
        return torch.mean(torch.stack(feat.chunk(n_templates), dim=1), dim=1)

    def build_text_prompts(self, prompts):
        """alpro_models.py:430-507: encode entity prompts, average over templates."""
        assert not self.prompt_initialized, "Repetitively building prompts?"
        if self.training:
            self.eval()
        with torch.no_grad():
            self.video_prompt_feat = self._prompt_feats(prompts['batch_enc_video_prompts'])
            self.image_prompt_feat = self._prompt_feats(prompts['batch_enc_image_prompts'])
        self.prompt_initialized = True

    def _forward_visual_embeds(self, visual_inputs):
        video_embeds = super()._forward_visual_embeds(visual_inputs)
        return video_embeds, self._video_feat(video_embeds)

    def _compute_soft_labels(self, sim_vp_masked):
        soft_labels = nn.Softmax(dim=1)(sim_vp_masked)
        ignore_masks = torch.max(sim_vp_masked, dim=1)[1] < self.ignore_threshold  # sic: argmax index (alpro_models.py:527)
        return soft_labels, ignore_masks

    def get_pseudo_labels(self, batch):
        if self.training:
            self.eval()
        from alpro_amd import config as rt
        with torch.no_grad(), rt.cls_precise_off():   # (soft labels, not VTC logits of the trained model: the plain 16-bit pass)
            if hasattr(self.visual_encoder, "forward_cls"):  # only the CLS feature is consumed: CLS-only tail of the last block
                cls = self.visual_encoder.forward_cls(batch['crop_visual_inputs'].transpose(1, 2))
                feat = F.normalize(_linear32(cls, self.vision_proj), dim=-1)
            else:
                _, feat = self._forward_visual_embeds(batch['crop_visual_inputs'])
            prompt_feat = self.video_prompt_feat if batch['type'] == 'video' else self.image_prompt_feat
            sim_masked = feat @ prompt_feat.t() / self.temp
            return self._compute_soft_labels(sim_masked)

    def forward_feats(self, batch):
        with torch.no_grad():
            self.temp.clamp_(0.001, 0.5)
        video_embeds, video_feat = self._forward_visual_embeds(batch['visual_inputs'])
        text_embeds = self._text_embeds(batch['text_input_ids'], batch['text_input_mask'])
        return video_embeds, video_feat, text_embeds, self._text_feat(text_embeds)

    def forward(self, batch):
        _, video_feat, _, text_feat = self.forward_feats(batch)
        ids = batch.get('video_ids')
        vtc_loss, sim_v2t, sim_t2v, b_start = self._vtc(video_feat, text_feat) if ids is None else self._vtc(video_feat, text_feat, ids=ids)
        itc_labels = b_start + torch.arange(video_feat.shape[0], device=sim_v2t.device)   # == max(sim_targets, 1)[1] (:589)
        return dict(itc_loss=vtc_loss, itc_labels=itc_labels,
                    i2t_scores=F.log_softmax(sim_v2t, dim=1), t2i_scores=F.log_softmax(sim_t2v, dim=1))


class AlproForVideoTextRetrieval(AlproBaseModel):
    def __init__(self, config, video_enc_cfg, input_format='RGB'):
        super().__init__(config, input_format=input_format, video_enc_cfg=video_enc_cfg)

    def forward(self, batch):
        with torch.no_grad():
            self.temp.clamp_(0.001, 0.5)
        visual_inputs, text_atts = batch['visual_inputs'], batch['text_input_mask']
        video_embeds = self._forward_visual_embeds(visual_inputs)
        video_feat = self._video_feat(video_embeds)
        video_atts = torch.ones(video_embeds.size()[:-1], dtype=torch.long, device=visual_inputs.device)
        text_embeds = self._text_embeds(batch['text_input_ids'], text_atts)
        text_feat = self._text_feat(text_embeds)
        ids = batch.get('video_ids')   # optional (B,) int64, see AlproForPretrain.forward
        if ids is None:
            vtc_loss, sim_v2t, sim_t2v, _ = self._vtc(video_feat, text_feat)
            vtm_loss, vtm_logits, vtm_labels, _ = self._vtm(text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v, cls_only=True)
        else:
            vtc_loss, sim_v2t, sim_t2v, _ = self._vtc(video_feat, text_feat, ids=ids)
            vtm_loss, vtm_logits, vtm_labels, _ = self._vtm(text_embeds, text_atts, video_embeds, video_atts, sim_v2t, sim_t2v, cls_only=True, ids=ids)
        return dict(itm_scores=vtm_logits, itm_loss=vtm_loss, itm_labels=vtm_labels, itc_loss=vtc_loss)

    def compute_vtm(self, text_embeds, text_atts, image_embeds, image_atts, sim_i2t, sim_t2i):
        return self._vtm(text_embeds, text_atts, image_embeds, image_atts, sim_i2t, sim_t2i)[:3]

    def forward_inference(self, batch):
        """One video against n captions (alpro_models.py:874-914)."""
        visual_inputs, text_input_mask = batch['visual_inputs'], batch['text_input_mask']
        video_embeds = self._forward_visual_embeds(visual_inputs)
        video_feat = self._video_feat(video_embeds)
        video_embeds = video_embeds.repeat(text_input_mask.shape[0], 1, 1)
        video_atts = torch.ones(video_embeds.size()[:-1], dtype=torch.long, device=visual_inputs.device)
        text_embeds = self._text_embeds(batch['text_input_ids'], text_input_mask)
        text_feat = self._text_feat(text_embeds)
        vtc_sim_scores = video_feat @ text_feat.t() / self.temp
        out = self._fusion(torch.cat([text_embeds, video_embeds], dim=1), torch.cat([text_input_mask, video_atts], dim=1))
        return dict(logits=_linear32(out[:, 0, :], self.itm_head), itc_scores=vtc_sim_scores)

    # ---- retrieval evaluation with cached encoders.  The reference's eval loop
    # (run_video_retrieval.py:642-690) calls forward_inference once per (video, caption mini-batch): the ViT runs
    # #mini-batches times per video and the text encoder #videos times per caption.  The three methods below split
    # forward_inference at its natural seams so a caller encodes every video and every caption ONCE and only the fusion
    # pass runs per pair; alpro_amd/retrieval_eval.py drives them and reproduces the reference's result records.
    @torch.no_grad()
    def encode_video(self, visual_inputs):
        """(1, T, C, H, W) -> (video_embeds (1, 1+N, D), video_feat (1, 256))."""
        video_embeds = self._forward_visual_embeds(visual_inputs)
        return video_embeds, self._video_feat(video_embeds)

    @torch.no_grad()
    def encode_text(self, text_input_ids, text_input_mask):
        """(n, Lt) -> (text_embeds (n, Lt, D), text_feat (n, 256))."""
        text_embeds = self._text_embeds(text_input_ids, text_input_mask)
        return text_embeds, self._text_feat(text_embeds)

    @torch.no_grad()
    def score_pairs(self, video_embeds, video_feat, text_embeds, text_feat, text_input_mask):
        """One cached video against n cached captions: the tail of forward_inference (alpro_models.py:893-914)."""
        n = text_embeds.shape[0]
        ve = video_embeds.repeat(n, 1, 1)
        video_atts = torch.ones(ve.size()[:-1], dtype=torch.long, device=ve.device)
        out = self._fusion(torch.cat([text_embeds, ve], dim=1), torch.cat([text_input_mask, video_atts], dim=1))
        return dict(logits=_linear32(out[:, 0, :], self.itm_head), itc_scores=video_feat @ text_feat.t() / self.temp)

    @torch.no_grad()
    def score_pair_list(self, video_embeds, text_embeds, text_input_mask, vi, ci):
        """ITM logits (S, 2) fp32 of S listed (video, caption) pairs over cached encoder outputs -- stage 2 of the two-stage search
        (alpro_amd/retrieval_eval.py rerank_retrieval): sequence s = [text_embeds[ci[s]] ; video_embeds[vi[s]]] (vi, ci (S,) int64 on the device),
        gathered by alpro_gather_seq_fwd (BertModel.forward encoder_embeds_parts), never repeated or concatenated; the last fusion layer's row-wise
        tail runs on the S [CLS] rows alone, as in AlproForSequenceClassification.answer_logits (ALPRO_FUSION_TAIL_ROWS=0: every row).  Evaluation
        only: the model must be in eval mode (no dropout, no RNG draw)."""
        if self.training:
            raise RuntimeError("score_pair_list scores cached features for evaluation: call model.eval() first")
        S, Lt = vi.numel(), text_embeds.shape[1]
        L = Lt + video_embeds.shape[1]
        att = torch.ones((S, L), dtype=text_input_mask.dtype, device=text_input_mask.device)
        att[:, :Lt] = text_input_mask[ci]
        tail = os.environ.get("ALPRO_FUSION_TAIL_ROWS", "1") != "0" and text_embeds.is_cuda
        rows = torch.arange(S, device=vi.device, dtype=torch.long) * L if tail else None
        out = self.text_encoder.bert(encoder_embeds_parts=(text_embeds, video_embeds, ci, vi), attention_mask=att, return_dict=True, mode='fusion',
                                     out_rows=rows).last_hidden_state
        return _linear32(out if rows is not None else out[:, 0, :], self.itm_head).float()


_HEAD_ROW_CHUNK = 512   # alpro_gemm_rows_f32 is sized for a handful of rows (_rows_ok): multi-clip evaluation's B * C rows run in chunks of this many


class _QAHead(torch.autograd.Function):
    """The VideoQA answer MLP and its loss (alpro_models.py:639-643,680-683) as one node, fp32 throughout:
        H = relu(X W1^T + b1)   alpro_gemm_rows_f32, act = ReLU
        Z = H W2^T + b2         alpro_gemm_rows_f32, any num_labels (the last 16-column tile is masked)
        loss_rows = CE(Z, y)    alpro_softmax_xent, which also writes softmax(Z) - onehot(y) for the backward
    Backward: dZ = (softmax - onehot) * d(loss_rows) [+ d(logits)], dH = (dZ W2) * [H > 0] (alpro_gemm_rows_f32_relu_mask on the saved H),
    dX = dH W1, weight gradients as the small NT products of _Linear32.  Z lives in a (M, A rounded up to 64) buffer: `logits` is its
    first A columns (rows 8-byte aligned for softmax_xent at any A; the zero-padded gradient feeds the next K-contraction directly)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, labels):
        M, A = x.shape[0], w2.shape[0]
        Ap = (A + 63) // 64 * 64
        w1_, w2_ = w1.detach().contiguous(), w2.detach().contiguous()
        h = torch.empty((M, w1.shape[0]), dtype=torch.float32, device=x.device)
        z = torch.empty((M, Ap), dtype=torch.float32, device=x.device)
        logits = z[:, :A]
        for r in range(0, M, _HEAD_ROW_CHUNK):
            s = slice(r, min(M, r + _HEAD_ROW_CHUNK))
            hip.gemm_rows(x[s], w1_, bias=b1.detach(), act=hip.ACT_RELU, out=h[s])
            hip.gemm_rows(h[s], w2_, bias=b2.detach(), out=logits[s])
        dl = None
        if labels is None:
            loss_rows = torch.zeros(M, dtype=torch.float32, device=x.device)
            ctx.mark_non_differentiable(loss_rows)
        elif any(ctx.needs_input_grad[:5]):
            one = torch.ones(1, dtype=torch.float32, device=x.device)
            loss_rows, dl = hip.softmax_xent(logits, labels, grad_dtype=torch.float32, grad_scale=one)   # dl: (M, Ap), zero past column A
        else:
            loss_rows = hip.softmax_xent(logits, labels)
        ctx.save_for_backward(x, w1, w2, h, dl)
        ctx.set_materialize_grads(False)
        return logits, loss_rows

    @staticmethod
    def backward(ctx, dlogits, dloss_rows):
        x, w1, w2, h, dl = ctx.saved_tensors
        M, A = x.shape[0], w2.shape[0]
        Ap = (A + 63) // 64 * 64
        if dl is not None and dloss_rows is not None:
            g = dl * dloss_rows.reshape(M, 1)
        else:
            g = torch.zeros((M, Ap), dtype=torch.float32, device=x.device)
        if dlogits is not None:
            g[:, :A] += dlogits
        w2t = _pad_k(w2.detach().t().contiguous(), 64)                     # (hidden, Ap): the contraction over the labels, zero-padded like g
        dh = torch.empty_like(h)
        for r in range(0, M, _HEAD_ROW_CHUNK):
            s = slice(r, min(M, r + _HEAD_ROW_CHUNK))
            hip.gemm_rows_relu_mask(g[s], w2t, h[s], out=dh[s])
        dx = None
        if ctx.needs_input_grad[0]:
            w1t = w1.detach().t().contiguous()
            dx = torch.empty_like(x)
            for r in range(0, M, _HEAD_ROW_CHUNK):
                s = slice(r, min(M, r + _HEAD_ROW_CHUNK))
                hip.gemm_rows(dh[s], w1t, out=dx[s])
        gz = g[:, :A]
        dw2 = hip.gemm(_pad_k(gz.t().contiguous()), _pad_k(h.t().contiguous()), out_dtype=torch.float32) if ctx.needs_input_grad[3] else None
        db2 = gz.sum(0) if ctx.needs_input_grad[4] else None
        dw1 = hip.gemm(_pad_k(dh.t().contiguous()), _pad_k(x.t().contiguous()), out_dtype=torch.float32) if ctx.needs_input_grad[1] else None
        db1 = dh.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw1, db1, dw2, db2, None


class AlproForSequenceClassification(AlproBaseModel):
    """VideoQA model (alpro_models.py:633-724, driven by run_video_qa.py): the encoders + an MLP classifier over the fusion [CLS] row.
    Same constructor, forward(batch) -> dict(loss, logits) and state_dict keys as the reference; results differ by fp32 rounding order only.
      * the fusion input is a row gather of the text and video sequences (alpro_gather_seq_*), not a torch.cat;
      * the last fusion layer's row-wise tail runs on the B [CLS] rows only -- the classifier reads nothing else (ALPRO_FUSION_TAIL_ROWS=0:
        every row, for A/B);
      * the answer MLP and its cross-entropy are one fp32 node on the row kernel (_QAHead).
    encode_questions / encode_clips / answer_logits split forward at its seams so that multi-clip evaluation (alpro_amd/qa_eval.py) encodes
    each question once and each clip once."""

    def __init__(self, config, video_enc_cfg, input_format='RGB'):
        super().__init__(config, video_enc_cfg=video_enc_cfg)
        self.text_encoder = BertModel.from_pretrained('bert-base-uncased', config=self.bert_config, add_pooling_layer=False)
        self.classifier = nn.Sequential(nn.Linear(config.hidden_size, config.hidden_size * 2), nn.ReLU(True),
                                        nn.Linear(config.hidden_size * 2, config.num_labels))
        self.fusion_tail_rows = os.environ.get("ALPRO_FUSION_TAIL_ROWS", "1") != "0"

    def _text_embeds(self, input_ids, attention_mask):
        return self.text_encoder(input_ids, attention_mask=attention_mask, return_dict=True, mode='text').last_hidden_state

    def _fusion(self, embeds, attention_mask):
        return self.text_encoder(encoder_embeds=embeds, attention_mask=attention_mask, return_dict=True, mode='fusion').last_hidden_state

    def encode_questions(self, text_input_ids, text_input_mask):
        """(n, Lt) -> text encoder output (n, Lt, D) fp32."""
        return self._text_embeds(text_input_ids, text_input_mask)

    def encode_clips(self, visual_inputs):
        """(n, T, C, H, W) clips -> visual encoder output (n, 1 + N, D) fp32."""
        return self._forward_visual_embeds(visual_inputs)

    def answer_logits(self, text_embeds, text_input_mask, video_embeds, ti, vi, labels=None):
        """Fusion + answer MLP over S (question, clip) pairs: sequence s = [text_embeds[ti[s]] ; video_embeds[vi[s]]] (ti, vi (S,) int64 on
        the device; the rows are gathered, never repeated) -> (logits (S, num_labels) fp32, per-pair cross-entropy (S,); zeros if labels is None)."""
        S, Lt = ti.numel(), text_embeds.shape[1]
        L = Lt + video_embeds.shape[1]
        att = torch.ones((S, L), dtype=text_input_mask.dtype, device=text_input_mask.device)
        att[:, :Lt] = text_input_mask[ti]
        bert = self.text_encoder
        tail = self.fusion_tail_rows and text_embeds.is_cuda
        rows = torch.arange(S, device=ti.device, dtype=torch.long) * L if tail else None
        out = bert(encoder_embeds_parts=(text_embeds, video_embeds, ti, vi), attention_mask=att, return_dict=True, mode='fusion',
                   out_rows=rows).last_hidden_state
        cls_rows = (out if rows is not None else out[:, 0, :]).contiguous().float()
        if labels is not None:
            labels = labels.contiguous()
        return _QAHead.apply(cls_rows, self.classifier[0].weight, self.classifier[0].bias, self.classifier[2].weight, self.classifier[2].bias, labels)

    def _logits(self, batch, labels=None):
        visual_inputs, mask = batch['visual_inputs'], batch['text_input_mask']
        text_embeds = self.encode_questions(batch['text_input_ids'], mask)
        video_embeds = self.encode_clips(visual_inputs)
        idx = torch.arange(visual_inputs.shape[0], device=visual_inputs.device)
        return self.answer_logits(text_embeds, mask, video_embeds, idx, idx, labels)

    def forward(self, batch):
        targets = batch['labels']
        prediction, loss_rows = self._logits(batch, targets)
        return dict(loss=loss_rows.mean() if targets is not None else 0, logits=prediction)

    def forward_inference(self, batch):
        """-> logits, equal to forward(batch)['logits'].  The reference's version (alpro_models.py:686-724) calls self.text_encoder.bert on
        a BertModel and raises AttributeError; this is the computation it evidently intends."""
        return self._logits(batch)[0]
