"""Text-video retrieval evaluation on cached encoder outputs.

Same result records and metrics as the reference's `inference_retrieval` / `eval_retrieval`
(src/tasks/run_video_retrieval.py:515-690), but every video goes through the visual encoder once and every caption through the
text encoder once; only the fusion pass + ITM head runs per (video, caption) pair, in mini-batches.  For V videos x C captions
with mini-batches of b captions the reference runs the ViT V*ceil(C/b) times and the text encoder on V*C captions.

Beside the reference's all-pairs evaluation: a two-stage search over the same cached features (rerank_retrieval / rerank_metrics: the k best
candidates per query by the contrastive features through hip.sim_topk, fusion + ITM on those only), for galleries where V*C passes are too many.

Several clips per video (the reference's inference_n_clips / score_agg_func, config.py:99,190): visual_inputs carries num_clips * num_frm frames,
clip j of a video is scored like a video of its own -- x_j = its ITC similarity / temp, l_j = its two ITM logits -- and both are pooled
elementwise over j by mean / max / lse with the rule of run_video_qa.py:269-279 (hip.clip_pool); score = softmax(pooled logits)[1], sim =
pooled x.  The reference's retrieval loop collects the per-clip logits (run_video_retrieval.py:663-675) and then squeezes the clip axis, which
only works for one clip; its QA loop still has the pooling, and that is the definition here.  With one clip every function does what it did.
"""
import math
from collections import defaultdict

import numpy as np
import torch

SCORE_AGG_FUNCS = ("mean", "max", "lse")   # hip.POOL_MODES (run_video_qa.py:259-268)


def _check_clips(num_clips, score_agg_func):
    if score_agg_func not in SCORE_AGG_FUNCS:   # qa_eval.inference_qa's text (run_video_qa.py:279)
        raise ValueError("Invalid value for pool_method, got %s, expect one of [`mean`, `max`, `lse`]" % score_agg_func)
    if int(num_clips) < 1:
        raise ValueError("num_clips=%r clips per video (need >= 1)" % (num_clips,))


def _pool_clips(x, num_clips, score_agg_func):
    """x (G * num_clips, A), rows group-major (g * num_clips + j) -> (G, A) fp32 pooled over j by hip.clip_pool; one clip: x itself, untouched"""
    if num_clips == 1:
        return x.float()
    from alpro_amd import hip
    return hip.clip_pool(x.float().contiguous(), num_clips, score_agg_func)[0]


@torch.no_grad()
def inference_retrieval_cached(model, videos, text_input_ids, text_input_mask, caption_ids, eval_bsz=64, num_clips=1, score_agg_func="mean"):
    """videos: iterable of (vid_id, visual_inputs (1, num_clips*num_frm, C, H, W)); the captions are shared by all videos
    (each reference batch carries one video and all captions).  Returns the reference's list of
    dict(vid_id, txt_id, score, sim): score = softmax(itm logits)[:, 1], sim = ITC similarity, both rounded to 4 decimals; with
    num_clips > 1 the logits and the similarities are pooled over the clips by score_agg_func first (module docstring)."""
    _check_clips(num_clips, score_agg_func)
    model.eval()
    n = text_input_ids.shape[0]
    text_cache = []
    for i in range(0, n, eval_bsz):
        ids, mask = text_input_ids[i:i + eval_bsz], text_input_mask[i:i + eval_bsz]
        emb, feat = model.encode_text(ids, mask)
        text_cache.append((emb, feat, mask, caption_ids[i:i + eval_bsz]))
    res = []
    for vid_id, visual_inputs in videos:
        T = visual_inputs.shape[1] // num_clips
        ve, vf = model.encode_video(visual_inputs.view((num_clips, T) + tuple(visual_inputs.shape[2:])))   # the clips as a batch: (n, 1+N, D), (n, 256)
        for emb, feat, mask, cids in text_cache:
            outs = [model.score_pairs(ve[j:j + 1], vf[j:j + 1], emb, feat, mask) for j in range(num_clips)]   # one pass per clip, as the reference's loop
            logits = torch.stack([o["logits"].float() for o in outs], dim=1).reshape(-1, 2)                    # rows caption-major: c * n + j
            probs = torch.softmax(_pool_clips(logits, num_clips, score_agg_func), dim=1)[:, 1].tolist()
            sims = _pool_clips(torch.cat([o["itc_scores"].float().reshape(1, -1) for o in outs], 0), num_clips, score_agg_func).reshape(-1).tolist()
            for cid, sc, sim in zip(cids, probs, sims):
                res.append(dict(vid_id=vid_id, txt_id=cid, score=round(sc, 4), sim=round(sim, 4)))
    return res


def _split_clips(videos, num_clips):
    """(V, n*T, C, H, W), or an iterable of (1, n*T, C, H, W), -> the clips as a batch (V*n, T, C, H, W), row v * n + j"""
    v = videos if torch.is_tensor(videos) else torch.cat(list(videos), 0)
    if num_clips == 1:
        return v
    if v.shape[1] % num_clips:
        raise ValueError("visual_inputs carries %d frames per video: not a whole number of num_clips=%d clips" % (v.shape[1], num_clips))
    return v.reshape((v.shape[0] * num_clips, v.shape[1] // num_clips) + tuple(v.shape[2:]))


@torch.no_grad()
def score_all_pairs(model, videos, text_input_ids, text_input_mask, pair_bsz=512, text_bsz=1024, num_clips=1, score_agg_func="mean"):
    """Every caption against every video with nothing leaving the device: videos (V, T, C, H, W) or an iterable of (1, T, C, H, W)
    clips, captions (C, Lt).  Each video / caption is encoded ONCE; the V*C fusion passes run in flat mini-batches of `pair_bsz`
    (video, caption) pairs gathered from the two caches -- the GEMMs see M = pair_bsz * 237 rows whatever V and C are, where the
    reference loop (run_video_retrieval.py:642-690) runs one video x eval_bsz captions at a time.
    num_clips = n > 1: videos (V, n*T, ...); the fusion passes run over the (pair, clip) sequences, pair_bsz SEQUENCES at a time (whole
    pairs: max(1, pair_bsz // n) of them), the logits are pooled over the clips (rows pair-major) and the (V*n, C) similarities likewise,
    both by hip.clip_pool (module docstring).
    Returns (score (V, C) = softmax(itm_logits)[:, 1], sim (V, C) = ITC similarity), fp32 device tensors (unrounded)."""
    _check_clips(num_clips, score_agg_func)
    from alpro_amd.modeling.alpro_models import _linear32
    n = int(num_clips)
    ve, vf = encode_gallery(model, videos, 8, n)                                    # (V*n, 1+N, D), (V*n, 256)
    te, tf = encode_captions(model, text_input_ids, text_input_mask, text_bsz)      # (C, Lt, D), (C, 256)
    V, C = ve.shape[0] // n, te.shape[0]
    sim = _pool_clips(vf @ tf.t() / model.temp, n, score_agg_func)                  # (V*n, C) is clip_pool's layout with A = C
    score = torch.empty(V * C, dtype=torch.float32, device=ve.device)
    ones = torch.ones(ve.shape[:2], dtype=text_input_mask.dtype, device=ve.device)
    step = max(1, pair_bsz // n)
    clip = torch.arange(n, device=ve.device)
    for s in range(0, V * C, step):
        idx = torch.arange(s, min(V * C, s + step), device=ve.device)
        vi, ci = idx // C, idx % C
        if n > 1:                                                                   # sequence p * n + j: caption ci[p] with clip j of video vi[p]
            vi, ci = (vi[:, None] * n + clip).reshape(-1), ci.repeat_interleave(n)
        out = model._fusion(torch.cat([te[ci], ve[vi]], dim=1), torch.cat([text_input_mask[ci], ones[vi]], dim=1))
        logits = _pool_clips(_linear32(out[:, 0, :], model.itm_head), n, score_agg_func)
        score[s:s + idx.numel()] = torch.softmax(logits, dim=1)[:, 1]
    return score.view(V, C), sim


@torch.no_grad()
def encode_gallery(model, videos, bsz=8, num_clips=1):
    """Every clip through the visual encoder once, `bsz` at a time: videos (V, n*T, C, H, W) or an iterable of (1, n*T, C, H, W), n = num_clips
    clips of T frames each -> (video_embeds (V*n, 1+N, D), video_feat (V*n, 256)), row v * n + j, device tensors."""
    model.eval()
    clips = _split_clips(videos, int(num_clips))
    ve, vf = [], []
    for i in range(0, clips.shape[0], bsz):
        e, f = model.encode_video(clips[i:i + bsz])
        ve.append(e)
        vf.append(f)
    return torch.cat(ve, 0), torch.cat(vf, 0)


@torch.no_grad()
def encode_captions(model, ids, mask, bsz=1024):
    """Every caption through the text encoder once, `bsz` at a time: ids, mask (C, Lt) -> (text_embeds (C, Lt, D), text_feat (C, 256))."""
    model.eval()
    te, tf = [], []
    for i in range(0, ids.shape[0], bsz):
        e, f = model.encode_text(ids[i:i + bsz], mask[i:i + bsz])
        te.append(e)
        tf.append(f)
    return torch.cat(te, 0), torch.cat(tf, 0)


@torch.no_grad()
def rerank_retrieval(model, video_embeds, video_feat, text_embeds, text_feat, text_input_mask, k, pair_bsz=512, num_clips=1, score_agg_func="mean"):
    """Two-stage search over cached features (the k_test evaluation of ALBEF / BLIP; the reference itself scores every pair, which
    score_all_pairs reproduces).  Stage 1: the k best videos per caption and the k best captions per video by the 256-d contrastive
    features (hip.sim_topk, scale = 1 / temp: no (V, C) matrix).  Stage 2: only the union of the two candidate sets goes through the
    fusion encoder and the ITM head (model.score_pair_list), every pair once, in the order of vi * C + ci, `pair_bsz` pairs at a time --
    at most 2 k max(V, C) fusion passes instead of V * C.  One host read (the pair count) and the read of `temp`.
    num_clips = n > 1: video_embeds / video_feat are encode_gallery(..., num_clips=n)'s, (V*n, ...) with row v * n + j.  Stage 1 orders by
    the POOLED similarity (hip.sim_topk_clips in both directions, still no matrix); stage 2 scores each candidate pair over its n clips
    (sequences pair-major, max(1, pair_bsz // n) pairs at a time) and pools the logits with hip.clip_pool before the softmax.
    Returns a dict of device tensors: t2v_idx (C, k) int32 video indices, t2v_sim (C, k) similarity / temp, t2v_score (C, k)
    softmax(itm logits)[:, 1]; v2t_idx / v2t_sim / v2t_score (V, k) likewise with caption indices.  Where k exceeds the gallery the tail
    of a row is idx -1, sim -inf, score -inf."""
    _check_clips(num_clips, score_agg_func)
    from alpro_amd import hip
    model.eval()
    n = int(num_clips)
    if video_feat.shape[0] % n:
        raise ValueError("video_feat has %d rows: not a whole number of videos of num_clips=%d clips" % (video_feat.shape[0], n))
    V, C = video_feat.shape[0] // n, text_feat.shape[0]
    vf, tf = video_feat.float().contiguous(), text_feat.float().contiguous()
    scale = 1.0 / float(model.temp)
    if n == 1:
        t2v_sim, t2v_idx = hip.sim_topk(tf, vf, k, scale=scale)
        v2t_sim, v2t_idx = hip.sim_topk(vf, tf, k, scale=scale)
    else:
        t2v_sim, t2v_idx = hip.sim_topk_clips(tf, vf, k, n, side="gallery", mode=score_agg_func, scale=scale)
        v2t_sim, v2t_idx = hip.sim_topk_clips(vf, tf, k, n, side="query", mode=score_agg_func, scale=scale)
    dev = vf.device
    t2v_pair = t2v_idx.long() * C + torch.arange(C, device=dev)[:, None]          # pair id = vi * C + ci
    v2t_pair = torch.arange(V, device=dev)[:, None] * C + v2t_idx.long()
    t2v_ok, v2t_ok = t2v_idx >= 0, v2t_idx >= 0
    pairs = torch.unique(torch.cat([t2v_pair[t2v_ok], v2t_pair[v2t_ok]]))        # sorted; its length is the one host read
    score = torch.empty(pairs.numel(), dtype=torch.float32, device=dev)
    step = max(1, pair_bsz // n)
    clip = torch.arange(n, device=dev)
    for s in range(0, pairs.numel(), step):
        p = pairs[s:s + step]
        vi, ci = torch.div(p, C, rounding_mode="floor"), p % C
        if n > 1:                                                                 # sequence i * n + j: clip j of pair p[i]
            vi, ci = (vi[:, None] * n + clip).reshape(-1), ci.repeat_interleave(n)
        logits = _pool_clips(model.score_pair_list(video_embeds, text_embeds, text_input_mask, vi, ci), n, score_agg_func)
        score[s:s + p.numel()] = torch.softmax(logits, dim=1)[:, 1]
    ninf = torch.full((), float("-inf"), dtype=torch.float32, device=dev)

    def lookup(pair, ok):
        pos = torch.searchsorted(pairs, pair.clamp(min=0).reshape(-1)).clamp(max=max(pairs.numel() - 1, 0)).view(pair.shape)
        return torch.where(ok, score[pos], ninf)

    return dict(t2v_idx=t2v_idx, t2v_sim=t2v_sim, t2v_score=lookup(t2v_pair, t2v_ok),
                v2t_idx=v2t_idx, v2t_sim=v2t_sim, v2t_score=lookup(v2t_pair, v2t_ok))


@torch.no_grad()
def rerank_metrics(idx, score, sim, gt):
    """R@1/5/10, median and mean rank of a re-ranked search: idx / score / sim (Q, k) are each query's candidates (idx -1 = no candidate), gt (Q,)
    its ground-truth gallery index.  A query's final order is its candidates sorted by (score descending, sim descending, idx ascending);
    with every column as a candidate and a constant sim that is the stable descending sort of the reference's eval_retrieval
    (run_video_retrieval.py:541-555).  `outside` counts the queries whose ground truth is not among their candidates; such a query counts as
    rank k + 1 in medianR and meanR, which are therefore LOWER BOUNDS when outside > 0.  R@1/5/10 are exact for k >= 10 (an outside query
    ranks below every candidate), which is why a smaller k raises ValueError."""
    idx, score, sim = torch.as_tensor(idx), torch.as_tensor(score), torch.as_tensor(sim)
    Q, k = idx.shape
    if k < 10:
        raise ValueError("rerank_metrics: k=%d candidates per query, need >= 10 for an exact R@10" % k)
    gt = torch.as_tensor(gt).to(idx.device).view(-1, 1).to(idx.dtype)
    hit = idx == gt
    inside = hit.any(1)
    neg = torch.full((), float("-inf"), dtype=score.dtype, device=score.device)
    gs = torch.where(hit, score, neg).max(1, keepdim=True)[0]     # the ground truth's own score / sim (idx holds it at most once)
    gm = torch.where(hit, sim, neg.to(sim.dtype)).max(1, keepdim=True)[0]
    before = (idx >= 0) & ((score > gs) | ((score == gs) & ((sim > gm) | ((sim == gm) & (idx < gt)))))
    rank = torch.where(inside, 1 + before.sum(1), torch.full_like(inside, k + 1, dtype=torch.long))
    r = rank.cpu().numpy()
    ins = inside.cpu().numpy()
    return dict(r1=100 * int((ins & (r <= 1)).sum()) / Q, r5=100 * int((ins & (r <= 5)).sum()) / Q, r10=100 * int((ins & (r <= 10)).sum()) / Q,
                medianR=float(np.median(r)), meanR=float(np.mean(r)), outside=int(Q - ins.sum()))


def records_from_matrices(score, sim, vid_ids, txt_ids):
    """(V, C) matrices -> the reference's result records (vid_id, txt_id, score, sim rounded to 4 decimals, :683-689), video-major."""
    sc, sm = score.detach().float().cpu().tolist(), sim.detach().float().cpu().tolist()
    return [dict(vid_id=v, txt_id=t, score=round(sc[i][j], 4), sim=round(sm[i][j], 4)) for i, v in enumerate(vid_ids) for j, t in enumerate(txt_ids)]


@torch.no_grad()
def retrieval_metrics_on_device(score, gt_col):
    """R@1/5/10, median and mean rank of a (rows, cols) device score matrix with ground-truth column gt_col[row], without sorting
    and without leaving the device until the five numbers are read: rank = 1 + #(columns scoring higher) + #(equal-scoring columns
    with a smaller index), i.e. the position a STABLE descending sort gives the ground truth (the reference sorts on the host,
    :541-555; on tie-free scores the two agree exactly)."""
    gt_col = gt_col.to(score.device).view(-1, 1)
    gt = score.gather(1, gt_col)
    cols = torch.arange(score.shape[1], device=score.device)[None, :]
    rank = 1 + (score > gt).sum(1) + ((score == gt) & (cols < gt_col)).sum(1)
    r = rank.double()
    out = torch.stack([(rank <= 1).double().mean() * 100, (rank <= 5).double().mean() * 100, (rank <= 10).double().mean() * 100, r.median() if r.numel() % 2 else
                       (r.sort()[0][r.numel() // 2 - 1] + r.sort()[0][r.numel() // 2]) / 2, r.mean()]).tolist()
    return dict(r1=out[0], r5=out[1], r10=out[2], medianR=out[3], meanR=out[4])


@torch.no_grad()
def topk_on_device(score, k):
    """Top-k columns of every row (values, indices) on the device -- e.g. the k best videos per caption of score.t()."""
    return torch.topk(score, min(k, score.shape[1]), dim=1)


def get_retrieval_metric_from_bool_matrix(bool_matrix):
    """R@1/5/10, median and mean rank from a (#rows, #cols) matrix sorted by decreasing score with exactly one ground-truth
    1 per row (run_video_retrieval.py:515-538)."""
    num_row = bool_matrix.shape[0]
    rows, gt_ranks = np.where(bool_matrix == 1)
    assert np.array_equal(rows, np.arange(num_row)), "each row should only a single GT"
    return dict(r1=100 * bool_matrix[:, 0].sum() / num_row, r5=100 * bool_matrix[:, :5].sum() / num_row,
                r10=100 * bool_matrix[:, :10].sum() / num_row, medianR=np.median(gt_ranks + 1), meanR=np.mean(gt_ranks + 1))


def _retrieval_scores(score_matrix, gt_row2col_id, row_idx2id, col_id2idx):
    order = torch.sort(score_matrix, dim=1, descending=True)[1]
    gt = torch.tensor([[col_id2idx[gt_row2col_id[row_idx2id[i]]]] for i in range(score_matrix.shape[0])])
    return get_retrieval_metric_from_bool_matrix((order == gt).numpy())


def eval_retrieval(vid_txt_score_dicts, gt_txt_id2vid_id):
    """text->video and video->text metrics from result records (run_video_retrieval.py:558-628; duplicates of a (txt, vid)
    pair keep the first record)."""
    by_txt = defaultdict(dict)
    for d in vid_txt_score_dicts:
        by_txt[d["txt_id"]].setdefault(d["vid_id"], d)
    txt_ids = list(by_txt)
    vid_ids = list(by_txt[txt_ids[0]])
    for t in txt_ids:
        assert len(by_txt[t]) == len(vid_ids), "each captions should be compared with the same #videos."
    txt_id2idx = {t: i for i, t in enumerate(txt_ids)}
    vid_id2idx = {v: i for i, v in enumerate(vid_ids)}
    score = torch.zeros(len(txt_ids), len(vid_ids))
    for t, preds in by_txt.items():
        for v, p in preds.items():
            score[txt_id2idx[t], vid_id2idx[v]] = p["score"]
    t2v = _retrieval_scores(score, gt_txt_id2vid_id, {i: t for t, i in txt_id2idx.items()}, vid_id2idx)
    gt_vid2txt = {v: k for k, v in gt_txt_id2vid_id.items()}
    v2t = _retrieval_scores(score.t(), gt_vid2txt, {i: v for v, i in vid_id2idx.items()}, txt_id2idx)
    return dict(text2video=t2v, video2text=v2t)
