"""TimeSformer (divided space-time ViT-B/16) on the MI355X kernels.

Mirrors the reference interface of src/modeling/timesformer/vit.py -- class names, constructor
arguments, `forward_features` signatures and the state_dict layout (`model.blocks.{i}.attn.qkv.weight`
...) -- while the arithmetic runs in libalpro_hip.so:

  reference (vit.py)                                   here
  ---------------------------------------------------  -----------------------------------------------
  PatchEmbed conv + flatten (:233-239), +pos/+time     alpro_patchify + alpro_gemm(PATCH_EMBED map) whose
  embeds via two rearranges (:342-361)                 residual is a (N*T, D) table bias+pos+time
  rearrange 'b (h w t) m -> (b h w) t m' (:147)        LayerNorm with SKIP_CLS gather (no copy)
  Attention (:81-100) on (B*N, T, D)                   alpro_gemm(qkv) -> alpro_attn_temporal -> alpro_gemm(proj)
  temporal_fc + residual (:161-162), rearrange/cat     the projection GEMM writes its 16-bit output only; the residual add,
  to (B*T, 1+N, D) (:165-172), norm1 (:180)            the frame-token gather and norm1 are ONE streaming kernel
                                                       (alpro_add_layernorm_fwd, PRE_SPATIAL)
  Attention on (B*T, 1+N, D) (:180)                    alpro_gemm(qkv) -> alpro_attn -> alpro_gemm(proj), 16-bit output
  CLS mean + scatter back + residual (:184-196),       alpro_add_layernorm_fwd (PRE_MLP): scatter map, frame mean of the CLS
  norm2 (:200)                                         rows, residual add and norm2 in one pass
  norm2 + Mlp + residual (:198-212)                    LayerNorm -> alpro_gemm(GELU) -> alpro_gemm(residual)
  norm (:372) + temporal mean pool (:484-492)          alpro_vit_final_pool
  DropPath per (b n)/(b t)/b rows (vit_utils.py:137)   row_scale vector in the GEMM epilogue
  forward hooks on attn.attn_drop / temporal_attn      forward_features(output_attentions=, output_hidden_states=): the maps are
  .attn_drop (the softmax of :92-93) and on the blocks  recomputed from q | k | v and the log-sum-exp rows (alpro_attn_probs,
                                                       alpro_attn_temporal_probs), the hidden states are copies -> VisualEncoderOutput
  retain_grad() on the input of attn.attn_drop /       forward_features(attn_grads=VitAttnGradients(...)): the blocks' backward hands the collector
  temporal_attn.attn_drop (:92-93)                     d(ctx) where it is final (alpro_attn_probs_grad, alpro_attn_temporal_probs_grad)
"""
import math
from functools import partial

import torch
import torch.nn as nn

from alpro_amd import config as rt
from alpro_amd import hip
from alpro_amd import streams
from alpro_amd.modeling import train as tr
from alpro_amd.modeling.weights import OperandCache, param_version

VIT_EPS = 1e-6


def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
    """vit_utils.py:56-76 semantics (delegates to torch's identical implementation)."""
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


def to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


class DropPath(nn.Module):
    """Stochastic depth (vit_utils.py:154-162).  In the fused path the Bernoulli row mask is sampled by
    `row_scale` below and applied inside the producing GEMM's epilogue."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def row_scale(self, rows, device):
        if not self.drop_prob or not self.training:
            return None
        keep = 1.0 - self.drop_prob
        return torch.floor(keep + torch.rand(rows, dtype=torch.float32, device=device)) / keep


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., with_qkv=True):
        super().__init__()
        assert with_qkv, "the ALPRO path always uses with_qkv=True (vit.py:114,120)"
        assert proj_drop == 0., "proj_drop (drop_rate) must be 0: element dropout behind the projections is not implemented (attn_drop is)"
        assert 0. <= attn_drop < 1., "attn_drop must be in [0, 1)"
        self.num_heads = num_heads
        head_dim = dim // num_heads
        assert head_dim == 64, "kernels are specialised for head_dim 64 (ViT-B/16, BERT-base)"
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        # vit.py:79,94: dropout on the softmax probabilities, train mode only.  Parameter-free (no state_dict key); applied inside the attention
        # kernels from a per-launch seed (Block._attn_drop_seeds), never as a module call.
        self.attn_drop = nn.Dropout(attn_drop)


class _ClsSide(streams.Side):
    """The precise-CLS chain of the ViT blocks on a second stream (alpro_amd.config.cls_stream, round 5).

    Per block the chain is: LayerNorm + q | k | v of the B CLS rows (needs only the block INPUT's CLS rows: the temporal half never touches
    them) -> [the CLS query's attention, inside the main path's attention launch] -> projection of B*T rows -> frame mean + residual ->
    norm2 + fc1 + GELU -> fc2 + residual, written over the 16-bit path's CLS rows of the block output.  Five skinny launches of 10-35 us
    that each leave most of the chip idle when they sit BETWEEN the block's big launches.  Here they go to a side stream:
        side:  [wait: block input ready]  snapshot x[:, 0], q|k|v rows                                   -> ev_q
        main:  temporal half, add+norm1, qkv GEMM, [wait ev_q] attention (+ CLS query)                   -> ev_attn, ... fc2 -> ev_out
        side:  [wait ev_attn / the main path's x2] proj rows, frame mean, fc1 rows, [wait ev_out] fc2 rows over out[:, 0]  -> done
        main (next block):  [wait done] before its first read of the CLS rows (the add + norm1 kernel)
    so the first part runs beside the temporal half and the second beside the MLP GEMMs.  All side-stream outputs live in buffers owned by
    this object (no allocation crosses streams); the event order above is also what makes their re-use from block to block safe."""
    def __init__(self, stream):
        self.stream, self.bufs, self.done = stream, {}, None

    def buf(self, name, shape, device):
        t = self.bufs.get((name, shape))
        if t is None:
            t = self.bufs[(name, shape)] = torch.empty(shape, dtype=torch.float32, device=device)
        return t

    def wait_done(self):
        """Main stream: the previous block's chain has written its CLS rows."""
        if self.done is not None:
            torch.cuda.current_stream().wait_event(self.done)
            self.done = None


# one chain (side stream + buffers) per LAUNCH stream: the two-stream block runner (run_blocks) drives two of them at once
_CLS_SIDES = streams.SideStreams("cls", _ClsSide)


def join_cls_chain(device):
    """The current stream waits for the precise-CLS chain that was driven from it."""
    side = _CLS_SIDES.peek(device)
    if side is not None:
        side.wait_done()


_ClsSide.join = staticmethod(join_cls_chain)


def _draws_per_call(blk):
    """True if a forward of the block draws from a random stream PER CALL (train mode only): its two attention-dropout seeds, or drop-path masks that
    sample_drop_paths did not draw for the whole step beforehand."""
    if not blk.training:
        return False
    live_dp = isinstance(blk.drop_path, DropPath) and bool(blk.drop_path.drop_prob)
    return blk.attn.attn_drop.p > 0 or blk.temporal_attn.attn_drop.p > 0 or (live_dp and not getattr(blk, "_presampled", None))


class VisualEncoderOutput:
    """What forward_features returns when output_attentions or output_hidden_states is set.
      features             what the call returns without the flags (still differentiable when the call is anchored)
      hidden_states        depth + 1 fp32 tensors (B, 1 + N*T, D): the embedding output (= the input of block 0), then every block's output; tokens
                           in the reference's order b (h w t) behind the CLS row; before the final norm and the pooling.  None if not asked for
      spatial_attentions   one (B*T, H, 1+N, 1+N) fp32 tensor per collected block (or its attn_window), batch index b*T + t, key / query 0 = the
                           frame's copy of CLS.  None if not asked for
      temporal_attentions  one (B*N, H, T, T) fp32 tensor per collected block, batch index b*N + n.  None if not asked for
    The maps are what a forward pre-hook on the reference's attn.attn_drop / temporal_attn.attn_drop receives (the softmax before dropout);
    all of them are detached copies."""
    __slots__ = ("features", "hidden_states", "spatial_attentions", "temporal_attentions")

    def __init__(self, features, hidden_states=None, spatial_attentions=None, temporal_attentions=None):
        self.features, self.hidden_states = features, hidden_states
        self.spatial_attentions, self.temporal_attentions = spatial_attentions, temporal_attentions


class _Collector:
    """The maps and hidden states of one forward_features call.  It only reads: no random draw, no write to anything the forward reads, every
    launch on the launch stream.  Blocks are counted as they run (block_begin / block_end), so a frozen prefix and the anchored blocks behind it
    share one object."""

    def __init__(self, depth, output_attentions, output_hidden_states, attn_layers=None, attn_window=None):
        self.want_attn, self.want_hidden = bool(output_attentions), bool(output_hidden_states)
        if attn_layers is None:
            self.layers = set(range(depth))
        else:
            self.layers = set()
            for i in attn_layers:
                i = int(i)
                if not -depth <= i < depth:
                    raise ValueError("attn_layers: block index %d outside -%d .. %d" % (i, depth, depth - 1))
                self.layers.add(i % depth)
        self.q_range = self.k_range = None
        if attn_window is not None:
            try:
                (q0, q1), (k0, k1) = attn_window
            except (TypeError, ValueError):
                raise ValueError("attn_window must be ((q_start, q_stop), (k_start, k_stop)) over the 1 + N tokens of a frame (got %r)" % (attn_window,))
            self.q_range, self.k_range = (int(q0), int(q1)), (int(k0), int(k1))
        self.i = 0
        self.hidden, self.spatial, self.temporal = [], [], []

    def start(self, tok):
        """The embedding output (nothing else writes it yet)."""
        if self.want_hidden:
            self.hidden.append(tok.detach().clone())

    def block_begin(self):
        """-> self if the block about to run collects its maps, else None."""
        return self if (self.want_attn and self.i in self.layers) else None

    def block_end(self, tok):
        self.i += 1
        if self.want_hidden:
            join_cls_chain(tok.device)   # a precise-CLS chain on its side stream still writes the block output's CLS rows
            self.hidden.append(tok.detach().clone())

    def add_temporal(self, qkv, lse, T, H, scale):
        self.temporal.append(hip.attn_temporal_probs(qkv, lse, T, H, scale))

    def add_spatial(self, qkv, lse, batch, L, H, scale):
        self.spatial.append(hip.attn_probs(qkv, lse, batch, L, H, scale, q_range=self.q_range, k_range=self.k_range))

    def result(self, features):
        return VisualEncoderOutput(features, tuple(self.hidden) if self.want_hidden else None, tuple(self.spatial) if self.want_attn else None,
                                   tuple(self.temporal) if self.want_attn else None)


class VitAttnGradients:
    """Collects, during backward(), the gradient of whatever is differentiated w.r.t. the attention probabilities of the divided space-time blocks
    of one pass (TimeSformer.forward_features attn_grads): G = d(score) / d(P) and the Grad-CAM map P * relu(G), fp32, keyed by block index i:
      spatial_grads[i] / spatial_cams[i]     (B*T, H, nq, nk), batch index b*T + t: the (1+N, 1+N) map of every frame, or its spatial_window
      temporal_grads[i] / temporal_cams[i]   (B*N, H, T, T), batch index b*N + n: the map of every patch position
    -- the layouts of VisualEncoderOutput's maps.  P is the softmax BEFORE dropout, bitwise the `spatial_attentions` / `temporal_attentions`
    entry; G is what the reference leaves in .grad after retain_grad() on the input of attn.attn_drop / temporal_attn.attn_drop (vit.py:92-93).
    One launch per chosen block and half (hip.attn_probs_grad, hip.attn_temporal_probs_grad), on the launch stream, right where the
    hand-written backward holds the final d(ctx); the flash-style backward kernels never form either tensor.
    layers: block indices, negative from the end (None: all); want: "grad", "cam" or both; spatial / temporal: which halves are collected;
    spatial_window: ((q_start, q_stop), (k_start, k_stop)) over the 1 + N tokens of a frame, bit for bit the slice of the full map (the temporal
    maps are always whole); grad_scale: the factor the differentiated score carries (a loss scale under fp16 operands): the kernels multiply G
    by 1 / grad_scale.  With precise [CLS] rows the CLS query row's P and G are the 16-bit graph's (the one the backward differentiates), not
    the fp32 re-evaluation's.  Drop-path in train mode is allowed (G is then that sampled graph's gradient); active attention dropout is not.
    Reading a result before the backward has run through the chosen blocks raises."""

    def __init__(self, layers=None, want=("cam",), spatial=True, temporal=True, spatial_window=None, grad_scale=1.0):
        self.layers = None if layers is None else tuple(int(l) for l in layers)
        self.want = (want,) if isinstance(want, str) else tuple(want)
        if not self.want or len(set(self.want)) != len(self.want) or any(w not in ("grad", "cam") for w in self.want):
            raise ValueError("VitAttnGradients: want=%r (one or both of 'grad', 'cam')" % (want,))
        if self.layers is not None and not self.layers:
            raise ValueError("VitAttnGradients: no layer chosen")
        self.spatial, self.temporal = bool(spatial), bool(temporal)
        if not (self.spatial or self.temporal):
            raise ValueError("VitAttnGradients: spatial=False and temporal=False (nothing to collect)")
        self.q_range = self.k_range = None
        if spatial_window is not None:
            try:
                (q0, q1), (k0, k1) = spatial_window
            except (TypeError, ValueError):
                raise ValueError("VitAttnGradients: spatial_window must be ((q_start, q_stop), (k_start, k_stop)) over the 1 + N tokens of a frame (got %r)"
                                 % (spatial_window,))
            self.q_range, self.k_range = (int(q0), int(q1)), (int(k0), int(k1))
        self.grad_scale = float(grad_scale)
        if not self.grad_scale > 0 or not math.isfinite(self.grad_scale):
            raise ValueError("VitAttnGradients: grad_scale=%r (a positive finite number)" % (grad_scale,))
        self._pick, self._pending = (), None
        self._store = {}

    def begin(self, depth):
        """A pass over `depth` blocks starts: resolve `layers` against it and forget what an earlier pass left."""
        idx = range(depth) if self.layers is None else self.layers
        for i in idx:
            if not -depth <= i < depth:
                raise ValueError("VitAttnGradients: block index %d outside -%d .. %d" % (i, depth, depth - 1))
        self._pick = tuple(sorted(set(i % depth for i in idx)))
        self._pending = set((half, i) for i in self._pick for half, on in (("spatial", self.spatial), ("temporal", self.temporal)) if on)
        self._store = {(half, w): {} for half in ("spatial", "temporal") for w in ("grad", "cam")}

    def wants(self, i):
        return i in self._pick

    def first(self):
        return self._pick[0]

    def _keep(self, half, i, res):
        for w, t in zip(self.want, res if isinstance(res, tuple) else (res,)):
            self._store[(half, w)][i] = t
        self._pending.discard((half, i))

    def add_spatial(self, i, qkv, dctx, lse, batch, L, H, scale):
        if ("spatial", i) in self._pending:
            self._keep("spatial", i, hip.attn_probs_grad(qkv, dctx, lse, batch, L, H, scale, q_range=self.q_range, k_range=self.k_range, want=self.want,
                                                         grad_scale=1.0 / self.grad_scale))

    def add_temporal(self, i, qkv, dctx, lse, T, H, scale):
        if ("temporal", i) in self._pending:
            self._keep("temporal", i, hip.attn_temporal_probs_grad(qkv, dctx, lse, T, H, scale, want=self.want, grad_scale=1.0 / self.grad_scale))

    def _read(self, half, w):
        what = "%s_%ss" % (half, w)
        if self._pending is None:
            raise RuntimeError("VitAttnGradients.%s: the collector was not passed to a TimeSformer.forward_features(attn_grads=...) yet" % what)
        if self._pending:
            raise RuntimeError("VitAttnGradients.%s: backward() has not run through %s yet"
                               % (what, ", ".join("block %d (%s)" % (i, h) for h, i in sorted(self._pending, key=lambda e: (e[1], e[0])))))
        if w not in self.want or not getattr(self, half):
            raise RuntimeError("VitAttnGradients.%s: the collector was built with want=%r, spatial=%r, temporal=%r" % (what, self.want, self.spatial, self.temporal))
        return self._store[(half, w)]

    spatial_grads = property(lambda self: self._read("spatial", "grad"))
    spatial_cams = property(lambda self: self._read("spatial", "cam"))
    temporal_grads = property(lambda self: self._read("temporal", "grad"))
    temporal_cams = property(lambda self: self._read("temporal", "cam"))


def _collector(depth, output_attentions, output_hidden_states, attn_layers, attn_window):
    if not (output_attentions or output_hidden_states):
        return None
    return _Collector(depth, output_attentions, output_hidden_states, attn_layers, attn_window)


def _run_collecting(blocks, tok, B, T, W, collect):
    """The one-stream no-grad loop with a collector (never two half batches: nothing is collected across streams)."""
    for blk in blocks:
        tok = blk(tok, B, T, W, collect=collect.block_begin())
        collect.block_end(tok)
    join_cls_chain(tok.device)
    return tok


def run_prefix_blocks(blocks, tok, B, T, W, collect=None):
    """The frozen prefix of a training forward (tr.frozen_prefix): the no-grad forward of `blocks`, in place -- nothing is saved for a backward
    and no W^T operand is built -- through run_blocks with what it brings (fused temporal launch, two half batches on two streams, deferred
    temporal add).  Train-mode stochasticity is the reference's: the drop-path masks are the ones sample_drop_paths drew for the whole step
    (run_blocks hands each half batch its rows of them), and a block with attention dropout draws its two seeds ONCE, so the seed stream reaches
    the trainable blocks where the all-trainable step's does -- two half-batch calls would draw twice, so blocks that draw per call take the
    whole batch on the launch stream."""
    with torch.no_grad():
        if collect is not None:
            return _run_collecting(blocks, tok, B, T, W, collect)
        if any(_draws_per_call(blk) for blk in blocks):
            for blk in blocks:
                tok = blk(tok, B, T, W)
            join_cls_chain(tok.device)
            return tok
        return run_blocks(blocks, tok, B, T, W)


def run_blocks(blocks, tok, B, T, W, collect=None):
    """The no-grad forward through `blocks` (tok updated in place and returned), CLS chains joined.

    Round 6: with alpro_amd.config.split_streams(B) the two halves of the batch go through every block on two HIP streams (clips are
    independent: vit.py:146-212 never mixes them).  Each half's launches are ordered on its own stream (and its precise-CLS chain on that
    stream's own side stream); the second stream is forked behind the embedding -- and again behind any block whose operand copies the launch
    stream had to (re)build -- and the launch stream waits for it once, behind the last block (ALPRO_SPLIT_LOCKSTEP=1: at every block boundary,
    a measurement aid that costs more than the split returns).  What it buys: a persistent GEMM's last, partly filled round of tiles and every
    kernel's ramp-up / drain no longer idle the chip -- workgroups of the other half's next launch take the CUs as they are vacated
    (B = 32 x 8 frames: -1.3 ... -3.2 % per forward, profiles/r6_split_streams_ab.txt).  Outputs are those of the one-stream forward bit for
    bit as long as the half batch sends every Linear to the same GEMM kernel as the whole batch."""
    dev = tok.device
    if collect is not None:
        return _run_collecting(blocks, tok, B, T, W, collect)
    if not (tok.is_cuda and not torch.is_grad_enabled() and rt.split_streams(B)):
        for blk in blocks:
            tok = blk(tok, B, T, W)
        join_cls_chain(dev)
        return tok
    from alpro_amd.modeling import weights
    main, aux = torch.cuda.current_stream(dev), streams.HALF.get(dev).stream
    h = B // 2
    lo, hi = tok[:h], tok[h:]
    lockstep = rt.split_lockstep()
    ev = main.record_event()        # the embedding is written
    for i, blk in enumerate(blocks):
        r0 = weights.operand_rebuilds()
        # drop-path masks drawn for the whole batch beforehand (sample_drop_paths; the frozen prefix of a training step): the rows of every mask are
        # clip-major and B is even here (split_streams refuses an odd B), so each half batch is handed its half of the three masks explicitly --
        # nothing is left on the module
        pre = getattr(blk, "_presampled", None)
        kw_lo = kw_hi = {}
        if pre:
            N = (tok.shape[1] - 1) // T
            masks = [pre[n] for n in (B * N, B * T, B)]    # temporal, spatial, MLP rows (distinct counts: sample_drop_paths draws only then)
            blk._presampled = None
            kw_lo, kw_hi = dict(drop_masks=tuple(m[:m.numel() // 2] for m in masks)), dict(drop_masks=tuple(m[m.numel() // 2:] for m in masks))
        blk(lo, h, T, W, **kw_lo)
        if weights.operand_rebuilds() != r0:   # the launch stream (re)built operand copies of this block: the second stream may only read them afterwards
            ev = main.record_event()
        with torch.cuda.stream(aux):
            if ev is not None:
                aux.wait_event(ev)
                ev = None
            blk(hi, h, T, W, **kw_hi)
            if lockstep or i == len(blocks) - 1:
                join_cls_chain(dev)
                ev_hi = aux.record_event()
        if lockstep or i == len(blocks) - 1:
            join_cls_chain(dev)
            main.wait_event(ev_hi)
            if lockstep:
                ev = main.record_event()
    return tok


class Block(nn.Module):
    def __init__(self, dim, num_heads, layer_num, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0.1, act_layer=nn.GELU, norm_layer=nn.LayerNorm, attention_type='divided_space_time',
                 use_grad_checkpointing=False):
        super().__init__()
        assert attention_type == 'divided_space_time', "TimeSformer.__init__ hard-codes divided_space_time (vit.py:435)"
        self.attention_type = attention_type
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.temporal_norm1 = norm_layer(dim)
        self.temporal_attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.temporal_fc = nn.Linear(dim, dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.layer_num = layer_num
        self.use_grad_checkpointing = use_grad_checkpointing
        self._ops = OperandCache()

    def _w(self, name, lin, dt):
        return self._ops.get(name, lin.weight, dt)

    # ---- merged temporal projection ------------------------------------------------------------------------------
    # vit.py:157-162 applies two Linears back to back with only drop_path between them:
    #     res_temporal = drop_path(temporal_attn.proj(attn_out));  xt = x + temporal_fc(res_temporal)
    # drop_path is a per-row scale s, so   temporal_fc(s * (a Wp^T + bp)) = s * (a (Wfc Wp)^T + Wfc bp) + bfc :
    # ONE (768 x 768) GEMM with the merged weight We = Wfc Wp (rebuilt per optimizer step from the two fp32 parameters, a
    # 0.9 GFLOP product), bias Wfc bp under the row scale and bfc after it (alpro_gemm bias2).  Saves one 100k x 768 x 768
    # GEMM per block in forward and, in backward, one dgrad and one wgrad: dWe = (s*dY)^T a is taken once and pushed through
    # the product rule (dWfc = dWe Wp^T + db1 bp^T, dWp = Wfc^T dWe, dbp = Wfc^T db1, dbfc = colsum(dY)).
    # With the merged projection the residual adds of the two attention halves run inside the following LayerNorm (alpro_add_layernorm_fwd);
    # merge_temporal_proj = False (the two Linears as written, fp32 residual in the GEMM epilogue) is the tests' oracle for it.
    merge_temporal_proj = True
    batch_merged_tproj = True   # the 12 blocks' merged-projection upkeep in batched launches (_MergedTProjBank); False = per block

    def _bank(self):
        bank = getattr(self, "_bank_obj", None) if (self.batch_merged_tproj and self.merge_temporal_proj) else None
        if bank is not None and (len(bank.blocks) <= self._bank_idx or bank.blocks[self._bank_idx] is not self):   # a deep copy of the model still points at the original's bank
            return None
        return bank

    def _merged_tproj(self, dt):
        bank = self._bank()
        if bank is not None:
            return bank.get(self._bank_idx, dt)
        wp, bp, wf = self.temporal_attn.proj.weight, self.temporal_attn.proj.bias, self.temporal_fc.weight
        ver = (param_version(wp), param_version(bp), param_version(wf), dt)
        hit = self._ops._store.get("t_merged")
        if hit is not None and hit[0] == ver:
            return hit[1]
        with torch.no_grad():
            we = hip.gemm(wf.detach().contiguous(), hip.transpose(wp.detach().contiguous()), out_dtype=torch.float32)   # (768, 768) fp32 = Wfc Wp
            b1 = torch.mv(wf.detach(), bp.detach()).contiguous()
            m = dict(w=we if dt == torch.float32 else hip.cast(we, dt), wT=hip.transpose(we, out_dtype=dt, pad_to=64), b1=b1)
        self._ops._store["t_merged"] = (ver, m)
        from alpro_amd.modeling import weights
        weights.note_operand_rebuild()
        return m

    # ---- precise CLS rows (alpro_amd.config.cls_precise; csrc/cls_precise.hip) -------------------------------------------------
    # The CLS row of the block output, re-evaluated in fp32 from the block input's CLS row: LayerNorm -> q | k | v (vit.py:84-85 on the
    # row that :165-167 replicates per frame: ONE row per clip) -> the CLS query's attention over the frame's tokens (K / V of the patch
    # tokens as the 16-bit GEMM produced them) -> proj -> frame mean + residual (:184-187) -> norm2 -> Mlp -> residual (:198-212).
    # B*T + 3*B fp32 rows per block against B*(1 + N*T) 16-bit rows; drop-path scales are the main path's.
    def _cls_qkv(self, x_cls_in, out=None):
        """(B, D) fp32 CLS rows of the block input -> their unrounded q in a (B, 3 D) buffer laid out like q | k | v (norm1 fused into the operand
        load).  Only the q third is computed (round 6): alpro_attn_fwd's CLS query reads q from this buffer and every K / V row -- the CLS
        token's included -- from the 16-bit images in LDS, so the k and v thirds were 2/3 of a 25 us launch per block for nothing."""
        sa = self.attn
        D = x_cls_in.shape[-1]
        if out is None:
            out = torch.empty((x_cls_in.shape[0], 3 * D), dtype=torch.float32, device=x_cls_in.device)
        hip.gemm_rows(x_cls_in, self._w("s_qkv", sa.qkv, torch.float32)[:D], bias=sa.qkv.bias[:D], ln=(self.norm1.weight, self.norm1.bias, VIT_EPS), out=out[:, :D])
        return out

    def _cls_side_begin(self, side, x, B, T, snapshot):
        """Side stream, at block entry: (snapshot of) the block input's CLS rows and their q | k | v.  -> (x_cls_in, cls_q, o_c buffer)."""
        main = torch.cuda.current_stream()
        D = x.shape[-1]
        ev_in = main.record_event()
        with torch.cuda.stream(side.stream):
            side.stream.wait_event(ev_in)
            if snapshot:    # the inference path updates x in place
                x_cls_in = side.buf("x_cls_in", (B, D), x.device)
                x_cls_in.copy_(x[:, 0])
            else:
                x_cls_in = x[:, 0]
            cls_q = self._cls_qkv(x_cls_in, out=side.buf("cls_q", (B, 3 * D), x.device))
            side.ev_q = side.stream.record_event()
        return x_cls_in, cls_q, side.buf("o_c", (B * T, D), x.device)

    def _cls_chain(self, x_cls_in, o_c, B, T, drop_s, drop_m, x2_out, out_out, side=None, ev_mid=None, ev_out=None):
        """The chain behind the attention.  x_cls_in: (B, D) fp32 CLS rows of the block input (a row-strided view is fine); o_c: (B*T, D) fp32
        attention output of the CLS query of every frame (alpro_attn_fwd's cls_out).  Writes the CLS rows before the MLP into x2_out and the CLS
        rows of the block output into out_out (both (B, D), row-strided views of the token tensors are fine): three alpro_gemm_rows_f32 launches
        (norm2 fused into fc1's operand load) and alpro_cls_mean_residual for the frame mean -- no torch glue in between.
        side = None: on the launch stream, fresh buffers.  side = the block's _ClsSide: the same launches on its stream and in its buffers, behind
        ev_mid (o_c -- and, training, the main path's x2 -- are written) and, for the last one, ev_out (so is the block output)."""
        sa, mlp, f32, dev = self.attn, self.mlp, torch.float32, o_c.device
        D = o_c.shape[-1]
        buf = (lambda name, rows, cols: side.buf(name, (rows, cols), dev)) if side is not None else (lambda name, rows, cols: None)
        with torch.cuda.stream(side.stream if side is not None else None):
            if side is not None:
                side.stream.wait_event(ev_mid)
            p_c = hip.gemm_rows(o_c, self._w("s_proj", sa.proj, f32), bias=sa.proj.bias, row_scale=drop_s, out=buf("p_c", B * T, D))
            hip.cls_mean_residual(x_cls_in, p_c, x2_out, B, T)
            f1c = hip.gemm_rows(x2_out, self._w("fc1", mlp.fc1, f32), bias=mlp.fc1.bias, act=hip.ACT_GELU, ln=(self.norm2.weight, self.norm2.bias, VIT_EPS),
                                out=buf("f1c", B, mlp.fc1.out_features))
            if side is not None:
                side.stream.wait_event(ev_out)
            hip.gemm_rows(f1c, self._w("fc2", mlp.fc2, f32), bias=mlp.fc2.bias, residual=x2_out, row_scale=drop_m, out=out_out)
            if side is not None:
                side.done = side.stream.record_event()

    def _drop(self, rows, device):
        if not isinstance(self.drop_path, DropPath):
            return None
        pre = getattr(self, "_presampled", None)
        if pre is not None and rows in pre:      # sampled for all 12 blocks at once by sample_drop_paths (4 launches, not 132)
            return pre.pop(rows)
        return self.drop_path.row_scale(rows, device)

    def _attn_drop_seeds(self):
        """-> (p temporal, seed temporal, p spatial, seed spatial) of this block for this step: two draws from the dropout-seed stream in train
        mode with attn_drop > 0 -- the reference drops whenever the module is in train mode, grad or not -- else zeros and NO draw (the stream
        of the BERT layers is not shifted).  A seed of 0 is "off" for the kernels."""
        pt, ps = self.temporal_attn.attn_drop.p, self.attn.attn_drop.p
        if not self.training:
            return 0.0, 0, 0.0, 0
        seed_t = rt.next_dropout_seed() if pt > 0 else 0
        seed_s = rt.next_dropout_seed() if ps > 0 else 0
        return (pt if seed_t else 0.0), seed_t, (ps if seed_s else 0.0), seed_s

    def forward(self, x, B, T, W, drop_masks=None, collect=None):
        """x: (B, 1 + N*T, D) fp32 contiguous token tensor; updated IN PLACE and returned (inference path).
        drop_masks: (temporal (B*N,), spatial (B*T,), MLP (B,)) drop-path row scales to apply instead of drawing them (run_blocks: a half batch's
        rows of the masks drawn for the whole step).  collect: the _Collector that takes this block's attention maps, or None."""
        return self._forward(x, B, T, drop_masks=drop_masks, collect=collect)

    def forward_train(self, x, B, T, W, collect=None, attn_grads=None):
        """Same arithmetic as forward() but out of place: fresh buffers (the backward needs every LayerNorm input); returns (out, saved) for the
        explicit backward().  attn_grads: (VitAttnGradients, this block's index) -- kept in `saved` (and by slim_saved / replay), backward()
        hands the collector d(ctx) of both attention halves."""
        return self._forward(x, B, T, save=True, collect=collect, attn_grads=attn_grads)

    def forward_cls(self, x, B, T, W):
        """LAST block when only the CLS output is consumed (the frozen prompter: get_pseudo_labels uses feat = proj(x[:, 0])):
        the temporal half and the spatial K/V need every token, but the spatial projection, the MLP and what follows are
        evaluated on the CLS rows alone -- (B*T, D) / (B, D) instead of (B*S, D).  Same arithmetic as forward() for those rows
        (vit.py:165-212); eval mode only (no drop-path).  Returns the block output's CLS rows, (B, D) fp32."""
        return self._forward(x, B, T, cls_only=True)

    def _forward(self, x, B, T, save=False, cls_only=False, drop_masks=None, replay=None, cls_precise=None, collect=None, attn_grads=None):
        """The divided space-time block (vit.py:146-212), every stage stated once.  The residual stream goes
            x --temporal branch--> xt --spatial branch--> x2 --MLP--> out
        and the three entry points differ in where those four live and in what is kept:
            forward        all four ARE x; with the merged projection xt is never written (its add rides in the add + norm2 kernel)
            forward_train  save: a fresh tensor each, q | k | v, the log-sum-exp rows and gelu' kept -> (out, saved)
            forward_cls    cls_only: as forward up to the spatial attention, the rest on the CLS rows -> their (B, D) output rows
        replay (Block.replay): the kept subset of an earlier forward_train's saved dict; operand dtype, projection form, drop-path scales and
        attention-dropout seeds are taken from it and nothing is drawn.  cls_precise: the precise-CLS decision of that earlier pass (None: read now).
        collect (a _Collector): the two attention maps of this block are recomputed from q | k | v and the log-sum-exp rows, which are then requested
        from the kernels in inference too (extra stores only; the attention outputs keep their bits), on the launch stream, before those temporaries go."""
        assert collect is None or not cls_only, "forward_cls collects nothing"
        keep = save or collect is not None   # q | k | v and the log-sum-exp rows are wanted
        dt = replay["dt"] if replay is not None else rt.compute_dtype()
        S, D = x.shape[1], x.shape[2]
        N = (S - 1) // T
        H = self.attn.num_heads
        ta, sa, fc, mlp, dev, f32 = self.temporal_attn, self.attn, self.temporal_fc, self.mlp, x.device, torch.float32
        merged = replay["merged"] if replay is not None else self.merge_temporal_proj
        xf = x.view(B * S, D)
        if cls_only:   # eval mode only: no drop-path mask and no dropout seed is drawn (the seed stream of later BERT layers does not shift)
            drop_t = drop_s = drop_m = None
            rs_t = rs_s = rs_m = {}
            seeds = ap_t, seed_t, ap_s, seed_s = 0.0, 0, 0.0, 0
        else:
            drop_t, drop_s, drop_m = drop_masks if drop_masks is not None else (self._drop(B * N, dev), self._drop(B * T, dev), self._drop(B, dev))
            rs_t, rs_s, rs_m = (dict(row_scale=d, row_scale_group=g) for d, g in ((drop_t, T), (drop_s, N + 1), (drop_m, S)))
            seeds = ap_t, seed_t, ap_s, seed_s = replay["attn_drop"] if replay is not None else self._attn_drop_seeds()   # the backward regenerates the masks from these
        # precise CLS rows, decided once: off (cp False) | on the launch stream (cp, side None) | on the side stream (side)
        cp = merged and not cls_only and (rt.cls_precise(dt) if cls_precise is None else cls_precise)
        side = _CLS_SIDES.get(dev) if (cp and rt.cls_stream(save) and x.is_cuda) else None
        ev_mid = None
        if side is not None:
            x_cls_in, cls_q, o_c_buf = self._cls_side_begin(side, x, B, T, snapshot=not save)
        elif cp:   # in place: a COPY (x is updated below; .contiguous() of a one-clip batch is a view); the temporal half never touches the CLS row
            x_cls_in = x[:, 0] if save else x[:, 0].clone()
        # ---- temporal attention (vit.py:146-156)
        h = hip.layernorm(x, self.temporal_norm1.weight, self.temporal_norm1.bias, VIT_EPS, dt, rows=B * N * T,
                          map_mode=hip.MAP_SKIP_CLS, map_p0=N * T)
        w_qkv = self._w("t_qkv", ta.qkv, dt)
        if rt.fuse_temporal_attention(training=save) and hip.qkv_tattn_ok(h, T) and ta.qkv.bias is not None and not seed_t:   # (the fused launch has no dropout)
            # round 6: qkv Linear + frame attention in one launch, q | k | v consumed out of the accumulators (alpro_gemm_qkv_tattn).  No-grad: the
            # (B*N*T, 2304) tensor is never written.  Training (ALPRO_FUSE_TATTN=1; off by default: alpro_amd/config.py): q | k | v are still
            # written (the backward reads them), what goes away is the attention launch and its re-read
            r = hip.gemm_qkv_tattn(h, w_qkv, ta.qkv.bias, T, H, ta.scale, want_qkv=keep)
            a_t, qkv_t, lse_t = r if keep else (r, None, None)
        else:
            qkv_t = hip.gemm(h, w_qkv, bias=ta.qkv.bias)
            r = hip.attn_temporal(qkv_t, T, H, ta.scale, want_lse=keep, drop_p=ap_t, drop_seed=seed_t)
            a_t, lse_t = r if keep else (r, None)
        del r
        if collect is not None:   # (B*N, H, T, T): the softmax before dropout
            collect.add_temporal(qkv_t, lse_t, T, H, ta.scale)
            if not save:
                qkv_t = lse_t = None
        # ---- temporal projection, x -> xt, norm1 in frame-token order (vit.py:157-172, 180)
        pr = None
        if merged:
            # round 3: the two N = 768 projections write 16-bit deltas in plain row order; residual add + row maps + LayerNorm are one
            # streaming kernel each (alpro_add_layernorm_fwd) -- see the kernel's header comment in csrc/core.hip
            mg = self._merged_tproj(dt)
            d_t = hip.gemm(a_t, mg["w"], bias=mg["b1"], **rs_t)
            if side is not None:
                side.wait_done()   # the previous block's chain has written this block's input CLS rows (first read: the kernel below)
            # round 6 (alpro_amd.config.defer_temporal_add): in place, x + temporal branch (vit.py:162) is not written here -- the add + norm2 kernel
            # below adds both branches to the block input in the same order of fp32 additions (bit for bit the same x').  forward_cls never needs
            # it: the patch rows of x are not read again and x[:, 0] is untouched
            defer = not save and (cls_only or rt.defer_temporal_add())
            hs, xt = hip.add_layernorm(x, d_t, self.norm1.weight, self.norm1.bias, VIT_EPS, mode=hip.ADD_PRE_SPATIAL,
                                       x_out=None if (save or defer) else x, want_x=not defer, delta_bias=fc.bias, T=T, N=N)
            if defer:
                xt = x
            else:
                del d_t
        else:   # the two Linears as written, fp32 residual read-modify-write in the GEMM epilogue (the tests' oracle for the merged form)
            xt = x
            if save:
                xt = torch.empty_like(x)
                xt[:, 0] = x[:, 0]
            pr = hip.gemm(a_t, self._w("t_proj", ta.proj, dt), bias=ta.proj.bias, **rs_t)
            hip.gemm(pr, self._w("t_fc", fc, dt), out=xt.view(B * S, D), bias=fc.bias, out_dtype=f32, residual=xf,
                     map_mode=hip.MAP_SKIP_CLS, map_p0=N * T)
            hs = hip.layernorm(xt, self.norm1.weight, self.norm1.bias, VIT_EPS, dt, rows=B * T * (N + 1),
                               map_mode=hip.MAP_FRAME_TOKENS, map_p0=T, map_p1=N)
        # ---- spatial attention (vit.py:180), the CLS query of every frame once more in fp32 inside the same launch if cp
        qkv_s = hip.gemm(hs, self._w("s_qkv", sa.qkv, dt), bias=sa.qkv.bias)
        cq = {}
        if side is not None:
            torch.cuda.current_stream().wait_event(side.ev_q)
            cq = dict(cls_q=cls_q, cls_group=T, cls_out=o_c_buf)
        elif cp:
            cq = dict(cls_q=self._cls_qkv(x_cls_in), cls_group=T)
        r = hip.attn(qkv_s, B * T, N + 1, H, sa.scale, want_lse=keep, drop_p=ap_s, drop_seed=seed_s, **cq)
        r = r if isinstance(r, tuple) else (r,)   # out [, lse] [, cls_out]
        a_s, lse_s, o_c = r[0], (r[1] if keep else None), (r[-1] if cp else None)
        del r, cq
        if collect is not None:   # (B*T, H, 1+N, 1+N) or its window; with precise CLS rows the CLS query row is the 16-bit graph's
            collect.add_spatial(qkv_s, lse_s, B * T, N + 1, H, sa.scale)
            if not save:
                lse_s = None
        if side is not None and not save:
            ev_mid = torch.cuda.current_stream().record_event()   # o_c is written
        # ---- spatial projection, xt -> x2, norm2 (vit.py:184-200)
        if cls_only:   # CLS query of every frame -> projection -> frame mean of the CLS rows (vit.py:187)
            a_cls = a_s.view(B * T, N + 1, D)[:, 0].contiguous()
            p_cls = hip.gemm(a_cls, self._w("s_proj", sa.proj, dt), bias=sa.proj.bias, out_dtype=f32)
            x2 = (x[:, 0] + p_cls.view(B, T, D).mean(1)).contiguous()
            h2 = hip.layernorm(x2, self.norm2.weight, self.norm2.bias, VIT_EPS, dt)
        elif merged:
            d_s = hip.gemm(a_s, self._w("s_proj", sa.proj, dt), bias=sa.proj.bias, **rs_s)
            if defer:
                h2, x2 = hip.add_layernorm_pre_mlp2(x, d_t, fc.bias, d_s, self.norm2.weight, self.norm2.bias, VIT_EPS, T, N, x_out=x), x
            else:
                h2, x2 = hip.add_layernorm(xt, d_s, self.norm2.weight, self.norm2.bias, VIT_EPS, mode=hip.ADD_PRE_MLP, x_out=None if save else x, T=T, N=N)
            del d_s
            if side is not None and save:
                ev_mid = torch.cuda.current_stream().record_event()   # o_c and the main path's x2 (whose CLS rows the chain overwrites) are written
        else:   # CLS side buffer: the epilogue leaves the frames' CLS deltas there, alpro_cls_mean_residual adds their mean
            x2 = torch.empty_like(x) if save else x
            cls_rows = torch.empty((B * T, D), dtype=f32, device=dev)
            hip.gemm(a_s, self._w("s_proj", sa.proj, dt), out=x2.view(B * S, D), bias=sa.proj.bias, out_dtype=f32, residual=xt.view(B * S, D), **rs_s,
                     map_mode=hip.MAP_FRAME_TOKENS, map_p0=T, map_p1=N, side=cls_rows)
            hip.cls_mean_residual(xt, cls_rows, x2, B, T)
            h2 = hip.layernorm(x2, self.norm2.weight, self.norm2.bias, VIT_EPS, dt)
        # ---- MLP, x2 -> out (vit.py:198-212)
        u, u_tiled = tr.gelu_save_buffer(B * S, mlp.fc1.out_features, D, dt, dev) if save else (None, False)
        # u holds gelu'(fc1 output) (round 3) rather than the fc1 output itself (round 5: in the GEMM's tile order)
        f1 = hip.gemm(h2, self._w("fc1", mlp.fc1, dt), bias=mlp.fc1.bias, act=hip.ACT_GELU_SAVE_GRAD if save else hip.ACT_GELU, pre_act=u, c2_tiled=u_tiled)
        out = hip.gemm(f1, self._w("fc2", mlp.fc2, dt), out=None if (save or cls_only) else xf, bias=mlp.fc2.bias, out_dtype=f32,
                       residual=x2.view(-1, D), **rs_m)
        if cls_only:
            return out
        out = out.view(B, S, D) if save else x
        if cp:
            # precise CLS rows: the block output's CLS row and (training) the saved pre-MLP stream's CLS row (norm2's backward input) take the fp32
            # values; the backward differentiates the 16-bit graph as before (its CLS-row operands differ from these by one rounding)
            ev_out = torch.cuda.current_stream().record_event() if side is not None else None
            x2_c = x2[:, 0] if save else (side.buf("x2_c", (B, D), dev) if side is not None else torch.empty_like(x_cls_in))
            self._cls_chain(x_cls_in, o_c, B, T, drop_s, drop_m, x2_c, out[:, 0], side, ev_mid, ev_out)
        if not save:
            return out
        ag = {} if attn_grads is None else dict(attn_grads=attn_grads)   # (no key without a collector: the saved dict is the one it always was)
        return out, dict(ag, x=x, dims=(B, T, N, S, D, H), dt=dt, drop_t=drop_t, drop_s=drop_s, drop_m=drop_m, attn_drop=seeds, merged=merged, u_tiled=u_tiled,
                         h=h, qkv_t=qkv_t, a_t=a_t, lse_t=lse_t, pr=pr, xt=xt, hs=hs, qkv_s=qkv_s, a_s=a_s, lse_s=lse_s, x2=x2, h2=h2, u=u, f1=f1)

    SLIM_KEYS = ("x", "drop_t", "drop_s", "drop_m", "attn_drop", "dims", "dt", "merged", "u_tiled")

    @staticmethod
    def slim_saved(sv):
        """What recomputation keeps of forward_train's saved dict (alpro_amd.config.recompute_blocks): the block input, the three drop-path scale
        vectors, the attention-dropout tuple and the scalars -- a dict of its own, so clearing `sv` releases every other activation and leaves this
        one whole.  Pure: no device work."""
        slim = {k: sv[k] for k in Block.SLIM_KEYS}
        if "attn_grads" in sv:   # (collector, block index): the replayed dict hands them to backward() again
            slim["attn_grads"] = sv["attn_grads"]
        return slim

    def replay(self, slim, W, cls_precise=None):
        """slim_saved(...) of an earlier forward_train -> the full saved dict again, by running the same _forward body on the kept input with the
        kept drop-path scales and dropout seeds.  Draws nothing: no dropout seed, no torch RNG, no pre-sampled mask is touched, and the module's
        train / eval state is not read.  The precise-CLS chain runs again where the first pass ran it (launch stream or its side stream) and is
        joined here, before anyone reads the rebuilt x2 and before the block output, which nobody needs, is released.
        The operand copies (16-bit weights, merged projection) are the step's: parameters must not have changed since the first pass."""
        B, T = slim["dims"][0], slim["dims"][1]
        out, sv = self._forward(slim["x"], B, T, save=True, drop_masks=(slim["drop_t"], slim["drop_s"], slim["drop_m"]), replay=slim, cls_precise=cls_precise,
                                attn_grads=slim.get("attn_grads"))
        join_cls_chain(out.device)
        return sv

    def _wt(self, name, lin, dt):
        return tr.transposed_operand(self._ops, name + "^T", lin.weight, dt)

    def _merged_tproj_backward(self, sv, dx, B, T, N, D, dt, G=None):
        """Backward of xt[:, 1:] = x[:, 1:] + s * (a We^T + Wfc bp) + bfc (see merge_temporal_proj); returns d(a).
        G: s * d(xt)[:, 1:] in the operand dtype when norm1's backward already emitted it (with dbfc accumulated), else built here."""
        ta, fc = self.temporal_attn, self.temporal_fc
        wp, bp, wf = ta.proj.weight.detach(), ta.proj.bias.detach(), fc.weight.detach()
        mg = self._merged_tproj(dt)
        dev = dx.device
        # G = s * dY in the operand dtype; dbfc = colsum(dY) (unscaled) from the same pass
        if G is None:
            G = hip.gather_cast(dx, dt, rows=B * N * T, map_mode=hip.MAP_SKIP_CLS, map_p0=N * T, row_scale=sv["drop_t"], row_scale_group=T,
                                colsum_pre=tr.bias_grad(fc.bias))
        # frozen members (requires_grad, read now): dWe feeds dWfc and dWp, db1 feeds dWfc and dbp; with none of the three trainable neither is
        # formed (temporal_fc.bias took its column sums from whoever built G)
        t_fc, t_p, t_bp = tr.trainable(fc.weight), tr.trainable(ta.proj.weight), tr.trainable(ta.proj.bias)
        if not (t_fc or t_p or t_bp):
            return tr.dgrad(G, mg["wT"])
        ws = sv.get("ws")  # zeroed slice of the per-backward workspace (one fill for all 12 blocks), else allocate
        if ws is None:
            ws = torch.zeros(D * D + D, dtype=torch.float32, device=dev)
        dWe, db1 = ws[:D * D].view(D, D), ws[D * D:]
        cs = db1 if (t_fc or t_bp) else None
        if dt != torch.float32 and not (t_fc or t_p):
            hip.colsum_tn(G, sv["a_t"].shape[1], db1)                            # only dbp wanted: db1 = colsum(G) with the GEMM's bits, no dWe
        elif dt != torch.float32:
            hip.gemm_tn_acc(G, sv["a_t"], dWe, colsum=cs)                        # dWe = G^T a, db1 = colsum(G)
        elif t_fc or t_p:
            hip.gemm(hip.transpose(G, colsum=cs), hip.transpose(sv["a_t"]), out=dWe, out_dtype=torch.float32)
        else:
            db1.add_(G.sum(0, dtype=torch.float32))
        da = tr.dgrad(G, mg["wT"])                                              # d(a) = G We
        if sv.get("defer_product_rule"):   # the bank applies the product rule for a whole group of blocks at once (_MergedTProjBank.product_rule)
            return da
        # product rule back onto the two real parameters (768^3 each).  Exact mode: fp32 MFMA.  16-bit modes: 16-bit operands with fp32
        # accumulation into the fp32 gradient, like every other weight gradient on this path (dWe itself came from 16-bit operands) --
        # the two fp32 768^3 GEMMs were 57 us each on 36 workgroups, 2 x 12 of them per step.
        g_fc, g_p = tr.grad_target(fc.weight), tr.grad_target(ta.proj.weight)     # None: frozen, its term of the product rule is not evaluated
        if dt != torch.float32:
            if g_fc is not None:
                hip.gemm(hip.cast(dWe, dt), self._w("t_proj", ta.proj, dt), out=g_fc, out_dtype=torch.float32, residual=g_fc)   # += dWe Wp^T
            if g_p is not None:
                hip.gemm(self._wt("t_fc", fc, dt)[:, :D], hip.transpose(dWe, out_dtype=dt), out=g_p, out_dtype=torch.float32, residual=g_p)  # += Wfc^T dWe
        else:
            if g_fc is not None:
                hip.gemm(dWe, wp.contiguous(), out=g_fc, out_dtype=torch.float32, residual=g_fc)                     # += dWe Wp^T
            if g_p is not None:
                hip.gemm(hip.transpose(wf.contiguous()), hip.transpose(dWe), out=g_p, out_dtype=torch.float32, residual=g_p)  # += Wfc^T dWe
        if g_fc is not None:
            g_fc.addr_(db1, bp)                                                                                   # += db1 bp^T
        if t_bp:
            tr.bias_grad(ta.proj.bias).add_(torch.mv(wf.t(), db1))                                                # += Wfc^T db1
        return da

    def backward(self, sv, dx, dz=None, emit_for=None):
        """dx: gradient w.r.t. the block output, (B, S, D) fp32; overwritten with the gradient w.r.t. the block input.
        dz: the operand rows drop_m * dx in the compute dtype if whoever produced dx already emitted them (the final norm's backward, or
        the next block's temporal-LayerNorm backward), else None -> built here by alpro_gather_cast.
        emit_for: saved state of the PREVIOUS block (the next one to run its backward): its dz is emitted by this block's last kernel; None
        for the first block of the anchored run (block 0, or the first block behind a frozen prefix).
        Frozen parameters get no gradient and no work: see tr.wgrad / tr.grad_target.
        Returns (dx, dz for the previous block or None)."""
        B, T, N, S, D, H = sv["dims"]
        dt = sv["dt"]
        ta, sa = self.temporal_attn, self.attn
        ap_t, seed_t, ap_s, seed_s = sv["attn_drop"]
        # ---- MLP: out = x2 + drop_m * (fc2(gelu(fc1(LN2(x2)))))
        if dz is None:
            dz = hip.gather_cast(dx, dt, row_scale=sv["drop_m"], row_scale_group=S)
        tr.wgrad(dz, sv["f1"], self.mlp.fc2.weight, self.mlp.fc2.bias)
        du = tr.dgrad(dz, self._wt("fc2", self.mlp.fc2, dt), gelu_grad=sv["u"], gelu_tiled=sv["u_tiled"])
        del dz
        tr.wgrad(du, sv["h2"], self.mlp.fc1.weight, self.mlp.fc1.bias)
        dh2 = tr.dgrad(du, self._wt("fc1", self.mlp.fc1, dt))
        g, b_ = tr.grad_target(self.norm2.weight), tr.grad_target(self.norm2.bias)   # (None: frozen -- both None is the data-only LayerNorm backward)
        # ---- spatial: x2 = scatter(xt + drop_s * proj(attn(qkv(LN1(gather(xt)))))), CLS averaged over frames
        # norm2's backward hands the finished d(x2) rows straight to the spatial projection's GEMMs (frame-token order, drop_s, CLS / T)
        _, dpo = hip.layernorm_bwd(dh2, sv["x2"], self.norm2.weight, VIT_EPS, dx, g, b_,
                                   emit=dict(mode=hip.EMIT_FRAME, rows=B * T * (N + 1), dtype=dt, T=T, N=N, scale=sv["drop_s"]))
        tr.wgrad(dpo, sv["a_s"], sa.proj.weight, sa.proj.bias)
        da = tr.dgrad(dpo, self._wt("s_proj", sa.proj, dt))
        del dpo
        ag, ag_i = sv.get("attn_grads") or (None, None)
        if ag is not None:   # d(ctx) of the spatial half is final: G = da v^T and P * relu(G), which the flash-style backward below never forms
            ag.add_spatial(ag_i, sv["qkv_s"], da, sv["lse_s"], B * T, N + 1, H, sa.scale)
        dqkv = hip.attn_bwd(sv["qkv_s"], sv["a_s"], da, sv["lse_s"], B * T, N + 1, H, sa.scale, drop_p=ap_s, drop_seed=seed_s)
        tr.wgrad(dqkv, sv["hs"], sa.qkv.weight, sa.qkv.bias)
        dhs = tr.dgrad(dqkv, self._wt("s_qkv", sa.qkv, dt))
        g, b_ = tr.grad_target(self.norm1.weight), tr.grad_target(self.norm1.bias)
        # ---- temporal: xt[:, 1:] = x[:, 1:] + fc(drop_t * proj(attn(qkv(LN_t(x[:, 1:])))))
        G = None
        if sv["merged"]:  # norm1's backward emits drop_t * d(xt)[:, 1:] and the temporal_fc bias gradient (unscaled column sums)
            _, G = hip.layernorm_bwd(dhs, sv["xt"], self.norm1.weight, VIT_EPS, dx, g, b_, rows=B * T * (N + 1), map_mode=hip.MAP_FRAME_TOKENS,
                                     map_p0=T, map_p1=N, emit=dict(mode=hip.EMIT_SKIP_CLS, rows=B * N * T, dtype=dt, T=T, N=N, scale=sv["drop_t"], group=T,
                                                                   colsum_pre=tr.bias_grad(self.temporal_fc.bias)))
        else:
            hip.layernorm_bwd(dhs, sv["xt"], self.norm1.weight, VIT_EPS, dx, g, b_, rows=B * T * (N + 1),
                              map_mode=hip.MAP_FRAME_TOKENS, map_p0=T, map_p1=N)
        if sv["merged"]:
            da = self._merged_tproj_backward(sv, dx, B, T, N, D, dt, G=G)
        else:
            dfo = hip.gather_cast(dx, dt, rows=B * N * T, map_mode=hip.MAP_SKIP_CLS, map_p0=N * T)
            tr.wgrad(dfo, sv["pr"], self.temporal_fc.weight, self.temporal_fc.bias)
            dpp = tr.dgrad(dfo, self._wt("t_fc", self.temporal_fc, dt), row_scale=sv["drop_t"], row_scale_group=T)
            tr.wgrad(dpp, sv["a_t"], ta.proj.weight, ta.proj.bias)
            da = tr.dgrad(dpp, self._wt("t_proj", ta.proj, dt))
        if ag is not None:   # ... and of the temporal half, on the merged and on the unmerged projection path
            ag.add_temporal(ag_i, sv["qkv_t"], da, sv["lse_t"], T, H, ta.scale)
        dqkv = hip.attn_temporal_bwd(sv["qkv_t"], sv["a_t"], da, sv["lse_t"], T, H, ta.scale, drop_p=ap_t, drop_seed=seed_t)
        tr.wgrad(dqkv, sv["h"], ta.qkv.weight, ta.qkv.bias)
        dh = tr.dgrad(dqkv, self._wt("t_qkv", ta.qkv, dt))
        g, b_ = tr.grad_target(self.temporal_norm1.weight), tr.grad_target(self.temporal_norm1.bias)
        dz_prev = None
        if emit_for is not None:  # ... and the temporal norm's backward emits the previous block's MLP operand (its drop_m, all rows incl. CLS)
            _, dz_prev = hip.layernorm_bwd(dh, sv["x"], self.temporal_norm1.weight, VIT_EPS, dx, g, b_, rows=B * N * T, map_mode=hip.MAP_SKIP_CLS,
                                           map_p0=N * T, emit=dict(mode=hip.EMIT_ROWS, rows=B * S, dtype=dt, T=T, N=N, scale=emit_for["drop_m"], group=S,
                                                                   extra_cls=B))
        else:
            hip.layernorm_bwd(dh, sv["x"], self.temporal_norm1.weight, VIT_EPS, dx, g, b_, rows=B * N * T,
                              map_mode=hip.MAP_SKIP_CLS, map_p0=N * T)
        return dx, dz_prev


_KEEP_CACHE = {}


def sample_drop_paths(blocks, B, T, N, device):
    """All stochastic-depth row masks of one training forward in ONE draw: per block three Bernoulli(keep_i) vectors of
    B*N (temporal), B*T (spatial) and B (MLP) rows, scaled by 1/keep_i (vit_utils.py:137-151, rates vit.py:272).  The reference
    draws them one by one (36 x {rand, add, floor, div}); the distribution is the same, the launch count is 4."""
    sizes = (B * N, B * T, B)
    live = [blk for blk in blocks if isinstance(blk.drop_path, DropPath) and blk.drop_path.drop_prob and blk.training]
    if not live:
        return
    per = sum(sizes)
    key = (per, str(device), tuple(blk.drop_path.drop_prob for blk in live))
    keep = _KEEP_CACHE.get(key)
    if keep is None:  # per-row keep probability, built once per (batch geometry, rates)
        keep = torch.tensor([1.0 - blk.drop_path.drop_prob for blk in live], dtype=torch.float32).repeat_interleave(per).to(device)
        _KEEP_CACHE.clear()
        _KEEP_CACHE[key] = keep
    scale = torch.floor(keep + torch.rand(per * len(live), dtype=torch.float32, device=device)) / keep
    off = 0
    for blk in live:
        blk._presampled = {}
        for n in sizes:
            blk._presampled[n] = scale[off:off + n]
            off += n


class _MergedTProjBank:
    """Batched upkeep of the merged temporal projections of ALL blocks of one encoder (round 3).

    Per block and optimizer step the merged form needs W_e = W_fc W_p (fp32 768^3 product), its 16-bit copy, its transpose and
    W_fc b_p -- five small launches of which the product alone takes 64 us on 36 workgroups -- and the backward needs the product rule
    back onto the two real weights (two more 768^3 products, a cast, a transpose, a rank-1 update and a gemv): ~230 launches and 2.8 ms
    per training step for 12 blocks.  Here the same arithmetic runs as five launches for the forward refresh (alpro_transpose_batch,
    alpro_gemm_batch, one cast, alpro_transpose_batch, alpro_tproj_small) and five per group of blocks for the product rule, on buffers and
    job tables that live across steps.  Blocks outside a VisionTransformer (tests build single Blocks) keep the per-block code."""

    def __init__(self, blocks):
        self.blocks = list(blocks)
        self.state = None          # forward side: dict(key, dt, bufs, tables)
        self.bwd = None            # backward side: persistent ws / 16-bit copies
        self._bwd_tables = {}

    def __reduce__(self):
        """copy.deepcopy / pickle of a model must not drag the job tables (ctypes pointers into THIS model's storage) along: the copy starts
        with an empty bank and VisionTransformer._attach_bank() rebuilds it over the copied blocks at the next forward."""
        return (_MergedTProjBank, ([],))

    def _params(self):
        return [p for b in self.blocks for p in (b.temporal_fc.weight, b.temporal_attn.proj.weight, b.temporal_attn.proj.bias)]

    def get(self, idx, dt):
        """-> dict(w = W_e (D, D) in dt, wT = W_e^T in dt, b1 = W_fc b_p fp32) of block idx, refreshing ALL blocks if any parameter changed."""
        from alpro_amd.modeling import weights
        ps = self._params()
        fast = (weights.param_epoch(), weights._EXT_EPOCH[0], dt, tuple(p._version for p in ps))
        st = self.state
        if st is None or st["fast"] != fast:
            key = (dt,) + tuple(param_version(p) for p in ps)   # frozen parameters (the prompter) keep their key across optimizer steps
            if st is None or st["key"] != key:
                st = self._refresh(dt, key)
            st["fast"] = fast
        return dict(w=st["we_dt"][idx], wT=st["weT_dt"][idx], b1=st["b1"][idx])

    def _refresh(self, dt, key):
        nb = len(self.blocks)
        wf = [b.temporal_fc.weight.detach() for b in self.blocks]
        wp = [b.temporal_attn.proj.weight.detach() for b in self.blocks]
        bp = [b.temporal_attn.proj.bias.detach() for b in self.blocks]
        D, dev = wf[0].shape[0], wf[0].device
        st = self.state
        if st is None or st["dt"] != dt or st["we32"].device != dev:
            we32 = torch.empty((nb, D, D), dtype=torch.float32, device=dev)
            st = dict(dt=dt, we32=we32, wpT32=torch.empty_like(we32), b1=torch.empty((nb, D), dtype=torch.float32, device=dev),
                      we_dt=we32 if dt == torch.float32 else torch.empty((nb, D, D), dtype=dt, device=dev),
                      weT_dt=torch.empty((nb, D, D), dtype=dt, device=dev), sig=None)
        sig = tuple(t.data_ptr() for t in wf + wp + bp)
        if st["sig"] != sig:   # the parameters moved (FlatAdamW adopted them into its flat buffer): rebuild the job tables
            st["t_wp"] = hip.transpose_jobs([(wp[i], st["wpT32"][i]) for i in range(nb)])
            gb = hip.GemmBatch()
            for i in range(nb):
                gb.add(wf[i], st["wpT32"][i], out=st["we32"][i], out_dtype=torch.float32)   # W_e = W_fc W_p
            st["gemm"] = gb
            st["t_we"] = hip.transpose_jobs([(st["we32"][i], st["weT_dt"][i]) for i in range(nb)])
            st["t_b1"] = hip.tproj_jobs([dict(wfc=wf[i], bp=bp[i], b1=st["b1"][i]) for i in range(nb)], dev)
            st["sig"] = sig
        with torch.no_grad():
            hip.transpose_batch(*st["t_wp"], torch.float32)
            st["gemm"].launch()
            if dt != torch.float32:
                hip.cast(st["we32"].view(-1), dt, out=st["we_dt"].view(-1))
            hip.transpose_batch(*st["t_we"], dt)
            hip.tproj_small(*st["t_b1"], D, 0)
        st["key"] = key
        self.state = st
        from alpro_amd.modeling import weights
        weights.note_operand_rebuild()
        return st

    # ---- backward ------------------------------------------------------------------------------------------------
    def workspace(self, dt, device):
        """(nb, D*D + D) fp32, zeroed: row i receives dW_e (D, D) and db1 (D) of block i from its weight-gradient GEMM."""
        nb, D = len(self.blocks), self.blocks[0].temporal_fc.weight.shape[0]
        b = self.bwd
        if b is None or b["ws"].device != device or b["dt"] != dt:
            ws = torch.empty((nb, D * D + D), dtype=torch.float32, device=device)
            b = self.bwd = dict(dt=dt, ws=ws, ws_dt=torch.empty((nb, D * D + D), dtype=dt, device=device) if dt != torch.float32 else None,
                                dweT=torch.empty((nb, D, D), dtype=dt, device=device))
            self._bwd_tables = {}
        b["ws"].zero_()
        return b["ws"]

    def all_trainable(self, idx):
        """True if the three parameters the batched product rule writes gradients for are all trainable in block idx; a block with a frozen
        member applies the rule itself, member by member (Block._merged_tproj_backward)."""
        blk = self.blocks[idx]
        return all(tr.trainable(p) for p in (blk.temporal_fc.weight, blk.temporal_attn.proj.weight, blk.temporal_attn.proj.bias))

    def product_rule(self, lo, hi, dt, idx=None):
        """Blocks lo..hi-1 -- or, with idx, those of them listed there (ascending, each all_trainable): dW_fc += dW_e W_p^T + db1 b_p^T,
        dW_p += W_fc^T dW_e, db_p += W_fc^T db1 -- 16-bit operands with fp32 accumulation into the fp32 gradients, like every other weight gradient
        on this path.  Five launches for the whole group."""
        assert dt != torch.float32 and self.bwd is not None
        idx = tuple(range(lo, hi)) if idx is None else tuple(idx)
        if not idx:
            return
        b, blocks = self.bwd, [self.blocks[i] for i in idx]
        D = blocks[0].temporal_fc.weight.shape[0]
        ops = []
        for i, blk in zip(idx, blocks):
            ta, fc = blk.temporal_attn, blk.temporal_fc
            g_fc, g_p = tr.grad_buffer(fc.weight, zero=True)[0], tr.grad_buffer(ta.proj.weight, zero=True)[0]
            g_bp = tr.bias_grad(ta.proj.bias)
            ops.append(dict(i=i, wp_dt=blk._w("t_proj", ta.proj, dt), wfT_dt=blk._wt("t_fc", fc, dt), g_fc=g_fc, g_p=g_p, g_bp=g_bp,
                            wf=fc.weight.detach(), bp=ta.proj.bias.detach()))
        sig = tuple((o["wp_dt"].data_ptr(), o["wfT_dt"].data_ptr(), o["g_fc"].data_ptr(), o["g_p"].data_ptr(), o["g_bp"].data_ptr(), o["wf"].data_ptr())
                    for o in ops)
        tb = self._bwd_tables.get(idx)
        if tb is None or tb["sig"] != sig:
            ga, gbb = hip.GemmBatch(), hip.GemmBatch()
            for o in ops:
                dwe_dt = b["ws_dt"][o["i"], :D * D].view(D, D)
                ga.add(dwe_dt, o["wp_dt"], out=o["g_fc"], out_dtype=torch.float32, residual=o["g_fc"])                        # += dW_e W_p^T
                gbb.add(o["wfT_dt"][:, :D], b["dweT"][o["i"]], out=o["g_p"], out_dtype=torch.float32, residual=o["g_p"])     # += W_fc^T dW_e
            tb = dict(sig=sig, ga=ga, gb=gbb, keep=ops,
                      t_dwe=hip.transpose_jobs([(b["ws"][o["i"], :D * D].view(D, D), b["dweT"][o["i"]]) for o in ops]),
                      t_small=hip.tproj_jobs([dict(wfc=o["wf"], bp=o["bp"], db1=b["ws"][o["i"], D * D:], g_fc=o["g_fc"], g_bp=o["g_bp"]) for o in ops],
                                             b["ws"].device))
            self._bwd_tables[idx] = tb
        lo, hi = idx[0], idx[-1] + 1
        hip.cast(b["ws"][lo:hi].reshape(-1), dt, out=b["ws_dt"][lo:hi].reshape(-1))
        hip.transpose_batch(*tb["t_dwe"], dt)
        tb["ga"].launch()
        tb["gb"].launch()
        hip.tproj_small(*tb["t_small"], D, 1)


class PatchEmbed(nn.Module):
    """Image to patch embedding: the stride-16 conv (vit.py:230) evaluated as im2col rows x weight GEMM."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        img_size, patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        assert patch_size == (16, 16), "alpro_patchify is specialised for 16x16 patches (ViT-B/16)"
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0])
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1,
                 hybrid_backbone=None, norm_layer=nn.LayerNorm, num_frames=8, attention_type='divided_space_time', dropout=0.,
                 cross_attention_config=None, use_grad_checkpointing=False):
        super().__init__()
        assert drop_rate == 0., "drop_rate must be 0 (pos / time / proj / MLP dropout is not implemented; attn_drop_rate is)"
        self.attention_type = attention_type
        self.depth = depth
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.time_embed = nn.Parameter(torch.zeros(1, num_frames, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, self.depth)]  # vit.py:272
        self.blocks = nn.ModuleList([
            Block(layer_num=i, use_grad_checkpointing=use_grad_checkpointing, dim=embed_dim, num_heads=num_heads,
                  mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                  drop_path=dpr[i], norm_layer=norm_layer, attention_type=self.attention_type) for i in range(self.depth)])
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)
        for i, blk in enumerate(self.blocks):  # vit.py:290-298
            if i > 0:
                nn.init.constant_(blk.temporal_fc.weight, 0)
                nn.init.constant_(blk.temporal_fc.bias, 0)
        self._ops = OperandCache()
        self._attach_bank()

    def _attach_bank(self):
        """(Re)build the merged-projection bank over THIS module's blocks (also after copy.deepcopy, whose blocks come back with an empty bank
        and fall back to the per-block path until then)."""
        self._tproj_bank = _MergedTProjBank(self.blocks)    # (plain attribute: not a module, nothing for state_dict)
        for i, blk in enumerate(self.blocks):
            blk._bank_obj, blk._bank_idx = self._tproj_bank, i   # (a plain reference: copies / pickles reduce the bank to an empty one)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token', 'time_embed'}

    def _embed(self, x):
        """(B, C, T, H, W) -> (B, 1 + N*T, D) fp32 tokens (vit.py:321-361)."""
        if not self._tproj_bank.blocks or self._tproj_bank.blocks[0] is not self.blocks[0]:
            self._attach_bank()
        dt = rt.compute_dtype()
        B, C, T, Hh, Ww = x.shape
        D = self.embed_dim
        N = (Hh // 16) * (Ww // 16)
        pidx, tidx = self._embed_index(N, T, Ww // 16)
        frames = x.transpose(1, 2).reshape(B * T, C, Hh, Ww).contiguous().float()
        rows = hip.patchify(frames, dt)
        w = self._ops.get("patch_w", self.patch_embed.proj.weight.view(D, -1), dt)
        # table[n*T + t] = conv bias + pos_embed[1 + n] + time_embed[t]
        pos_p, time_e = self.pos_embed.detach()[0, 1:], self.time_embed.detach()[0]
        if pidx is not None:
            pos_p = pos_p.index_select(0, pidx)
        if tidx is not None:
            time_e = time_e.index_select(0, tidx)
        table = (self.patch_embed.proj.bias.detach()[None, None, :] + pos_p[:, None, :] + time_e[None, :, :]).reshape(N * T, D).contiguous()
        tok = torch.empty((B, 1 + N * T, D), dtype=torch.float32, device=x.device)
        tok[:, 0] = (self.cls_token.detach() + self.pos_embed.detach()[:, :1]).view(1, D)
        hip.gemm(rows, w, out=tok.view(-1, D), out_dtype=torch.float32, residual=table, map_mode=hip.MAP_PATCH_EMBED, map_p0=T, map_p1=N)
        self._last_rows = rows
        return tok, T, Ww // 16, N

    def _embed_index(self, N, T, Wg):
        """Nearest-neighbour resampling of pos_embed / time_embed when the input grid differs from the tables
        (vit.py:328-340: the P x P patch table is resampled in 2-D to the (N / Wg) x Wg input grid; :350-357: the frame
        table in 1-D).  Returns (patch index (N,) or None, frame index (T,) or None)."""
        from alpro_amd.utils.load_save import nearest_index
        dev = self.pos_embed.device
        pidx = tidx = None
        P2 = self.pos_embed.size(1) - 1
        if N != P2:
            P = int(P2 ** 0.5)
            if P * P != P2 or N % Wg != 0:
                raise RuntimeError("pos_embed holds %d patch slots (not a square grid) / input has %d patches in rows of %d" % (P2, N, Wg))
            Hg = N // Wg
            pidx = (nearest_index(P, Hg, dev)[:, None] * P + nearest_index(P, Wg, dev)[None, :]).reshape(-1)
        if T != self.time_embed.size(1):
            tidx = nearest_index(self.time_embed.size(1), T, dev)
        return pidx, tidx

    def _embed_backward(self, rows, dtok, B, T, N, Wg=None, pixel_grad=False):
        """Gradients of patch_embed.proj / cls_token / pos_embed / time_embed from dtok (B, 1+N*T, D).
        pixel_grad (needs Wg): also the data gradient of the patch embedding, returned as a (B, T, C, H, W) fp32 tensor -- drows @ W through the
        W^T operand of tr.transposed_operand, then alpro_unpatchify.  The CLS row, the tables and the conv bias are additive: nothing of them in it."""
        dt = rows.dtype
        D = self.embed_dim
        pe = self.patch_embed.proj
        dpix = None
        if tr.trainable(pe.weight) or pixel_grad:   # (neither: no operand rows and no GEMM)
            drows = hip.gather_cast(dtok, dt, rows=B * T * N, map_mode=hip.MAP_PATCH_EMBED, map_p0=T, map_p1=N)
        if pixel_grad:
            C, Hh, Ww = pe.weight.shape[1], (N // Wg) * 16, Wg * 16
            dpix = torch.empty((B, T, C, Hh, Ww), dtype=torch.float32, device=dtok.device)
            hip.unpatchify(tr.dgrad(drows, tr.transposed_operand(self._ops, "patch_w^T", pe.weight, dt), out_dtype=torch.float32), B * T, C, Hh, Ww, out=dpix)
        if tr.trainable(pe.weight):
            if dt != torch.float32:  # 16-bit operands: in-place TN weight gradient (contraction over the B*T*N patch rows)
                gw = tr.grad_buffer(pe.weight, zero=True)[0]
                hip.gemm_tn_acc(drows, rows, gw.view(D, -1))
            else:
                gw, existed = tr.grad_buffer(pe.weight)
                gw2 = gw.view(D, -1)
                hip.gemm(hip.transpose(drows), hip.transpose(rows), out=gw2, out_dtype=torch.float32, residual=gw2 if existed else None)
        # small (N*T, D) reductions: parameter-sized, stay in torch; each one is formed only for a trainable table
        t_pos, t_time, t_cls, t_b = (tr.trainable(q) for q in (self.pos_embed, self.time_embed, self.cls_token, pe.bias))
        dtable = dtok[:, 1:].sum(0).view(N, T, D) if (t_pos or t_time or t_b) else None
        if t_b:
            tr.add_grad(pe.bias, dtable.sum((0, 1)))
        dcls = dtok[:, 0].sum(0) if (t_cls or t_pos) else None
        tr.add_grad(self.cls_token, dcls)
        pidx, tidx = self._embed_index(N, T, Wg) if Wg is not None else (None, None)
        if t_pos:
            dpos = dtable.sum(1)
            if pidx is not None:  # resampled tables: scatter the gradients back onto the slots they were read from
                dpos = torch.zeros((self.pos_embed.size(1) - 1, D), dtype=dpos.dtype, device=dpos.device).index_put_((pidx,), dpos, accumulate=True)   # (sorted accumulate: fixed order, unlike index_add_'s atomics)
            tr.add_grad(self.pos_embed, torch.cat([dcls[None], dpos], 0))
        if t_time:
            dtime = dtable.sum(0)
            if tidx is not None:
                dtime = torch.zeros((self.time_embed.size(1), D), dtype=dtime.dtype, device=dtime.device).index_put_((tidx,), dtime, accumulate=True)
            tr.add_grad(self.time_embed, dtime)
        return dpix

    def stage_params(self):
        """Parameter lists of the encoder's stages in forward order -- embedding, block 0, block 1, ... -- for tr.frozen_prefix."""
        emb = list(self.patch_embed.parameters()) + [self.cls_token, self.pos_embed, self.time_embed]
        return [emb] + [list(blk.parameters()) for blk in self.blocks]

    def forward_features(self, x, return_all_tokens=False, output_attentions=False, output_hidden_states=False, attn_layers=None, attn_window=None):
        """The four keywords are TimeSformer.forward_features' (a VisualEncoderOutput when a flag is set; inference path)."""
        B = x.shape[0]
        collect = _collector(len(self.blocks), output_attentions, output_hidden_states, attn_layers, attn_window)
        tok, T, W, N = self._embed(x)
        if collect is not None:
            collect.start(tok)
        tok = run_blocks(self.blocks, tok, B, T, W, collect=collect)
        y = hip.layernorm(tok, self.norm.weight, self.norm.bias, VIT_EPS, torch.float32).view(B, -1, self.embed_dim)
        y = y if return_all_tokens else y[:, 0]
        return y if collect is None else collect.result(y)

    def forward(self, x):
        raise NotImplementedError("the Kinetics classification head is outside ALPRO's video-text path")


default_cfgs = {'vit_base_patch16_224': {'num_classes': 1000, 'input_size': (3, 224, 224), 'first_conv': 'patch_embed.proj', 'classifier': 'head'}}


class TimeSformer(nn.Module):
    """Same constructor / forward_features contract as vit.py:419-503."""

    def __init__(self, model_cfg, input_format='BGR', cross_attention_config=None, **kwargs):
        super().__init__()
        self.config_file = str(model_cfg)
        self.img_size = model_cfg['img_size']
        self.patch_size = model_cfg['patch_size']
        self.num_frames = model_cfg['num_frm']
        self.attn_drop_rate = model_cfg['attn_drop_rate']
        self.drop_path_rate = model_cfg['drop_path_rate']
        self.drop_rate = model_cfg['drop_rate']
        self.use_pooling = model_cfg['use_maxpooling']
        self.use_grad_ckpt = model_cfg['gradient_checkpointing']
        if self.use_grad_ckpt:
            # config_release/timesformer_divst_8x32_224_k600_gc.json:9.  The reference re-runs each Block in backward to fit 16-40 GB devices
            # (vit.py:366-370) -- and loses the blocks' parameter gradients doing so, so "what the reference does" is no
            # contract.  The flag is accepted for config compatibility and has NO effect -- said once, not silently; recomputation
            # is a runtime switch of its own (alpro_amd.config.recompute_blocks) and the warning names it
            import warnings
            warnings.warn("alpro_amd: gradient_checkpointing=true is accepted and ignored -- by default activations are kept in HBM (288 GB per MI355X; "
                          "B=64 x 8 frames peaks at 64 GB) and no block is recomputed in backward.  To recompute the ViT blocks' activations in backward "
                          "(bit for bit the same step, one block's activations live at a time) set ALPRO_RECOMPUTE=1 or use alpro_amd.config.use_recompute(True)",
                          RuntimeWarning, stacklevel=2)
        self.attention_type = 'divided_space_time'
        self.num_classes = 400
        self.input_format = input_format
        assert input_format == "RGB", "Official TimeSformer uses RGB input."
        self.model = VisionTransformer(img_size=self.img_size, num_classes=self.num_classes, patch_size=self.patch_size,
                                       embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                       norm_layer=partial(nn.LayerNorm, eps=VIT_EPS), drop_rate=self.drop_rate,
                                       attn_drop_rate=self.attn_drop_rate, drop_path_rate=self.drop_path_rate,
                                       num_frames=self.num_frames, attention_type=self.attention_type,
                                       cross_attention_config=cross_attention_config, use_grad_checkpointing=self.use_grad_ckpt, **kwargs)
        if self.use_pooling:
            self.maxpool_kernel_size = model_cfg['maxpool_kernel_size']
            self.maxpooling = torch.nn.MaxPool2d(kernel_size=self.maxpool_kernel_size)
        self.model.default_cfg = default_cfgs['vit_base_patch' + str(self.patch_size) + '_224']
        self.num_patches = (self.img_size // self.patch_size) * (self.img_size // self.patch_size)

    POOLING = {'temporal': hip.POOL_TEMPORAL, 'spatial': hip.POOL_SPATIAL, 'none': hip.POOL_NONE}   # vit.py:489

    def forward_features(self, x, return_all_tokens=True, pooling='temporal', output_attentions=False, output_hidden_states=False, attn_layers=None,
                         attn_window=None, attn_grads=None):
        """x: (b, c, t, h, w); the final LayerNorm fused with the pooling (vit.py:475-503), n = h*w/256 patches per frame:
          'temporal' -> (b, 1 + n, 768)     CLS, then every patch averaged over the frames
          'spatial'  -> (b, 1 + t, 768)     CLS, then every frame averaged over its patches
          'none'     -> (b, t, 1 + n, 768)  every patch of every frame, the clip's CLS token in front of each frame
        The reference reshapes the tokens by the CONFIG's img_size / num_frm (vit.py:481-487), so an input of another geometry raises there; here
        it raises too in the two frame-resolved modes (the temporal mode keeps taking the resampled geometries the ALPRO models feed it).
        With autograd enabled the whole encoder is one autograd node with a hand-written backward.

        output_attentions / output_hidden_states: return a VisualEncoderOutput (features = the value above, plus the hidden states and the spatial /
        temporal attention maps of the 12 divided space-time blocks: see that class) -- what forward hooks on the reference's blocks and on their
        attn.attn_drop / temporal_attn.attn_drop modules receive.  The forward is flash-style, so the maps are recomputed per block from its
        q | k | v and log-sum-exp rows (alpro_attn_probs, alpro_attn_temporal_probs) and the hidden states are copies; all are detached, the maps are
        the softmax BEFORE attention dropout, drop-path shows in the hidden states only.  With both flags off nothing of this runs.  Asking changes
        no bit of `features`, of a gradient or of a random stream, with one exception of schedule: an even batch of 16 clips or more runs as ONE
        stream (as under config.set_split_streams(False)), not as two half batches.  With precise [CLS] rows the CLS query row of a spatial map is
        the 16-bit graph's while the hidden states' CLS rows carry the fp32 re-evaluation.
        attn_layers: block indices (negative: from the end) whose maps are collected; None = all 12.  Mind the size: the full set at B = 8 clips of
        8 frames at 224 px is 12 x (64, 12, 197, 197) fp32 = 1.4 GB of spatial maps.
        attn_window: ((q_start, q_stop), (k_start, k_stop)) over the 1 + N tokens of a frame: only this window of every spatial map is formed, bit
        for bit the slice of the full map (the temporal maps are always whole).

        attn_grads (this repo's extension; the reference: retain_grad() on the input of attn.attn_drop / temporal_attn.attn_drop): a
        VitAttnGradients.  The backward of whatever is computed from the result fills it with d(score) / d(P) and / or P * relu(d score / d P) of
        the chosen blocks' spatial and temporal maps (see that class).  The pass is anchored even when no parameter is trainable and the clip
        needs no gradient: the frozen prefix then ends in front of the first chosen block and the frozen blocks behind it run their data-only
        backward (no .grad is written).  It changes no bit of `features`, of a gradient or of a random stream, and combines with the flags above.
        Refused: grad mode off (no backward would run), and a chosen block whose attention dropout is active (the maps are the pre-dropout
        softmax's; call model.eval()).  Drop-path in train mode is allowed."""
        if attn_grads is not None:   # host-side refusals, in front of any device work
            if not isinstance(attn_grads, VitAttnGradients):
                raise TypeError("forward_features(attn_grads=...): a VitAttnGradients collector is needed (got %s)" % type(attn_grads).__name__)
            if not torch.is_grad_enabled():
                raise RuntimeError("forward_features(attn_grads=...): grad mode is off (torch.no_grad / inference_mode) -- no backward will run, the collector would stay empty")
            attn_grads.begin(len(self.model.blocks))
            for i in attn_grads._pick:
                blk = self.model.blocks[i]
                if blk.training and (blk.attn.attn_drop.p > 0 or blk.temporal_attn.attn_drop.p > 0):
                    raise RuntimeError("forward_features(attn_grads=...): block %d has active attention dropout (train mode, attn_drop_rate > 0) -- the collected "
                                       "maps are the pre-dropout softmax's and its gradient; call model.eval() first" % i)
        assert return_all_tokens, "forward_features(return_all_tokens=False) is not supported (the reference fails on it: vit.py:484 indexes the 2-D CLS tensor with three subscripts)"
        assert pooling in ['temporal', 'spatial', 'none'], 'Invalid pooling type {}'.format(pooling)
        mode = self.POOLING[pooling]
        if mode != hip.POOL_TEMPORAL:
            G, (t, h, w) = self.img_size // self.patch_size, x.shape[2:]
            if (t, h // self.patch_size, w // self.patch_size) != (self.num_frames, G, G):
                raise RuntimeError("forward_features(pooling=%r): the input has %d frames of %d x %d patches, the config (num_frm=%d, img_size=%d) says %d frames of "
                                   "%d x %d -- the reference's rearrange (vit.py:487) fails on this input too" % (pooling, t, h // self.patch_size, w // self.patch_size,
                                                                                                               self.num_frames, self.img_size, self.num_frames, G, G))
        m = self.model
        collect = _collector(len(m.blocks), output_attentions, output_hidden_states, attn_layers, attn_window)
        if attn_grads is not None:
            # anchored whatever requires a gradient: a fresh scalar rides along as the one "parameter" that makes autograd schedule the node when
            # nothing else does (its gradient is None)
            rider = torch.zeros((), dtype=torch.float32, device=x.device, requires_grad=True)
            out = tr.run_anchored(_VisualRun(self, mode, collect, attn_grads), [x], list(self.parameters()) + [rider])
            return out if collect is None else collect.result(out)
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or x.requires_grad):   # (x.requires_grad: the pixel gradient)
            out = tr.run_anchored(_VisualRun(self, mode, collect), [x], list(self.parameters()))
            return out if collect is None else collect.result(out)
        B = x.shape[0]
        in_step = torch.is_grad_enabled()   # a wholly frozen encoder inside a training step: the frozen prefix is the whole encoder
        with torch.no_grad():               # (run_blocks forks its two half-batch streams only without grad)
            tok, T, W, N = m._embed(x)
            if collect is not None:
                collect.start(tok)
            if in_step:   # as _VisualRun.forward treats a prefix: the step's drop-path masks in one draw, one pair of dropout seeds per block
                if B * N != B * T and B * T != B:
                    sample_drop_paths(m.blocks, B, T, N, tok.device)
                tok = run_prefix_blocks(m.blocks, tok, B, T, W, collect=collect)
                for blk in m.blocks:
                    blk._presampled = None
            else:
                tok = run_blocks(m.blocks, tok, B, T, W, collect=collect)
            if mode == hip.POOL_TEMPORAL:
                out32, _ = hip.vit_final_pool(tok, m.norm.weight, m.norm.bias, VIT_EPS, B, T, N, torch.float32)
            else:
                out32, _ = hip.vit_final_pool_mode(tok, m.norm.weight, m.norm.bias, VIT_EPS, B, T, N, torch.float32, mode)
        return out32 if collect is None else collect.result(out32)

    def forward_cls(self, x, **flags):
        """x: (b, c, t, h, w) -> (b, 768): the CLS row of forward_features(x) only, inference only.  The last block's spatial
        projection and MLP run on the CLS rows alone (Block.forward_cls); used by the frozen prompter, whose pseudo labels
        depend on nothing else (alpro_models.py:531-551)."""
        if flags:
            raise TypeError("forward_cls takes no %s: its last block runs on the CLS rows alone, so it has neither whole hidden states nor the last "
                            "block's maps -- use forward_features(..., output_attentions=True / output_hidden_states=True)" % ", ".join(sorted(flags)))
        assert not torch.is_grad_enabled(), "forward_cls is an inference path"
        m = self.model
        B = x.shape[0]
        tok, T, W, N = m._embed(x)
        tok = run_blocks(m.blocks[:-1], tok, B, T, W)
        cls = m.blocks[-1].forward_cls(tok, B, T, W)
        return hip.layernorm(cls, m.norm.weight, m.norm.bias, VIT_EPS, torch.float32)

    def forward(self, x):
        return self.model(x)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """A string is a pre-trained checkpoint source exactly as in the reference (vit.py:515-533: 'vit_base_patch16_224', a CLIP
        ViT file, or a Kinetics TimeSformer checkpoint path; remapped by timesformer/helpers.py); a mapping is a plain state_dict."""
        if isinstance(state_dict, str):
            from alpro_amd.modeling.timesformer.helpers import load_visual_checkpoint
            return load_visual_checkpoint(self, state_dict)
        return super().load_state_dict(state_dict, strict=strict, **kw)


class _VisualRun:
    """Forward/backward of the whole visual encoder for tr.Anchor (alpro_models.py:186-194 under autograd)."""

    def __init__(self, enc, mode=hip.POOL_TEMPORAL, collect=None, attn_grads=None):
        self.enc, self.mode = enc, mode   # mode: the pooling behind the final norm (hip.POOL_*)
        self.collect = collect            # a _Collector (output_attentions / output_hidden_states) or None
        self.attn_grads = attn_grads      # a VitAttnGradients the blocks' backward fills, or None

    def forward(self, x):
        m = self.enc.model
        B = x.shape[0]
        # the frozen prefix (requires_grad is read NOW, at every forward): k leading stages -- embedding, block 0, ... -- hold no trainable parameter
        # and pixels need no gradient, so those blocks run their no-grad forward and the backward ends at the input of block k - 1.  A clip that
        # requires a gradient makes the prefix 0: the patch rows and the embedding stage are kept behind frozen parameters too, and backward()
        # goes on through the patch embedding to the pixels
        self.x_grad = (tuple(x.shape), x.dtype) if torch.is_tensor(x) and x.requires_grad else None
        k = tr.frozen_prefix(m.stage_params(), self.x_grad is not None)
        ag, self.attn_grads = self.attn_grads, None   # (the saved dicts of the chosen blocks carry it to backward)
        if ag is not None:   # a chosen block must be inside the backward range: the prefix ends in front of the first one
            k = min(k, 1 + ag.first())
        self.nfro, self.embed_frozen = max(k - 1, 0), k >= 1
        tok, T, W, N = m._embed(x)
        collect, self.collect = self.collect, None   # (nothing of it is needed in backward)
        if collect is not None:
            collect.start(tok)
        self.rows, self.dims, self.Wg = (None if self.embed_frozen else m._last_rows), (B, T, N), W
        if self.embed_frozen:
            m._last_rows = None   # (the patch rows are the weight gradient's operand: nobody reads them)
        self.saved = []
        # recomputation (alpro_amd.config.recompute_blocks, read NOW like requires_grad): every trainable block's saved dict is cut down to what
        # Block.replay needs as soon as the block is through -- one block's activations are live at a time -- and backward() rebuilds it
        self.recompute = rt.recompute_blocks()
        self.cp = rt.cls_precise(rt.compute_dtype())   # (the replay takes the first pass's precise-CLS decision, not the one in force at backward time)
        if B * N != B * T and B * T != B:  # (the table is keyed by row count: the three counts must differ, else draw per call)
            sample_drop_paths(m.blocks, B, T, N, tok.device)
        if self.nfro:
            tok = run_prefix_blocks(m.blocks[:self.nfro], tok, B, T, W, collect=collect)
            for blk in m.blocks[:self.nfro]:
                blk._presampled = None
        for j, blk in enumerate(m.blocks[self.nfro:], self.nfro):
            tok, sv = blk.forward_train(tok, B, T, W, collect=collect.block_begin() if collect is not None else None,
                                        attn_grads=(ag, j) if (ag is not None and ag.wants(j)) else None)
            blk._presampled = None
            if collect is not None:   # (the maps are already taken, inside the block: before the saved dict is cut down below)
                collect.block_end(tok)
            if self.recompute:
                join_cls_chain(tok.device)   # a precise-CLS chain on its side stream still writes x2's CLS rows: it is through before x2 is released
                sv, full = Block.slim_saved(sv), sv
                full.clear()
                del full
            self.saved.append(sv)
        join_cls_chain(tok.device)
        self.tok = tok
        if self.mode == hip.POOL_TEMPORAL:
            out32, _ = hip.vit_final_pool(tok, m.norm.weight, m.norm.bias, VIT_EPS, B, T, N, torch.float32)
        else:
            out32, _ = hip.vit_final_pool_mode(tok, m.norm.weight, m.norm.bias, VIT_EPS, B, T, N, torch.float32, self.mode)
        return out32

    def backward(self, dout):
        m = self.enc.model
        B, T, N = self.dims
        D = m.embed_dim
        nb, nfro = len(m.blocks), self.nfro
        g, b_ = tr.grad_target(m.norm.weight), tr.grad_target(m.norm.bias)
        S_ = 1 + N * T   # the final norm's backward emits the last block's MLP operand rows (its drop-path scale)
        last = self.saved[-1] if self.saved else None   # None: every block is in the frozen prefix, only the final norm is trainable
        emit_dt = last["dt"] if last is not None else rt.compute_dtype()
        if self.mode == hip.POOL_TEMPORAL:
            # final norm + temporal mean pool (vit.py:372,484-492): every frame token receives dout / T, the CLS token dout
            dy = torch.empty((B, 1 + N * T, D), dtype=torch.float32, device=dout.device)
            dy[:, 0] = dout[:, 0]
            torch.mul(dout[:, 1:].unsqueeze(2).expand(B, N, T, D), 1.0 / T, out=dy[:, 1:].view(B, N, T, D))  # one broadcast pass (was mul + repeat_interleave + copy)
            dtok = torch.empty_like(dy)
            r = hip.layernorm_bwd(dy.view(-1, D), self.tok, m.norm.weight, VIT_EPS, dtok, g, b_, accumulate=False,
                                  emit=dict(mode=hip.EMIT_ROWS, rows=B * S_, dtype=emit_dt, scale=last["drop_m"], group=S_) if last is not None else None)
            dz = r[1] if last is not None else None
            del dy, r
        else:   # spatial / none (vit.py:493-499): dout is un-pooled inside the LayerNorm-backward pass itself, dy is never built
            if g is None or b_ is None:   # frozen: this kernel (once per step) keeps its column sums and adds them to a pair nobody reads
                tg, tb = hip.ln_throwaway_pair(dout.device)
                g, b_ = (tg if g is None else g), (tb if b_ is None else b_)
            r = hip.vit_final_pool_mode_bwd(dout, self.tok, m.norm.weight, VIT_EPS, g, b_, B, T, N, self.mode,
                                            emit=dict(dtype=emit_dt, scale=last["drop_m"], group=S_) if last is not None else None)
            dtok, dz = r if last is not None else (r, None)
        if last is None:
            return self._embed_backward(dtok)
        bank = m.blocks[0]._bank()
        dt_run = last["dt"]
        banked = bank is not None and dt_run != torch.float32 and all(sv["merged"] for sv in self.saved)
        ws = bank.workspace(dt_run, dout.device) if banked else torch.zeros((nb, D * D + D), dtype=torch.float32, device=dout.device)
        # Data parallel: in the pretraining / retrieval models this node is the LAST one autograd runs (created first, its input needs
        # no gradient), so every gradient outside the visual encoder is final now and can be exchanged while the ViT backward (half of
        # the backward pass) runs; the blocks' own gradients follow four blocks at a time (alpro_amd.dist.grads_final -> FlatAdamW).
        # That is only true when no other anchored backward is still pending (tr.Anchor sets others_pending; a model that anchors the
        # text encoder first runs this node BEFORE it): then nothing is declared final here and everything goes at synchronize().
        from alpro_amd import dist
        overlap = dist.collectives_active() and not getattr(self, "others_pending", False)
        if overlap:
            dist.grads_final(all_but=list(self.enc.parameters()))
        group_hi, group_rule = nb, []
        marks = {}
        for j in range(nb - 1, nfro - 1, -1):   # block j; blocks below nfro are the frozen prefix: the backward ends at block nfro's input
            blk, sv = m.blocks[j], self.saved[j - nfro]
            if self.recompute:
                # rebuilt right before its backward and cleared right behind it; block j - 1 hands over its drop-path scales (emit_for) from its
                # kept dict and is replayed only when its turn comes.  The weight-gradient side stream holds the operands of the blocks behind us
                # (record_stream) until it has read them: the host lets it fall at most two blocks behind, so that what it is done with can be
                # handed out again instead of piling up beside the replayed block
                ev = marks.pop(j + 2, None)
                if ev is not None:
                    ev.synchronize()
                sv = blk.replay(sv, self.Wg, cls_precise=self.cp)
                self.saved[j - nfro] = None
            sv["ws"] = ws[j]
            sv["defer_product_rule"] = banked and bank.all_trainable(j)   # (a block with a frozen member applies the rule itself)
            if sv["defer_product_rule"]:
                group_rule.insert(0, j)
            dtok, dz = blk.backward(sv, dtok, dz=dz, emit_for=self.saved[j - 1 - nfro] if j > nfro else None)
            done = nb - j
            if done % 4 == 0 or j == nfro:   # a group of blocks is through: their merged-projection product rule in batched launches ...
                if banked:
                    bank.product_rule(j, group_hi, dt_run, idx=group_rule)
                if overlap and j > nfro:       # ... and then their gradients are final (the last group goes at synchronize())
                    dist.grads_final(params=[p for b in m.blocks[j:group_hi] for p in b.parameters()] + (list(m.norm.parameters()) if group_hi == nb else []))
                group_hi, group_rule = j, []
            sv.clear()
            if self.recompute:
                marks[j] = rt.wgrad_side_event(dtok.device)
        return self._embed_backward(dtok)

    def _embed_backward(self, dtok):
        """The embedding stage's backward behind the last block's, and the gradient of the clip when it asked for one: (B, C, T, H, W) in the
        clip's dtype, a view of (B, T, C, H, W)-contiguous memory -- the models pass visual_inputs.transpose(1, 2), whose backward then hands
        visual_inputs.grad over contiguous, without a copy."""
        B, T, N = self.dims
        dx = None
        if not self.embed_frozen:
            dx = self.enc.model._embed_backward(self.rows, dtok, B, T, N, self.Wg, pixel_grad=self.x_grad is not None)
        self.saved = self.rows = self.tok = None
        if dx is None:
            return None   # pixels need no gradient
        return dx.to(self.x_grad[1]).transpose(1, 2)
