"""Runtime knobs of the MI355X path (not part of the reference's JSON surface; all optional)."""
import contextlib
import os
import weakref

import torch

from alpro_amd import streams

_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16, "fp16": torch.float16,
           "float16": torch.float16, "f32": torch.float32, "fp32": torch.float32, "float32": torch.float32}

# Storage dtype of GEMM / attention operands.  bf16 is the throughput mode BASELINE.json quotes;
# float32 is the exact mode (fp32 MFMA) that reproduces the reference's fp32 arithmetic.
_compute_dtype = _DTYPES[os.environ.get("ALPRO_COMPUTE_DTYPE", "bf16").lower()]


def compute_dtype():
    return _compute_dtype


def set_compute_dtype(dt):
    global _compute_dtype
    _compute_dtype = _DTYPES[dt.lower()] if isinstance(dt, str) else dt
    return _compute_dtype


class use_compute_dtype:
    """Context manager: `with use_compute_dtype(torch.float32): ...`"""

    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        self.prev = compute_dtype()
        set_compute_dtype(self.dt)

    def __exit__(self, *a):
        set_compute_dtype(self.prev)


# ---- runtime switches: each is one _Switch in SWITCHES; the set_* / getter names below are its `set` and the switch itself
_ON, _OFF = ("1", "true", "on"), ("0", "false", "off")
SWITCHES = {}     # name (the * of set_*) -> _Switch


class _Switch:
    """With `decide` (value, *args) -> bool a tri-state switch: it holds a lower-case word (one of _ON, one of _OFF, or its third word, the default)
    and calling it decides for the arguments.  Without: on / off, it holds a bool and calling it returns that."""

    def __init__(self, name, env, default, decide=None, parse=None):
        self.name, self.env, self.default, self.decide = name, env, default, decide
        self.parse = parse or (str.lower if decide else lambda v: v != "0")
        self.read_env()
        SWITCHES[name] = self

    def read_env(self):
        self.value = self.parse(os.environ.get(self.env, self.default))

    def set(self, v):
        self.value = (v.lower() if isinstance(v, str) else ("1" if v else "0")) if self.decide else bool(v)

    def __call__(self, *args, **kw):
        return self.decide(self.value, *args, **kw) if self.decide else self.value

    def __getitem__(self, i):   # switch[0]: the value it holds, which `set` takes back unchanged
        return (self.value,)[i]

    def __setitem__(self, i, v):   # switch[0] = a value read from switch[0] earlier
        self.value = (v,)[i]


@contextlib.contextmanager
def override(*names, **values):
    """`with override("cls_stream", split_streams="0", wgrad_stream=False): ...` -- sets the switches given by keyword as their set_* would and, on
    exit, puts these and the ones merely named (for a block that calls their set_* itself) back to exactly what they held."""
    prev = {n: SWITCHES[n].value for n in (*names, *values)}
    try:
        for n, v in values.items():
            SWITCHES[n].set(v)
        yield
    finally:
        for n, v in prev.items():
            SWITCHES[n].value = v


def _on_or_inference_only(v, training=False):
    return v in _ON or (v == "infer" and not training)


# ---- precise CLS rows (round 4).  The VTC features are projections of one row per sequence (the CLS token); in the 16-bit modes its own
# chain of roundings (LayerNorm output -> q/k/v -> attention output -> projection -> MLP, once per block) carries most of the VTC-logit
# error, and re-evaluating exactly those rows in fp32 costs < 1e-3 of the FLOPs (csrc/cls_precise.hip).
# ALPRO_CLS_PRECISE = auto (default: on with fp16 operands -- the mode that then meets "VTC logits within 1e-3" on every reference fixture;
# off with bf16, whose 8-bit mantissa stays far from the bar either way) | 1 | 0.
_cls_precise = _Switch("cls_precise", "ALPRO_CLS_PRECISE", "auto", lambda v, dt: dt == torch.float16 if v == "auto" else v in _ON)
set_cls_precise = _cls_precise.set
_cls_off = [0]


def cls_precise(dt=None):
    dt = dt if dt is not None else _compute_dtype
    if dt == torch.float32 or _cls_off[0] > 0:
        return False
    return _cls_precise(dt)


def use_cls_precise(v):
    """`with use_cls_precise(False): ...` (tests, bench.py's mode table)."""
    return override(cls_precise=v)


# The chain's launches are skinny (32 ... 512 rows against whole weight matrices: latency, not throughput).  On a second HIP stream, ordered
# against the main path by events (modeling/timesformer/vit.py::_ClsSide), they run beside the block's big launches instead of between them
# (round 5; it rests on the dynamic tile scheduler: a persistent GEMM that finds a CU taken must not wait a round for it).  Measured
# (profiles/r5_cls_stream_ab.txt): B = 32 encoder forward 18.48 -> 18.01 ms, training step unchanged (161.6 ms either way).
# ALPRO_CLS_STREAM = infer (default: the inference forward only) | 1 (training forward too) | 0.
cls_stream = _cls_stream = _Switch("cls_stream", "ALPRO_CLS_STREAM", "infer", _on_or_inference_only)    # cls_stream(training=False)
set_cls_stream = cls_stream.set


# Round 6: the temporal half's qkv Linear and its T-frame attention as ONE launch (alpro_gemm_qkv_tattn: q | k | v are consumed out of the GEMM's
# accumulators; csrc/gemm_tattn.hip).  ALPRO_FUSE_TATTN = infer (default: every no-grad forward -- the retrieval / inference models and, inside a
# training step, the frozen prompter's visual pass) | 1 (the training forward too: the kernel then also writes q | k | v and the log-sum-exp rows
# for the backward) | 0 (the two launches everywhere).  Measured (MI355X, B = 64, fp16, one box): inference form 365 us against 308 + 115 us for
# the two launches inside a step; training form 441 us against the same 423 us -- its 256 x 192 tiles run the K loop at ~975 TF/s where the
# 8-phase qkv GEMM reaches ~1150, so with q | k | v still to be written the fusion does not pay in training and stays off there.
fuse_temporal_attention = _fuse_tattn = _Switch("fuse_temporal_attention", "ALPRO_FUSE_TATTN", "infer", _on_or_inference_only)    # fuse_temporal_attention(training=False)
set_fuse_temporal_attention = fuse_temporal_attention.set


# Round 6: the no-grad encoder forward as two half batches on two HIP streams (modeling/timesformer/vit.py::run_blocks).  Every big launch of a
# block is a persistent kernel whose last round of tiles leaves most CUs idle (the N = 768 projections at B = 32: 591 tiles = 2.3 rounds on 256
# CUs) and the next launch of the same stream depends on it; the other half's launches do not, and the dynamic tile scheduler lets their
# workgroups start on the CUs the first kernel's workgroups have left.  ALPRO_SPLIT_STREAMS = 0 | 1 | auto (default; on for even B >= 16).
def _split_for(v, B):
    if v in _OFF or B % 2 != 0:
        return False
    return B >= (2 if v in _ON else 16)


split_streams = _split_streams = _Switch("split_streams", "ALPRO_SPLIT_STREAMS", "auto", _split_for)    # split_streams(B)
set_split_streams = split_streams.set


def split_lockstep():
    """ALPRO_SPLIT_LOCKSTEP=1: the two streams meet at every block boundary (measurement aid: a block's launches are then bracketed on the launch
    stream); default: they meet once, behind the last block."""
    return os.environ.get("ALPRO_SPLIT_LOCKSTEP", "0") == "1"


# Round 6 (third session): weight gradients on a side stream.  Inside an anchored backward (alpro_amd.modeling.train.Anchor) every 16-bit weight-gradient
# GEMM (alpro_gemm_tn_acc_ws: dW += dY^T X, a leaf of the backward graph -- nothing downstream reads it before the optimizer / the gradient exchange)
# is launched on a second HIP stream behind an event of the launch stream; the launch stream goes on with the data gradient and waits for the side
# stream once, where the backward returns (and before a gradient range is reported final to the exchange).  What it buys is what the two-stream
# forward buys: the weight-gradient kernel's workgroups take the CUs a persistent GEMM's last, partly filled round of tiles leaves idle, and vice
# versa.  Sums are unchanged bit for bit (each kernel's own order; accumulations into one .grad stay ordered on the side stream).
# Measured (profiles/r6_wgrad_side_stream_ab.txt): B = 64 pretrain step -0.3 ... -1.0 % on one box, +0.08 GB peak memory.  ALPRO_WGRAD_STREAM = 0 | 1 (default 1).
wgrad_stream_enabled = _Switch("wgrad_stream", "ALPRO_WGRAD_STREAM", "1")
set_wgrad_stream = wgrad_stream_enabled.set
_wgrad_active = [0]      # > 0 while an anchored backward runs


def _several_ranks():
    """True in a job with more than one rank.  The weight-gradient and prompter side streams are single-GPU schedules unless forced
    (ALPRO_WGRAD_STREAM=force / ALPRO_PROMPTER_STREAM=force): with the collective library's stream the job would have more than four streams in play,
    i.e. streams sharing a hardware queue -- and a weight-gradient kernel queued in front of an all-reduce (or behind one) on a shared queue is exactly
    the coupling the overlapped exchange must not have.  Nothing of this could be measured on more than one GPU; with the text
    side stream alone a rank has launch + collective + text + the prompter's second half-batch stream = four, each on a queue of its own."""
    try:
        import torch.distributed as td
        return td.is_available() and td.is_initialized() and td.get_world_size() > 1
    except Exception:  # noqa: BLE001
        return False


def _forks(switch, device, single_gpu_only=True):
    """True if the role that `switch` governs takes a side stream on `device`: switched on, a GPU, and -- the single-GPU schedules, see
    _several_ranks -- not in a job of several ranks unless the switch's environment variable says `force`."""
    return switch.value and device.type == "cuda" and not (single_gpu_only and _several_ranks() and os.environ.get(switch.env) != "force")


def wgrad_scope(enter):
    """Entering / leaving an anchored backward; returns how many are running now."""
    _wgrad_active[0] += 1 if enter else -1
    return _wgrad_active[0]


def wgrad_side_stream(device):
    """The side stream of the current launch stream, or None when weight gradients stay on the launch stream."""
    if not (_wgrad_active[0] > 0 and _forks(wgrad_stream_enabled, device)):
        return None
    cur = torch.cuda.current_stream(device)
    if streams.TEXT.owns(cur):
        # a backward that already runs on the text side stream keeps its weight gradients there: at most four streams are active at a time (launch, text,
        # weight gradients in backward; launch, text, 2 x prompter in forward) -- the number of hardware queues that do not share a dispatch pipe
        # (profiles/r6_hw_queues.txt: a side stream of the side stream measured 148.75 ms against 148.5; default stream priority: high costs 14 %)
        return None
    ent = streams.WGRAD.get(device, cur)
    ent.pending = True
    return ent.stream


def side_streams_of_current(device):
    """Raw handles of the side streams that carry weight-gradient GEMMs for the current launch stream (created if the switch is on): per-stream
    launch options of the launch stream (FlatAdamW's cu_budget while all-reduces are in flight) have to be mirrored onto them -- the weight-gradient
    kernel plans one workgroup per available CU, and it runs on the side stream now."""
    return [streams.WGRAD.get(device).stream.cuda_stream] if _forks(wgrad_stream_enabled, device) else []


def wgrad_side_event(device):
    """An event behind every weight gradient launched so far on the side stream of the current launch stream, or None if there is none."""
    ent = streams.WGRAD.peek(device)
    return ent.stream.record_event() if (ent is not None and ent.pending) else None


join_wgrad = streams.WGRAD.join     # the current stream of every device waits for the weight gradients that were launched from it


# Round 6 (third session): the pretraining forward's 2B-caption text-encoder pass (M = 2B x 40 rows: 60 ... 240 tiles per Linear, a quarter to all of the
# CUs for a few microseconds each) on a side stream beside the visual encoder's forward, and -- autograd runs a node's backward on the stream of its
# forward -- its backward beside the visual encoder's backward.  The launch stream waits for the side stream where the text rows are first needed
# (the VTC features); the side stream's parameter gradients are handed to the caller's stream by an end-of-backward callback, and any gradient range
# reported final to the exchange (N > 1) waits for the side stream first.  Measured (profiles/r6_text_side_stream_ab.txt): B = 64 pretrain step
# 151.7 -> 149.4 ms (-1.5 %, A/B/A/B on one box), outputs and gradients bit for bit, +0.14 GB.  ALPRO_TEXT_STREAM = 0 | 1 (default 1).
text_stream_enabled = _Switch("text_stream", "ALPRO_TEXT_STREAM", "1")
set_text_stream = text_stream_enabled.set


def text_side_stream(device):
    return streams.TEXT.get(device).stream if _forks(text_stream_enabled, device, single_gpu_only=False) else None


is_text_side_stream = streams.TEXT.owns
join_text_streams = streams.TEXT.join     # the current stream waits for every text side stream that was forked from it (gradient ranges about to go on the wire)


# Third session: the frozen prompter's pass (get_pseudo_labels: a no-grad B-clip encoder forward, itself two half batches on two streams)
# forked BEHIND the trained visual encoder's forward, so that it runs beside the VTC / negative sampling / fusion / head launches of the launch stream
# instead of after them.  Forked at the START of the forward it ran beside the visual encoder's forward and cost +0.2 ... +0.7 % (profiles/r6_split_streams_ab.txt:
# big beside big); forked behind it: 150.47 -> 150.09 ms (-0.25 %, A/B/A/B on one box, run-to-run spread 0.03 ms; profiles/r6_prompter_side_stream_ab.txt),
# labels bit for bit.  ALPRO_PROMPTER_STREAM = 0 | 1 (default 1).
prompter_stream_enabled = _Switch("prompter_stream", "ALPRO_PROMPTER_STREAM", "1")
set_prompter_stream = prompter_stream_enabled.set


def prompter_side_stream(device):
    return streams.PROMPTER.get(device).stream if _forks(prompter_stream_enabled, device) else None


# Round 6: the no-grad Block.forward keeps the block input until both attention halves are done -- the add + norm1 kernel reads it and writes only the
# normalised rows, the add + norm2 kernel adds the temporal AND the spatial branch (alpro_add_layernorm_pre_mlp2; bit for bit the same sums).
# ALPRO_DEFER_TEMPORAL_ADD=0: the round-3 form (x + temporal branch written by the first kernel), for A/B.
defer_temporal_add = _defer_tadd = _Switch("defer_temporal_add", "ALPRO_DEFER_TEMPORAL_ADD", "1")
set_defer_temporal_add = defer_temporal_add.set


# Recompute the ViT blocks' activations in backward.  Off (default): the anchored visual backward keeps every activation
# of the step (~37 KB per token row and block).  On: each trainable block keeps its input, its three drop-path scale vectors and its two
# attention-dropout seeds (~3 KB per row) and its forward_train body runs once more right before its backward -- the same kernels on the same
# operands, so outputs, gradients and both random streams are those of the stored step bit for bit, at the price of one more ViT training forward.
# ALPRO_RECOMPUTE = 0 | 1 (default 0), read at every _VisualRun.forward.  `video_enc_cfg.gradient_checkpointing` does NOT set it.
def _zero_or_one(v):
    v = v.strip()
    if v not in ("0", "1"):
        raise ValueError("ALPRO_RECOMPUTE=%r: expected 0 (keep every ViT block activation, the default) or 1 (recompute them in backward)" % v)
    return v == "1"


recompute_blocks = _Switch("recompute", "ALPRO_RECOMPUTE", "0", parse=_zero_or_one)
set_recompute = recompute_blocks.set


def use_recompute(flag):
    """Context manager: `with use_recompute(True): loss = model(batch); loss.backward()` (the switch is read by the forward; the backward
    follows what its forward kept)."""
    return override(recompute=flag)


class cls_precise_off:
    """Passes whose CLS row feeds no VTC logit (the frozen teacher's pseudo-label pass) skip the side path."""

    def __enter__(self):
        _cls_off[0] += 1

    def __exit__(self, *a):
        _cls_off[0] -= 1


# ---- fp16 operands: loss scaling (alpro_amd.amp).  The hand-written backward passes refuse to run on fp16 gradient operands unless the
# loss was scaled (an unscaled fp16 backward silently flushes most activation gradients to zero); the LM head writes its logit gradient
# at FORWARD time and therefore needs to know the scale that the coming backward will use ("armed" scaler).
_scaling = [None]   # the LossScaler of the scale_loss context we are inside, else None
_armed = [None]     # weakref to the most recently attached LossScaler


def set_armed_loss_scaler(scaler):
    _armed[0] = weakref.ref(scaler) if scaler is not None else None


def armed_loss_scale(device):
    """(1,) device tensor holding the loss scale the next backward will carry, or None (not fp16 / no scaler attached)."""
    if _compute_dtype != torch.float16 or _armed[0] is None:
        return None
    sc = _armed[0]()
    return None if sc is None else sc.to(device).scale


class loss_scaling:
    """`with loss_scaling(scaler): scaled_loss.backward()` -- marks the backward as scaled."""

    def __init__(self, scaler):
        self.scaler = scaler

    def __enter__(self):
        self.prev = _scaling[0]
        _scaling[0] = self.scaler
        return self.scaler

    def __exit__(self, *a):
        _scaling[0] = self.prev


def loss_scaling_active():
    return _scaling[0] is not None


def check_backward_precision(dt):
    """Called by every hand-written backward: fp16 gradient operands without loss scaling are refused loudly."""
    if dt == torch.float16 and _scaling[0] is None and os.environ.get("ALPRO_ALLOW_UNSCALED_FP16_BACKWARD", "0") != "1":
        raise RuntimeError("fp16 operands: the backward pass needs a scaled loss (activation gradients underflow fp16's range otherwise). Use "
                           "`optimizer.backward(loss)` (alpro_amd.optim.FlatAdamW) or `with amp.scale_loss(loss, optimizer) as s: s.backward()` "
                           "(alpro_amd.amp / the apex.amp facade), or pick bf16 / fp32 operands (ALPRO_COMPUTE_DTYPE).")


# ---- dropout seeds: the HIP kernels draw masks from hash(seed, element index); every dropout site of every forward
# gets a fresh 31-bit seed from this counter-based stream (deterministic given seed_dropout()).
#
# Seeding: unless seed_dropout() was called explicitly, the stream is keyed on first use by torch.initial_seed() (what the
# reference's set_random_seed -> torch.manual_seed controls, src/utils/misc.py:20-24) plus the data-parallel rank, so a different run
# seed gives different masks and the ranks of one job do not drop the same element indices.
_drop_state = [None, 0]


def seed_dropout(seed):
    _drop_state[0] = int(seed) & 0x7FFFFFFF
    _drop_state[1] = 0


def dropout_state():
    """(seed, counter) of the stream: the seed is None until first use, the counter is the number of seeds drawn since seed_dropout()."""
    return tuple(_drop_state)


def _auto_seed():
    import torch.distributed as td
    rank = td.get_rank() if (td.is_available() and td.is_initialized()) else 0
    seed_dropout((torch.initial_seed() * 0x9E3779B1 + rank * 0x85EBCA77 + 0x1234567) & 0x7FFFFFFF)


def next_dropout_seed():
    if _drop_state[0] is None:
        _auto_seed()
    _drop_state[1] += 1
    x = (_drop_state[0] * 0x9E3779B1 + _drop_state[1] * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    return (x & 0x7FFFFFFF) | 1  # never 0 (0 means "dropout off" in the C ABI)
