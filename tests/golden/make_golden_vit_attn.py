"""Golden vectors for TimeSformer.forward_features(output_attentions=True, output_hidden_states=True), from the REFERENCE's own TimeSformer (CPU,
fp32, eval mode) observed through the hooks its users work with.

    python -m tests.golden.make_golden_vit_attn     # writes tests/golden/vit_attn_img48_T2_B2.npz, vit_attn_img64_T3_B2.npz

Geometries, weights (det_init's closed forms as they are: no gain on q / k), clips and drop-path rate 0 are make_golden_pool_modes'.  Hooks:
  forward pre-hook on every block's attn.attn_drop / temporal_attn.attn_drop   the softmax of vit.py:92-93, (B*T, 12, 1+N, 1+N) / (B*N, 12, T, T)
  forward hook on every block, forward pre-hook on block 0                     the 13 hidden states (B, 1 + N*T, 768)
Per file:
  temporal/<i>   the temporal map of every block i
  spatial/<i>    the spatial map of the blocks SPATIAL_BLOCKS
  hidden_rows    (13, B, 3, 768): the rows HIDDEN_ROWS(N, T) = CLS, first patch of frame 0, last patch of the last frame of every hidden state
  features       forward_features(x) (temporal pooling)
The clips are the pool-modes fixture's `x` (pool_clips) and are not stored again.  The script prints every stored map's peak and refuses a map
whose peak is above 0.95 (saturated) or below 1.5 x uniform (flat).  Two-key maps (T = 2) are the exception to the floor: 1.5 x uniform is 0.75
there, half way to the largest value a probability can take, and the reference's maps peak at 0.741-0.823 per block with these weights and
clips (log-odds of 1.05 and more between the two frames: not flat); their floor is 0.74.  main() needs the reference and never runs on the GPU
machine.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.det_init import fill_state_dict_  # noqa: E402
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips  # noqa: E402

SPATIAL_BLOCKS = (0, 5, 11)
DEPTH = 12


def fixture_name(geo):
    return "vit_attn_img%d_T%d_B%d.npz" % (geo["img"], geo["T"], geo["B"])


def hidden_rows(N, T):
    """Token rows of a hidden state that the fixture keeps: CLS, the first patch of frame 0 (token 1 + 0*T + 0), the last patch of the last frame."""
    return (0, 1, N * T)


def case(TimeSformer, rh, geo):
    _, venc = rh.make_configs(num_frm=geo["T"], img_size=geo["img"])
    venc["drop_path_rate"] = 0
    enc = TimeSformer(venc, input_format="RGB")
    fill_state_dict_(enc)
    enc.eval()
    x = pool_clips(geo)
    B, T, N = geo["B"], geo["T"], (geo["img"] // 16) ** 2
    spatial, temporal, hidden = [], [], []
    blocks = enc.model.blocks
    assert len(blocks) == DEPTH
    handles = [blocks[0].register_forward_pre_hook(lambda m, args: hidden.append(args[0].detach().clone()))]
    for blk in blocks:
        handles.append(blk.attn.attn_drop.register_forward_pre_hook(lambda m, args: spatial.append(args[0].detach().clone())))
        handles.append(blk.temporal_attn.attn_drop.register_forward_pre_hook(lambda m, args: temporal.append(args[0].detach().clone())))
        handles.append(blk.register_forward_hook(lambda m, args, out: hidden.append(out.detach().clone())))
    with torch.no_grad():
        feats = enc.forward_features(x, return_all_tokens=True, pooling="temporal")
    for h in handles:
        h.remove()
    assert len(spatial) == DEPTH and len(temporal) == DEPTH and len(hidden) == DEPTH + 1
    assert all(tuple(m.shape) == (B * T, 12, 1 + N, 1 + N) for m in spatial) and all(tuple(m.shape) == (B * N, 12, T, T) for m in temporal)
    assert all(tuple(h.shape) == (B, 1 + N * T, 768) for h in hidden)
    g = {"features": feats.numpy().astype(np.float32),
         "hidden_rows": np.stack([h[:, list(hidden_rows(N, T))].numpy() for h in hidden]).astype(np.float32)}
    for i in range(DEPTH):
        g["temporal/%d" % i] = temporal[i].numpy().astype(np.float32)
        if i in SPATIAL_BLOCKS:
            g["spatial/%d" % i] = spatial[i].numpy().astype(np.float32)
    for k in sorted(g, key=lambda k: (k.split("/")[0], int(k.split("/")[1]) if "/" in k else 0)):
        if "/" not in k:
            continue
        peak, uniform = float(g[k].max()), 1.0 / g[k].shape[-1]
        print("  %-12s %-18s peak %.3f (uniform %.3f)" % (k, g[k].shape, peak, uniform))
        assert peak <= 0.95, "%s is saturated (peak %.3f)" % (k, peak)
        floor = 0.74 if g[k].shape[-1] == 2 else 1.5 * uniform   # (module docstring)
        assert peak >= floor, "%s is flat (peak %.3f, uniform %.3f)" % (k, peak, uniform)
        assert np.abs(g[k].astype(np.float64).sum(-1) - 1.0).max() < 1e-5
    path = os.path.join(HERE, fixture_name(geo))
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    print(fixture_name(geo), size, "bytes")
    assert size < 1 << 20


def main():
    from tests.golden import ref_harness as rh
    rh.import_reference()
    from src.modeling.timesformer.vit import TimeSformer
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for geo in GEOMETRIES:
        case(TimeSformer, rh, geo)


if __name__ == "__main__":
    main()
