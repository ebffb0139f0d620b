"""Golden vectors for TimeSformer.forward_features(attn_grads=VitAttnGradients(...)), from the REFERENCE's own TimeSformer (CPU, fp32, eval mode):
the gradient of a score w.r.t. the softmax of every attention, reached the way the reference's users reach it -- retain_grad() on the input of
attn.attn_drop / temporal_attn.attn_drop (vit.py:92-93), set by a forward pre-hook.

    python -m tests.golden.make_golden_vit_gradcam     # writes tests/golden/vit_gradcam_img48_T2_B2.npz, vit_gradcam_img64_T3_B2.npz

Geometries, weights (det_init's closed forms), clips and drop-path rate 0 are make_golden_pool_modes'; the score is
(features * pool_probe("temporal", features.shape)).sum() with features = forward_features(x) (temporal pooling).  Per file:
  temporal_grad/<i>   G = d score / d P of the temporal map of every block i, (B*N, 12, T, T)
  spatial_grad/<i>    G of the spatial map of the blocks SPATIAL_BLOCKS, (B*T, 12, 1+N, 1+N) -- all 24 raw maps at img 64 are 1.16 MB uncompressed,
                      against 1 MiB per committed file
  features            forward_features(x)
The maps P themselves are in the vit_attn_* fixtures (make_golden_vit_attn: same weights, clips and blocks) and are not stored again.  The script
prints every stored map's figures and refuses a degenerate one: the share of positive entries outside [0.4, 0.6], a query row that is all
zero, or max |G| below 0.5.  main() needs the reference and never runs on the GPU machine.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.det_init import fill_state_dict_  # noqa: E402
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips, pool_probe  # noqa: E402
from tests.golden.make_golden_vit_attn import DEPTH, SPATIAL_BLOCKS  # noqa: E402


def fixture_name(geo):
    return "vit_gradcam_img%d_T%d_B%d.npz" % (geo["img"], geo["T"], geo["B"])


def case(TimeSformer, rh, geo):
    _, venc = rh.make_configs(num_frm=geo["T"], img_size=geo["img"])
    venc["drop_path_rate"] = 0
    enc = TimeSformer(venc, input_format="RGB")
    fill_state_dict_(enc)
    enc.eval()
    x = pool_clips(geo)
    B, T, N = geo["B"], geo["T"], (geo["img"] // 16) ** 2
    spatial, temporal = [], []
    blocks = enc.model.blocks
    assert len(blocks) == DEPTH

    def retain(store):
        def hook(m, args):
            args[0].retain_grad()
            store.append(args[0])
        return hook

    handles = []
    for blk in blocks:
        handles.append(blk.attn.attn_drop.register_forward_pre_hook(retain(spatial)))
        handles.append(blk.temporal_attn.attn_drop.register_forward_pre_hook(retain(temporal)))
    feats = enc.forward_features(x, return_all_tokens=True, pooling="temporal")
    for h in handles:
        h.remove()
    (feats * pool_probe("temporal", feats.shape)).sum().backward()
    assert len(spatial) == DEPTH and len(temporal) == DEPTH
    assert all(tuple(m.grad.shape) == (B * T, 12, 1 + N, 1 + N) for m in spatial) and all(tuple(m.grad.shape) == (B * N, 12, T, T) for m in temporal)
    g = {"features": feats.detach().numpy().astype(np.float32)}
    for i in range(DEPTH):
        g["temporal_grad/%d" % i] = temporal[i].grad.numpy().astype(np.float32)
        if i in SPATIAL_BLOCKS:
            g["spatial_grad/%d" % i] = spatial[i].grad.numpy().astype(np.float32)
    for k in sorted((k for k in g if "/" in k), key=lambda k: (k.split("/")[0], int(k.split("/")[1]))):
        m = g[k]
        pos, zero_rows, top = float((m > 0).mean()), int((np.abs(m).max(-1) == 0).sum()), float(np.abs(m).max())
        print("  %-18s %-18s positive share %.3f, all-zero query rows %d, max |G| %.3e" % (k, m.shape, pos, zero_rows, top))
        assert np.isfinite(m).all()
        assert 0.4 <= pos <= 0.6, "%s: positive share %.3f outside [0.4, 0.6]" % (k, pos)
        assert zero_rows == 0, "%s: %d query rows are all zero" % (k, zero_rows)
        assert top >= 0.5, "%s: max |G| %.3e below 0.5" % (k, top)
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
