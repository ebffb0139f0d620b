"""Golden vectors for the pixel gradient of TimeSformer.forward_features, from the REFERENCE's own TimeSformer (CPU, fp32, eval mode) and autograd.

    python -m tests.golden.make_golden_pixel_grad     # writes tests/golden/vit_pixel_grad_img64_T3_B2.npz, vit_pixel_grad_img48_T2_B2.npz

The encoder, its det_init weights, the clips (pool_clips) and the cotangents (pool_probe) are make_golden_pool_modes.py's; here the clip requires
a gradient.  Per file:
  x              the clips (B, 3, T, img, img): on the 2^-6 grid in [-1.7, 1.7], exact in the fp16 they are stored in
  <mode>/out     forward_features(x, pooling=<mode>), fp32, for mode in out_modes(geo): all three at img 48; at img 64 'temporal' alone -- x, the
                 three dx and the three outputs together are 1.33 MB compressed against 1 MiB per committed file, and the 'spatial' and 'none'
                 outputs of this very encoder on these very clips are already in pool_modes_img64_T3_B2.npz (make_golden_pool_modes.py)
  <mode>/dx      d loss / d x, fp32, x's shape, under loss = (out * pool_probe(mode, out.shape)).sum()
fixture_name / MODES need no reference and are shared with the tests; main() needs the reference and never runs on the GPU box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.det_init import fill_state_dict_  # noqa: E402
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips, pool_probe  # noqa: E402

MODES = ("temporal", "spatial", "none")
LIMIT = 1 << 20   # bytes a committed file may have


def fixture_name(geo):
    return "vit_pixel_grad_img%d_T%d_B%d.npz" % (geo["img"], geo["T"], geo["B"])


def out_modes(geo):
    return MODES if geo["img"] <= 48 else ("temporal",)


def case(TimeSformer, rh, geo):
    _, venc = rh.make_configs(num_frm=geo["T"], img_size=geo["img"])
    venc["drop_path_rate"] = 0
    enc = TimeSformer(venc, input_format="RGB")
    fill_state_dict_(enc)
    enc.eval()
    x = pool_clips(geo)
    g = {"x": x.numpy().astype(np.float16)}
    assert np.array_equal(g["x"].astype(np.float32), x.numpy())
    for mode in MODES:
        xr = x.clone().requires_grad_(True)
        out = enc.forward_features(xr, return_all_tokens=True, pooling=mode)
        (out * pool_probe(mode, out.shape)).sum().backward()
        if mode in out_modes(geo):
            g[mode + "/out"] = out.detach().numpy().astype(np.float32)
        g[mode + "/dx"] = xr.grad.numpy().astype(np.float32)
        assert g[mode + "/dx"].shape == tuple(x.shape) and np.isfinite(g[mode + "/dx"]).all() and np.abs(g[mode + "/dx"]).max() > 0
    path = os.path.join(HERE, fixture_name(geo))
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    print(fixture_name(geo), size, "bytes of", LIMIT, {m: float(np.abs(g[m + "/dx"]).max()) for m in MODES})
    assert size < LIMIT, "%s is over the limit for a committed file" % path


def main():
    from tests.golden import ref_harness as rh
    rh.import_reference()
    from src.modeling.timesformer.vit import TimeSformer
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for geo in GEOMETRIES:
        case(TimeSformer, rh, geo)


if __name__ == "__main__":
    main()
