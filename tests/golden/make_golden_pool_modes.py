"""Golden vectors for TimeSformer.forward_features(pooling='spatial' | 'none'), from the REFERENCE's own TimeSformer (CPU, fp32, eval mode).

    python -m tests.golden.make_golden_pool_modes     # writes tests/golden/pool_modes_img64_T3_B2.npz, pool_modes_img48_T2_B2.npz

Two small geometries (GEOMETRIES): img_size 64 with 3 frames (N = 16 patches per frame) and img_size 48 with 2 frames (N = 9, odd), 2 clips each.
The encoder stands alone (parameter names 'model. ...'), weights are det_init's closed forms, the drop-path rate is 0.  Per file:
  x                     the clips (B, 3, T, img, img): closed-form values on the 2^-6 grid in [-1.7, 1.7], exact in the fp16 they are stored in
  <mode>/out            forward_features(x, pooling=<mode>)
  grad_norm_names, <mode>/grad_norms
                        gradient norm of EVERY encoder parameter under loss = (out * pool_probe(mode, out.shape)).sum()
  <mode>/grad/<name>    the full gradient (fp32) of the parameters full_grad_names() lists: the final norm, the embeddings (cls_token, pos_embed,
                        time_embed, the patch projection's bias) and every 1-D parameter of the last two blocks.  All gradients in full are 344 MB
                        per mode and one weight matrix of a block is 2.4-9.4 MB, against 1 MiB per committed file; the matrices are covered by
                        their norms.
pool_probe / GEOMETRIES / full_grad_names need no reference and are shared with tests/test_pool_modes_parity.py; main() needs the reference
and never runs on the GPU box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.det_init import fill_state_dict_, unit_uniform  # noqa: E402

GEOMETRIES = [dict(img=64, T=3, B=2), dict(img=48, T=2, B=2)]
MODES = ("spatial", "none")


def fixture_name(geo):
    return "pool_modes_img%d_T%d_B%d.npz" % (geo["img"], geo["T"], geo["B"])


def pool_probe(mode, shape):
    """The fixed weight of the scalar loss: closed form in [-1, 1), one value per output element."""
    return torch.from_numpy(unit_uniform("pool_modes/probe/" + mode, int(np.prod(shape))).astype(np.float32)).view(*shape)


def pool_clips(geo):
    n = geo["B"] * 3 * geo["T"] * geo["img"] * geo["img"]
    v = np.round(1.7 * unit_uniform("pool_modes/x/img%d_T%d" % (geo["img"], geo["T"]), n) * 64.0) / 64.0
    return torch.from_numpy(v.astype(np.float32)).view(geo["B"], 3, geo["T"], geo["img"], geo["img"])


def full_grad_names(named_parameters, depth=12):
    last_two = tuple("model.blocks.%d." % i for i in (depth - 2, depth - 1))
    keep = []
    for n, p in named_parameters:
        if n in ("model.norm.weight", "model.norm.bias", "model.cls_token", "model.pos_embed", "model.time_embed", "model.patch_embed.proj.bias"):
            keep.append(n)
        elif n.startswith(last_two) and p.dim() == 1:
            keep.append(n)
    return keep


def case(TimeSformer, rh, geo):
    _, venc = rh.make_configs(num_frm=geo["T"], img_size=geo["img"])
    venc["drop_path_rate"] = 0
    enc = TimeSformer(venc, input_format="RGB")
    fill_state_dict_(enc)
    enc.eval()
    x = pool_clips(geo)
    g = {"x": x.numpy().astype(np.float16)}
    assert np.array_equal(g["x"].astype(np.float32), x.numpy())
    pd = dict(enc.named_parameters())
    names = [n for n, p in pd.items() if p.requires_grad and not n.startswith("model.head.")]   # (the classification head is outside forward_features)
    g["grad_norm_names"] = np.array(names)
    for mode in MODES:
        for p in pd.values():
            p.grad = None
        out = enc.forward_features(x, return_all_tokens=True, pooling=mode)
        g[mode + "/out"] = out.detach().numpy().astype(np.float32)
        (out * pool_probe(mode, out.shape)).sum().backward()
        assert all(pd[n].grad is not None for n in names)
        g[mode + "/grad_norms"] = np.array([float(pd[n].grad.double().norm()) for n in names], dtype=np.float64)
        for n in full_grad_names(pd.items()):
            g[mode + "/grad/" + n] = pd[n].grad.detach().numpy().astype(np.float32)
    path = os.path.join(HERE, fixture_name(geo))
    np.savez_compressed(path, **g)
    print(fixture_name(geo), os.path.getsize(path), {m: g[m + "/out"].shape for m in MODES})


def main():
    from tests.golden import ref_harness as rh
    rh.import_reference()
    from src.modeling.timesformer.vit import TimeSformer
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for geo in GEOMETRIES:
        case(TimeSformer, rh, geo)


if __name__ == "__main__":
    main()
