"""GPU: TimeSformer.forward_features(pooling='spatial' | 'none') against the reference's own TimeSformer (tests/golden/pool_modes_*.npz, written by
tests/golden/make_golden_pool_modes.py), under torch.no_grad() and through the anchored autograd node, in exact fp32 mode and in fp16 with the
precise CLS chain (fp16's default).

Limits are the ones tests/test_model_parity.py applies to encoder outputs (video_embeds in test_retrieval_vs_reference) and to parameter gradients
against reference fixtures (test_pretrain_gradients_vs_reference: the relative error of every gradient norm, and full gradients within rtol of their
largest element), read from those tests' own parametrisation.  The fixtures hold the gradient NORM of every encoder parameter but full gradients
only of the final norm, the embeddings and the 1-D parameters of the last two blocks: all gradients in full are 344 MB per mode, one block's weight
matrix alone is 2.4-9.4 MB, a committed file may have 1 MiB.
"""
import os

import numpy as np
import pytest
import torch

from tests import test_model_parity as mp
from tests.conftest import GOLDEN
from tests.golden.det_init import fill_state_dict_
from tests.golden.make_golden_pool_modes import GEOMETRIES, fixture_name, pool_probe
from tests.test_host_cpu import VENC

pytestmark = pytest.mark.gpu

OUT_TOL = {m: tol_emb for m, _, tol_emb in mp.test_retrieval_vs_reference.pytestmark[0].args[1]}          # fp32 1e-3, fp16 6e-3
GRAD_RTOL = dict(mp.test_pretrain_gradients_vs_reference.pytestmark[0].args[1])                            # fp32 5e-3, fp16 1e-2
MODES = ["fp32", "fp16"]
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def cases():
    """geometry index -> (encoder in eval mode on the device, clips, fixture), built once."""
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    built = {}

    def get(i):
        if i not in built:
            geo = GEOMETRIES[i]
            enc = TimeSformer(dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0), input_format="RGB")
            fill_state_dict_(enc)
            g = np.load(os.path.join(GOLDEN, fixture_name(geo)))
            built[i] = (enc.eval().cuda(), torch.from_numpy(g["x"].astype(np.float32)).cuda(), g)
        return built[i]
    return get


# fp16 backward: the fixed loss scale.  4096 is the suite's (test_model_parity.backward / arm_scale) and fits 'temporal' and 'spatial', whose token rows
# receive 1 / T or 1 / N of a probe row.  Under 'none' every token row receives a whole probe row, N times as much: at 4096 the fp16 operands of the
# backward's GEMMs pass 65504 (inf, then NaN in the weight gradients of the early blocks -- the overflow that training answers by backing the dynamic
# scale off).  256 = 4096 / 16 gives the token gradients of 'none' at N = 16 the magnitude that 'spatial' has at 4096.
FP16_SCALE = {"temporal": 4096.0, "spatial": 4096.0, "none": 256.0}


def arm_scale(mode, pooling):
    """test_model_parity.arm_scale with the scale of this pooling: attached before the forward; returns a keep-alive."""
    from alpro_amd import amp, config as rt
    if mode != "fp16":
        return mp.arm_scale(mode)
    sc = amp.LossScaler(init_scale=FP16_SCALE[pooling], dynamic=False, device="cuda")
    rt.set_armed_loss_scaler(sc)
    return sc


def scaled_backward(out, weight, mode, pooling):
    """loss = (out * weight).sum() backward, loss-scaled in fp16 (test_model_parity.backward with the scale of this pooling); returns the factor
    the gradients carry."""
    from alpro_amd import amp, config as rt
    loss = (out * weight).sum()
    if mode != "fp16":
        return mp.backward(loss, mode)
    sc = amp.LossScaler(init_scale=FP16_SCALE[pooling], dynamic=False, device=loss.device)
    rt.set_armed_loss_scaler(sc)
    with rt.loss_scaling(sc):
        (loss * sc.scale.reshape(())).backward()
    return FP16_SCALE[pooling]


@pytest.mark.parametrize("pooling", ["spatial", "none"])
@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
@pytest.mark.parametrize("mode", MODES)
def test_pool_modes_vs_reference(cases, mode, geo, pooling):
    from alpro_amd import config as rt
    enc, x, g = cases(geo)
    ref = g[pooling + "/out"]
    mp.fresh_grads(enc)
    with rt.use_compute_dtype(mode):
        with torch.no_grad():
            out = enc.forward_features(x, return_all_tokens=True, pooling=pooling)
        assert tuple(out.shape) == ref.shape and out.dtype == torch.float32 and not out.requires_grad
        e_inf = mp.close(out, ref, OUT_TOL[mode], what="%s output, no_grad" % pooling)
        keep = arm_scale(mode, pooling)
        out = enc.forward_features(x, return_all_tokens=True, pooling=pooling)
        assert out.requires_grad
        e_trn = mp.close(out, ref, OUT_TOL[mode], what="%s output, autograd" % pooling)
        gs = scaled_backward(out, pool_probe(pooling, out.shape).cuda(), mode, pooling)
        del keep
    pd = dict(enc.named_parameters())
    names = [str(n) for n in g["grad_norm_names"]]
    assert not [n for n in names if pd[n].grad is None], "parameters without a gradient"
    assert not [n for n, p in pd.items() if p.grad is not None and n not in names], "gradients the reference does not have"
    got = np.array([float(pd[n].grad.double().norm()) / gs for n in names])
    want = g[pooling + "/grad_norms"]
    rel = np.abs(got - want) / np.maximum(want, 1e-5)
    worst = int(rel.argmax())
    full = {}
    for k in g.files:
        if k.startswith(pooling + "/grad/"):
            r = g[k].astype(np.float64)
            full[k] = (np.abs(pd[k[len(pooling) + 6:]].grad.float().cpu().numpy().astype(np.float64) / gs - r).max(), np.abs(r).max())
    worst_full = max(full, key=lambda k: full[k][0] / max(full[k][1], 1e-6))
    print("\n[pool modes %s %s img%d] output err %.2e (no_grad) %.2e (autograd), limit %.1e; worst grad-norm rel err %.2e at %s, limit %.1e; "
          "worst full gradient %s: err %.2e of max %.2e" % (mode, pooling, GEOMETRIES[geo]["img"], e_inf, e_trn, OUT_TOL[mode], rel.max(), names[worst],
                                                          GRAD_RTOL[mode], worst_full, *full[worst_full]))
    assert np.isfinite(got).all(), "non-finite gradients: %s" % [n for n, v in zip(names, got) if not np.isfinite(v)][:5]
    assert rel.max() < GRAD_RTOL[mode], (names[worst], got[worst], want[worst])
    assert len(full) >= 6 + 2 * 10
    for k, (e, rmax) in full.items():
        assert e <= GRAD_RTOL[mode] * max(rmax, 1e-6) + 1e-7, (k, e, rmax)


@pytest.mark.parametrize("mode", MODES)
def test_the_three_poolings_agree_with_each_other(cases, mode):
    """B = 2, T = 3, img 64 (N = 16), no fixture: the 'none' output averaged over the frames is the 'temporal' output's patch rows, averaged over the
    patches it is the 'spatial' output's frame rows, and the CLS row is the same LayerNorm of the same token row in all three (bitwise: one
    arithmetic).  The averages here are taken in fp64 from the fp32 'none' output, so the difference is the kernels' own.  Its bound: the k-th of the
    K - 1 fp32 additions rounds a partial sum of at most (k + 1) max |y|, together at most K (K + 1) / 2 * 2^-24 * max |y|, i.e. (K + 1) / 2 * 2^-24
    * max |y| after the division by K, and the multiplication by the rounded 1 / K adds 2 * 2^-24 * max |y|: below (K + 1) * 2^-24 * max |y| for
    K >= 3 (K = T = 3 and K = N = 16 here), max taken over the averaged elements."""
    from alpro_amd import config as rt
    enc, x, _ = cases(0)
    B, T, N = x.shape[0], 3, 16
    with rt.use_compute_dtype(mode), torch.no_grad():
        tmp, spa, non = (enc.forward_features(x, pooling=p) for p in ("temporal", "spatial", "none"))
    assert tuple(tmp.shape) == (B, 1 + N, 768) and tuple(spa.shape) == (B, 1 + T, 768) and tuple(non.shape) == (B, T, 1 + N, 768)
    for t in range(T):
        assert torch.equal(non[:, t, 0], tmp[:, 0]), "CLS row of frame %d ('none') is not the 'temporal' CLS row" % t
    assert torch.equal(spa[:, 0], tmp[:, 0])
    p64 = non[:, :, 1:].double()
    for got, dim, K, what in ((tmp[:, 1:], 1, T, "mean over frames vs 'temporal'"), (spa[:, 1:], 2, N, "mean over patches vs 'spatial'")):
        err = (got.double() - p64.mean(dim)).abs()
        lim = (K + 1) * U24 * p64.abs().amax(dim)
        print("\n[pool cross-check %s] %s: max err %.3e, smallest limit %.3e" % (mode, what, float(err.max()), float(lim.min())))
        assert bool((err <= lim).all()), (what, float((err / lim).max()))


@pytest.mark.parametrize("mode", MODES)
def test_temporal_pooling_is_bitwise_what_it_was(cases, mode):
    """pooling='temporal' (the default) at B = 2, T = 3, img 64: outputs equal hip.vit_final_pool called here on the block stack's output, the
    final norm's gradients equal hip.layernorm_bwd called here on the un-pooled gradient built as before, and every parameter gradient equals the
    one the node built the way it was before the pooling argument existed (_VisualRun(enc)) leaves -- all bit for bit."""
    from alpro_amd import config as rt, hip
    from alpro_amd.modeling import train as tr
    from alpro_amd.modeling.timesformer import vit
    enc, x, _ = cases(0)
    m = enc.model
    B, T, N, D = x.shape[0], 3, 16, 768
    probe = pool_probe("temporal", (B, 1 + N, D)).cuda()
    with rt.use_compute_dtype(mode):
        with torch.no_grad():
            out = enc.forward_features(x)
            tok, T_, W, N_ = m._embed(x)
            tok = vit.run_blocks(m.blocks, tok, B, T_, W)
            direct, _ = hip.vit_final_pool(tok, m.norm.weight, m.norm.bias, vit.VIT_EPS, B, T, N, torch.float32)
        assert (T_, N_) == (T, N) and torch.equal(out, direct) and torch.equal(out, enc.forward_features(x, pooling="temporal"))
        grads = []
        for call in (lambda: enc.forward_features(x, return_all_tokens=True, pooling="temporal"),
                     lambda: tr.run_anchored(vit._VisualRun(enc), [x], list(enc.parameters()))):
            mp.fresh_grads(enc)
            keep = arm_scale(mode, "temporal")
            o = call()
            gs = scaled_backward(o, probe, mode, "temporal")
            del keep
            grads.append((o.detach().clone(), {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}))
        (o1, g1), (o2, g2) = grads
        assert torch.equal(o1, o2) and g1.keys() == g2.keys() and len(g1) > 100
        assert all(torch.equal(g1[n], g2[n]) for n in g1), [n for n in g1 if not torch.equal(g1[n], g2[n])][:5]
        # the final norm's own gradients from the un-pooled gradient, as _VisualRun.backward built it before: tok of the TRAINING forward
        run = vit._VisualRun(enc)
        with torch.no_grad():
            assert torch.equal(run.forward(x), o1)
            dout = probe * gs
            dy = torch.empty((B, 1 + N * T, D), dtype=torch.float32, device="cuda")
            dy[:, 0] = dout[:, 0]
            torch.mul(dout[:, 1:].unsqueeze(2).expand(B, N, T, D), 1.0 / T, out=dy[:, 1:].view(B, N, T, D))
            dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            hip.layernorm_bwd(dy.view(-1, D), run.tok, m.norm.weight, vit.VIT_EPS, torch.empty_like(dy), dg, db, accumulate=False,
                              emit=dict(mode=hip.EMIT_ROWS, rows=B * (1 + N * T), dtype=rt.compute_dtype(), scale=run.saved[-1]["drop_m"], group=1 + N * T))
        assert torch.equal(dg, g1["model.norm.weight"]) and torch.equal(db, g1["model.norm.bias"])
