"""GPU: the optional batch key `video_ids` in AlproForVideoTextRetrieval, AlproForPretrain (both branches) and Prompter.  Small models as the
other GPU tests build them (VENC, 2 frames of 48 x 48, a 2 + 2 layer BERT), B = 4, exact fp32 mode, training mode with every dropout on.
With distinct ids a step is the step without the key bit for bit (same kernels' values, same RNG consumption); with two captions of one video
the contrastive loss is the fp64 contract's on the model's own features, and the pair is never drawn as a hard negative."""
import numpy as np
import pytest
import torch

from tests import vtc_ids_cases as ic
from tests.conftest import BERT_CFG
from tests.golden.det_init import fill_state_dict_, unit_uniform
from tests.test_host_cpu import VENC, make_cfg

pytestmark = pytest.mark.gpu

B, T, IMG, LT, VOCAB = 4, 2, 48, 10, 2048
DUP_IDS = [5, 5, 6, 7]


def _cfg(**kw):
    return make_cfg(dict(BERT_CFG, num_hidden_layers=4, fusion_layer=2, vocab_size=VOCAB), **kw)


def _batch(with_mlm=False):
    u = lambda name, *shape: torch.from_numpy(unit_uniform("vtc_ids_model/" + name, int(np.prod(shape))).astype(np.float32).reshape(shape))  # noqa: E731
    ids = (110 + torch.floor((u("ids", B, LT) + 1.0) * 0.5 * 1900)).long()
    ids[:, 0] = 101
    mask = torch.ones(B, LT, dtype=torch.long)
    mask[1, LT - 3:] = 0
    ids[1, LT - 3:] = 0
    batch = dict(visual_inputs=1.7 * u("clips", B, T, 3, IMG, IMG), text_input_ids=ids, text_input_mask=mask)
    if with_mlm:
        sel = (u("mlm_sel", B, LT) > 0.5) & (mask > 0)
        sel[:, 0], sel[:, 1] = False, True
        mlm_ids, labels = ids.clone(), torch.full((B, LT), -100, dtype=torch.long)
        mlm_ids[sel] = 103
        labels[sel] = ids[sel]
        batch.update(mlm_text_input_ids=mlm_ids, mlm_labels=labels)
    return {k: v.cuda() for k, v in batch.items()}


def _model(cls, **cfg_kw):
    from alpro_amd import hip
    hip.load()
    m = fill_state_dict_(cls(_cfg(**cfg_kw), dict(VENC, num_frm=T, img_size=IMG)))
    return m.cuda().train()


@pytest.fixture(scope="module")
def retrieval():
    from alpro_amd.modeling.alpro_models import AlproForVideoTextRetrieval
    return _model(AlproForVideoTextRetrieval), _batch()


@pytest.fixture(scope="module")
def pretrain():
    from alpro_amd.modeling.alpro_models import AlproForPretrain
    return _model(AlproForPretrain, num_entities=8)


def _step(m, batch, keys, seed=3, backward=True):
    """One forward (+ backward of the sum of `keys`) in exact fp32 mode under fixed torch and dropout seeds -> (outputs, {name: gradient})."""
    from alpro_amd import config as rt
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(seed)
    rt.seed_dropout(seed)
    with rt.use_compute_dtype("fp32"):
        out = m(batch)
        if backward:
            sum(out[k] for k in keys).backward()
    torch.cuda.synchronize()
    return out, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().reshape(-1).contiguous().view(torch.uint8), b.detach().reshape(-1).contiguous().view(torch.uint8))


def _assert_same_step(m, batch, keys, ids):
    out0, g0 = _step(m, batch, keys)
    out1, g1 = _step(m, dict(batch, video_ids=ids), keys)
    assert set(out0) == set(out1) and set(g0) == set(g1) and len(g0) > 10
    for k in out0:
        if torch.is_tensor(out0[k]):
            assert same_bits(out0[k], out1[k]), "%s changes with distinct video_ids" % k
        else:
            assert out0[k] is None and out1[k] is None, k
    for n in g0:
        assert same_bits(g0[n], g1[n]), "the gradient of %s changes with distinct video_ids" % n
    return out0


def test_retrieval_step_with_distinct_ids_is_the_step_without_the_key(retrieval):
    m, batch = retrieval
    out = _assert_same_step(m, batch, ("itc_loss", "itm_loss"), torch.tensor([11, 1 << 40, 7, (1 << 40) + 7], device="cuda"))
    assert float(out["itc_loss"]) > 0
    _assert_same_step(m, batch, ("itc_loss", "itm_loss"), torch.full((B,), -1, dtype=torch.long, device="cuda"))


def test_retrieval_with_two_captions_of_one_video(retrieval, monkeypatch):
    from alpro_amd.modeling.alpro_models import AlproBaseModel
    m, batch = retrieval
    ids = torch.tensor(DUP_IDS, device="cuda")
    _, grads_plain = _step(m, batch, ("itc_loss", "itm_loss"))
    seen, drawn = {}, []
    orig_vtc, orig_neg = m._vtc, AlproBaseModel.__dict__["_sample_negatives_ids"].__func__

    def vtc(video_feat, text_feat, ids=None):
        seen.update(v=video_feat.detach().float().cpu(), t=text_feat.detach().float().cpu(), ids=ids)
        return orig_vtc(video_feat, text_feat, ids=ids)

    def record(sim_v2t, sim_t2v, bs, ids_):
        drawn.append(tuple(x.cpu() for x in orig_neg(sim_v2t, sim_t2v, bs, ids_)))
        return tuple(x.cuda() for x in drawn[-1])

    def plain(*a):
        raise AssertionError("the plain sampler ran although the batch carries video_ids")
    monkeypatch.setattr(m, "_vtc", vtc)
    monkeypatch.setattr(AlproBaseModel, "_sample_negatives_ids", staticmethod(record))
    monkeypatch.setattr(AlproBaseModel, "_sample_negatives", staticmethod(plain))
    out, grads = _step(m, dict(batch, video_ids=ids), ("itc_loss", "itm_loss"))
    # the contrastive loss: the fp64 contract on the features the model handed to _vtc
    assert seen["ids"] is ids
    temp = m.temp.detach().float().cpu()
    c = ic.IdCase("retrieval_B4", B, B, 256, 0, "model", temp, seen["v"], seen["t"], seen["v"], seen["t"], "model", ids.cpu(), ids.cpu())
    ref, A = ic.reference(c), ic.allowances(c)
    assert int(ic.match(c.ids, c.gids, 0).sum()) == B + 2
    allowed = ic.C["loss"] * float(A["loss"])          # the kernel test's loss allowance, nothing added
    err = abs(float(out["itc_loss"]) - float(ref["loss"]))
    plain_loss = float(ic.reference(c._replace(ids=torch.arange(B), gids=torch.arange(B)))["loss"])
    print("itc_loss %.7f, fp64 contract %.7f (without ids %.7f), error %.3e, allowance %.3e" % (float(out["itc_loss"]), float(ref["loss"]), plain_loss, err, allowed))
    assert err <= allowed, (err, allowed)
    assert abs(plain_loss - float(ref["loss"])) > 4 * allowed          # (the ids matter on this batch)
    # everything after the draw is unchanged
    assert torch.equal(out["itm_labels"].cpu(), torch.tensor([1] * B + [0] * 2 * B)) and out["itm_scores"].shape == (3 * B, 2)
    assert len(drawn) == 1
    # every parameter that the step without the key trains (all but the MLM head, which this model's losses do not reach) has a finite gradient
    assert set(grads) == set(grads_plain) and len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(not same_bits(grads[n], grads_plain[n]) for n in grads)
    # the hard negatives over 20 seeds: rows 0 and 1 are never each other's
    for seed in range(20):
        with torch.no_grad():
            _step(m, dict(batch, video_ids=ids), (), seed=100 + seed, backward=False)
    assert len(drawn) == 21
    for nv, nt in drawn:
        for neg in (nv, nt):
            assert neg.shape == (B,) and int(neg[0]) not in (0, 1) and int(neg[1]) not in (0, 1) and int(neg[2]) != 2 and int(neg[3]) != 3


@pytest.mark.parametrize("with_mlm", [True, False], ids=["batched", "separate"])
def test_pretrain_branches_take_the_key(pretrain, with_mlm):
    """Both branches of AlproForPretrain.forward that call _vtc (one fusion pass over 4B sequences with the MLM pairs; separate passes without
    them): distinct ids leave the step as it is, and with two captions of one video the contrastive loss moves and every gradient is finite."""
    m = pretrain
    batch = _batch(with_mlm=with_mlm)
    keys = ("itc_loss", "itm_loss") + (("mlm_loss",) if with_mlm else ())
    out0 = _assert_same_step(m, batch, keys, 1000 + torch.arange(B, device="cuda"))
    out, grads = _step(m, dict(batch, video_ids=torch.tensor(DUP_IDS, device="cuda")), keys)
    assert not same_bits(out["itc_loss"], out0["itc_loss"]) and torch.equal(out["itm_labels"], out0["itm_labels"])
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_prompter_takes_the_key():
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import Prompter
    m = _model(Prompter, num_entities=8)
    batch = _batch()
    outs = []
    for ids in (None, 1000 + torch.arange(B, device="cuda"), torch.tensor(DUP_IDS, device="cuda")):
        torch.manual_seed(3)
        rt.seed_dropout(3)
        with rt.use_compute_dtype("fp32"):
            outs.append(m(batch if ids is None else dict(batch, video_ids=ids)))
    for k in ("itc_loss", "itc_labels", "i2t_scores", "t2i_scores"):
        assert same_bits(outs[0][k], outs[1][k]), k
    for k in ("itc_labels", "i2t_scores", "t2i_scores"):
        assert same_bits(outs[0][k], outs[2][k]), k
    assert not same_bits(outs[0]["itc_loss"], outs[2]["itc_loss"])
    outs[2]["itc_loss"].backward()
    assert bool(torch.isfinite(m.temp.grad))
