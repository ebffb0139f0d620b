"""GPU: multi-clip retrieval evaluation (inference_n_clips = 3, score_agg_func mean / max / lse) on the retrieval_T2 fixture model against
tests/golden/retrieval_clips_T2_V4_C3.npz -- the REFERENCE's forward_inference once per clip for 4 videos x 3 clips x 2 frames and 5
captions, pooled over the clips in fp64 (tests/golden/make_golden_ret_clips.py) -- and the two-stage search with clips (rerank_retrieval:
hip.sim_topk_clips, score_pair_list over the clips, hip.clip_pool) against the all-pairs evaluation it shortcuts.

Tolerances: those of tests/test_model_parity.py::test_batched_retrieval_scoring_vs_reference_records for one clip -- 2e-4 / 1e-3 / 8e-3 on
the match probability in fp32 / fp16 / bf16 mode, five times that on the similarity.  mean, max and lse are 1-Lipschitz in the sup norm, and
so is the softmax probability in the logits' sup norm up to a factor 1/2, so pooling does not enlarge them; the 4-decimal rounding of the
records adds 5e-5."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.test_host_cpu import VENC, make_cfg

pytestmark = pytest.mark.gpu

V, N, C, T = 4, 3, 5, 2
TOL = 2e-4                       # tests/test_rerank_gpu.py: two paths of this model in fp32 mode
MODES = ("mean", "max", "lse")
KEYS = ("t2v_idx", "t2v_sim", "t2v_score", "v2t_idx", "v2t_sim", "v2t_score")
VID_IDS, TXT_IDS = ["v%d" % v for v in range(V)], ["t%d" % c for c in range(C)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "retrieval_clips_T2_V4_C3.npz"))


@pytest.fixture(scope="module")
def setup(bert_cfg, golden):
    """(model, videos (4, 6, C, H, W), caption ids, mask, the fp32-mode (score, sim) of score_all_pairs per mode) -- computed once for the module"""
    from tests.golden import parity_cases as pc
    from tests.golden.det_init import det_batch
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import score_all_pairs
    m = pc.build_case("retrieval_T2", bert_cfg, VENC, make_cfg, "cuda")[0]
    batch = det_batch(V * N, T, seed_name=str(golden["seed_name"]), with_mlm=False, with_mpm=False)
    vis = batch["visual_inputs"]
    videos = vis.view((V, N * T) + tuple(vis.shape[2:])).cuda()          # clip j of video v = row v * 3 + j of the batch: frames 2j, 2j + 1 of the video
    ids, mask = batch["text_input_ids"][:C].cuda(), batch["text_input_mask"][:C].cuda()
    with rt.use_compute_dtype("fp32"):
        full = {mode: tuple(t.clone() for t in score_all_pairs(m, videos, ids, mask, pair_bsz=7, num_clips=N, score_agg_func=mode)) for mode in MODES}
    return m, videos, ids, mask, full


def _err(got, want):
    return float(np.abs(got.detach().double().cpu().numpy() - want).max())


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-4), ("fp16", 1e-3), ("bf16", 8e-3)])
@pytest.mark.parametrize("mode", MODES)
def test_pooled_scores_sims_and_records_vs_the_reference(setup, golden, mode, dtype, tol):
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import eval_retrieval, inference_retrieval_cached, score_all_pairs
    m, videos, ids, mask, full = setup
    with rt.use_compute_dtype(dtype):
        score, sim = full[mode] if dtype == "fp32" else score_all_pairs(m, videos, ids, mask, pair_bsz=7, num_clips=N, score_agg_func=mode)
        recs = inference_retrieval_cached(m, [(VID_IDS[v], videos[v:v + 1]) for v in range(V)], ids, mask, TXT_IDS, eval_bsz=3, num_clips=N,
                                          score_agg_func=mode)
    assert score.is_cuda and score.shape == sim.shape == (V, C) and score.dtype == sim.dtype == torch.float32
    e_score, e_sim = _err(score, golden["score/" + mode]), _err(sim, golden["sim/" + mode])
    assert [(r["vid_id"], r["txt_id"]) for r in recs] == [(v, t) for v in VID_IDS for t in TXT_IDS]
    rs, rm = (np.array([r[key] for r in recs]).reshape(V, C) for key in ("score", "sim"))
    e_rs, e_rm = np.abs(rs - golden["rec_score/" + mode]).max(), np.abs(rm - golden["rec_sim/" + mode]).max()
    print("%s %s: score err %.3e (tol %.1e), sim err %.3e (tol %.1e); records: score %.3e, sim %.3e" % (mode, dtype, e_score, tol, e_sim, 5 * tol, e_rs, e_rm))
    assert e_score <= tol and e_sim <= 5 * tol
    assert e_rs <= tol + 5e-5 and e_rm <= 5 * tol + 5e-5          # both sides rounded to 4 decimals
    assert all(r["score"] == round(r["score"], 4) and r["sim"] == round(r["sim"], 4) for r in recs)
    if dtype == "fp32":
        metrics = eval_retrieval(recs, {TXT_IDS[c]: VID_IDS[c % V] for c in range(C)})
        for d in ("text2video", "video2text"):
            for key in ("r1", "r5", "r10", "medianR", "meanR"):
                assert float(metrics[d][key]) == float(golden["%s/%s/%s" % (mode, d, key)]), (mode, d, key, metrics[d][key])


def _rerank(setup, mode, k=2, pair_bsz=4):
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import encode_captions, encode_gallery, rerank_retrieval
    m, videos, ids, mask, _ = setup
    with rt.use_compute_dtype("fp32"):
        ve, vf = encode_gallery(m, videos, bsz=5, num_clips=N)
        te, tf = encode_captions(m, ids, mask)
        assert ve.shape[0] == vf.shape[0] == V * N
        return rerank_retrieval(m, ve, vf, te, tf, mask, k, pair_bsz=pair_bsz, num_clips=N, score_agg_func=mode)


@pytest.mark.parametrize("mode", MODES)
def test_rerank_with_clips_candidates_sims_and_scores(setup, mode):
    score, sim = setup[4][mode]
    out = _rerank(setup, mode)
    for d, rows, S, P in (("t2v", C, sim.t().contiguous(), score.t().contiguous()), ("v2t", V, sim, score)):
        idx = out[d + "_idx"].long()
        assert idx.shape == (rows, 2) and out[d + "_idx"].dtype == torch.int32
        want = torch.topk(S, 2, dim=1)[1]
        assert torch.equal(idx.sort(1)[0], want.sort(1)[0]), (mode, d, idx.tolist(), want.tolist())
        e_sim = float((out[d + "_sim"] - S.gather(1, idx)).abs().max())
        e_score = float((out[d + "_score"] - P.gather(1, idx)).abs().max())
        print("%s %s: sim err %.3e, score err %.3e" % (mode, d, e_sim, e_score))
        assert e_sim <= TOL and e_score <= TOL, (mode, d, e_sim, e_score)
        assert bool((out[d + "_sim"][:, 0] >= out[d + "_sim"][:, 1]).all())
    again = _rerank(setup, mode)
    for key in KEYS:
        assert torch.equal(out[key], again[key]), (mode, key)


@pytest.mark.parametrize("mode", MODES)
def test_rerank_with_clips_pads_rows_when_k_exceeds_the_gallery(setup, mode):
    from alpro_amd.retrieval_eval import rerank_metrics
    score = setup[4][mode][0]
    out = _rerank(setup, mode, k=10, pair_bsz=512)
    for d, rows, n, P, gt in (("t2v", C, V, score.t(), torch.arange(C) % V), ("v2t", V, C, score, torch.arange(V))):
        idx = out[d + "_idx"].long()
        assert torch.equal(idx[:, :n].sort(1)[0], torch.arange(n, device="cuda").repeat(rows, 1)) and bool((idx[:, n:] == -1).all())
        assert bool(torch.isneginf(out[d + "_sim"][:, n:]).all()) and bool(torch.isneginf(out[d + "_score"][:, n:]).all())
        assert float((out[d + "_score"][:, :n] - P.gather(1, idx[:, :n])).abs().max()) <= TOL
        mt = rerank_metrics(out[d + "_idx"], out[d + "_score"], out[d + "_sim"], gt)
        assert mt["outside"] == 0 and mt["r5"] == 100.0 and 1 <= mt["medianR"] <= n


def test_one_clip_returns_exactly_what_the_calls_return_without_the_keyword(setup):
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import encode_captions, encode_gallery, inference_retrieval_cached, rerank_retrieval, score_all_pairs
    m, videos, ids, mask, _ = setup
    one = videos[:, :T].contiguous()                                  # the first clip of every video
    vids = [(VID_IDS[v], one[v:v + 1]) for v in range(V)]
    with rt.use_compute_dtype("fp32"):
        a, b = score_all_pairs(m, one, ids, mask, pair_bsz=7), score_all_pairs(m, one, ids, mask, pair_bsz=7, num_clips=1, score_agg_func="lse")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert inference_retrieval_cached(m, vids, ids, mask, TXT_IDS, eval_bsz=3) == inference_retrieval_cached(m, vids, ids, mask, TXT_IDS, eval_bsz=3, num_clips=1,
                                                                                                                 score_agg_func="max")
        (ve, vf), (ve1, vf1) = encode_gallery(m, one), encode_gallery(m, one, num_clips=1)
        assert torch.equal(ve, ve1) and torch.equal(vf, vf1)
        te, tf = encode_captions(m, ids, mask)
        r, r1 = rerank_retrieval(m, ve, vf, te, tf, mask, 2, pair_bsz=3), rerank_retrieval(m, ve, vf, te, tf, mask, 2, pair_bsz=3, num_clips=1, score_agg_func="lse")
        for key in KEYS:
            assert torch.equal(r[key], r1[key]), key
