"""GPU: the two-stage retrieval search (alpro_amd/retrieval_eval.py rerank_retrieval, AlproForVideoTextRetrieval.score_pair_list) against the
all-pairs evaluation it shortcuts (score_all_pairs), on the retrieval_T2 fixture model (closed-form weights, 2 frames) with the 5 videos x
5 captions of tests/golden/retrieval_eval_T2_V5.npz, exact fp32 mode.  2e-4 is the tolerance tests/test_long_text_parity.py uses for the
ITM match probability between two paths of this model."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_host_cpu import VENC, make_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 5
TOL = 2e-4
PAIR_ORDER = np.random.RandomState(11).permutation(V * V)   # all 25 pairs, shuffled: pair id = vi * 5 + ci


def _build(bert_cfg):
    from tests.golden import parity_cases as pc
    from tests.golden.det_init import det_batch
    m = pc.build_case("retrieval_T2", bert_cfg, VENC, make_cfg, "cuda")[0]
    batch = det_batch(V, 2, seed_name="retrieval_eval_T2", with_mlm=False, with_mpm=False)
    return m, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


def _pair_probabilities(m, batch):
    """softmax(score_pair_list logits)[:, 1] of the 25 pairs in PAIR_ORDER, 7 at a time (uneven mini-batches), fp32 mode"""
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import encode_captions, encode_gallery
    with rt.use_compute_dtype("fp32"):
        ve, _ = encode_gallery(m, batch["visual_inputs"], bsz=2)
        te, _ = encode_captions(m, batch["text_input_ids"], batch["text_input_mask"], bsz=3)
        order = torch.from_numpy(PAIR_ORDER).cuda()
        out = []
        for s in range(0, order.numel(), 7):
            p = order[s:s + 7]
            logits = m.score_pair_list(ve, te, batch["text_input_mask"], p // V, p % V)
            assert logits.shape == (p.numel(), 2) and logits.dtype == torch.float32
            out.append(torch.softmax(logits, dim=1)[:, 1])
    return torch.cat(out).cpu().numpy()


@pytest.fixture(scope="module")
def setup(bert_cfg):
    """(model, batch, cached features, score_all_pairs' (score, sim)) -- built and computed once for the module"""
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import encode_captions, encode_gallery, score_all_pairs
    m, batch = _build(bert_cfg)
    with rt.use_compute_dtype("fp32"):
        score, sim = score_all_pairs(m, batch["visual_inputs"], batch["text_input_ids"], batch["text_input_mask"], pair_bsz=7)
        ve, vf = encode_gallery(m, batch["visual_inputs"])
        te, tf = encode_captions(m, batch["text_input_ids"], batch["text_input_mask"])
    return m, batch, (ve, vf, te, tf), score.clone(), sim.clone()


def test_score_pair_list_matches_score_all_pairs(setup):
    m, batch, _, score, _ = setup
    got = _pair_probabilities(m, batch)
    want = score.cpu().numpy().reshape(-1)[PAIR_ORDER]
    err = np.abs(got.astype(np.float64) - want)
    print("score_pair_list vs score_all_pairs: max err %.3e" % err.max())
    assert err.max() <= TOL
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.score_pair_list(None, None, None, None, None)
    finally:
        m.eval()


def test_score_pair_list_with_the_tail_on_every_row_in_a_child_process(setup, tmp_path):
    """ALPRO_FUSION_TAIL_ROWS=0 (the last fusion layer's tail on every row instead of the [CLS] rows) in a fresh process, same tolerance."""
    score = setup[3]
    out = str(tmp_path / "pairs.npy")
    env = dict(os.environ, ALPRO_FUSION_TAIL_ROWS="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    err = np.abs(got.astype(np.float64) - score.cpu().numpy().reshape(-1)[PAIR_ORDER])
    print("score_pair_list (tail on every row) vs score_all_pairs: max err %.3e" % err.max())
    assert err.max() <= TOL


def _rerank(setup, k=2, pair_bsz=3):
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import rerank_retrieval
    m, batch, (ve, vf, te, tf), _, _ = setup
    with rt.use_compute_dtype("fp32"):
        return rerank_retrieval(m, ve, vf, te, tf, batch["text_input_mask"], k, pair_bsz=pair_bsz)


def test_rerank_retrieval_candidates_sims_and_scores(setup):
    score, sim = setup[3], setup[4]
    out = _rerank(setup)
    for d, idx_key, sim_key, score_key, S, P in (("t2v", "t2v_idx", "t2v_sim", "t2v_score", sim.t().contiguous(), score.t().contiguous()),
                                                 ("v2t", "v2t_idx", "v2t_sim", "v2t_score", sim, score)):
        idx = out[idx_key].long()
        assert idx.shape == (V, 2) and out[idx_key].dtype == torch.int32
        want = torch.topk(S, 2, dim=1)[1]
        assert torch.equal(idx.sort(1)[0], want.sort(1)[0]), (d, idx.tolist(), want.tolist())
        e_sim = float((out[sim_key] - S.gather(1, idx)).abs().max())
        e_score = float((out[score_key] - P.gather(1, idx)).abs().max())
        print("%s: sim err %.3e, score err %.3e" % (d, e_sim, e_score))
        assert e_sim <= TOL and e_score <= TOL, (d, e_sim, e_score)
        assert bool((out[sim_key][:, 0] >= out[sim_key][:, 1]).all())


def test_rerank_retrieval_pads_rows_when_k_exceeds_the_gallery(setup):
    """k = 10 of 5: every pair is a candidate (each scored once), the tail of every row is idx -1 / sim -inf / score -inf, and rerank_metrics
    takes the result as it stands."""
    from alpro_amd.retrieval_eval import rerank_metrics
    score = setup[3]
    out = _rerank(setup, k=10, pair_bsz=512)
    for d, P in (("t2v", score.t()), ("v2t", score)):
        idx = out[d + "_idx"].long()
        assert torch.equal(idx[:, :V].sort(1)[0], torch.arange(V, device="cuda").repeat(V, 1)) and bool((idx[:, V:] == -1).all())
        assert bool(torch.isneginf(out[d + "_sim"][:, V:]).all()) and bool(torch.isneginf(out[d + "_score"][:, V:]).all())
        assert float((out[d + "_score"][:, :V] - P.gather(1, idx[:, :V])).abs().max()) <= TOL
        m = rerank_metrics(out[d + "_idx"], out[d + "_score"], out[d + "_sim"], torch.arange(V))
        assert m["outside"] == 0 and m["r5"] == 100.0 and 1 <= m["medianR"] <= V


def test_rerank_retrieval_is_bitwise_repeatable(setup):
    a, b = _rerank(setup), _rerank(setup)
    for key in ("t2v_idx", "t2v_sim", "t2v_score", "v2t_idx", "v2t_sim", "v2t_score"):
        assert torch.equal(a[key], b[key]), key


if __name__ == "__main__":   # the child of test_score_pair_list_with_the_tail_on_every_row_in_a_child_process
    from tests.conftest import BERT_CFG
    assert os.environ.get("ALPRO_FUSION_TAIL_ROWS") == "0"
    model, data = _build(dict(BERT_CFG))
    np.save(sys.argv[1], _pair_probabilities(model, data))
