"""Golden vectors for multi-clip retrieval evaluation (inference_n_clips > 1, score_agg_func), from the REFERENCE itself (CPU, fp32, eval).

    python -m tests.golden.make_golden_ret_clips          # writes tests/golden/retrieval_clips_T2_V4_C3.npz

4 videos x 3 clips x 2 frames against 5 captions on the retrieval_T2 closed-form model (det_init.py, as make_golden.case_retrieval_eval): the
12 clips and the captions come from det_batch(12, 2, seed_name=SEED_NAME), clip j of video v is row v * 3 + j, the captions are rows 0..4.
The reference's forward_inference runs once per clip against all captions, as its evaluation loop does (run_video_retrieval.py:663-675), and
gives the per-clip ITM logits and ITC scores.  That loop then squeezes the clip axis, which only works for one clip; the pooling stored here
is the rule of its video-QA loop (run_video_qa.py:269-279: mean / max / lse over the clip axis), written in plain torch fp64, as
make_golden_qa.case_qa_clips does.  Stored: clip_logits (12, 5, 2), clip_itc (12, 5); per mode the pooled logits (4, 5, 2), sims (4, 5) and
scores = softmax(pooled logits)[1] (4, 5) in fp64, the records' 4-decimal score / sim tables, and the metrics the reference's eval_retrieval
computes from those records (caption c belongs to video c % 4).

The generator asserts that the fixture can tell pooling from taking the first clip: for every mode, in each direction, at least one row's
top-2 by pooled sim differs (as a set) from its top-2 by clip 0 alone.  SEED_NAMES are tried in order until that holds; the one used is stored
as `seed_name` (the first four agree with clip 0 in some mode or direction; the one used is "retrieval_clips_T2_4").  Needs the reference; never runs on the GPU box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as mg  # noqa: E402
from tests.golden import ref_harness as rh  # noqa: E402
from tests.golden.det_init import det_batch, fill_state_dict_  # noqa: E402

T, V, N, C = 2, 4, 3, 5
SEED_NAMES = ["retrieval_clips_T2"] + ["retrieval_clips_T2_%d" % i for i in range(1, 8)]
FNAME = "retrieval_clips_T%d_V%d_C%d.npz" % (T, V, N)


def pool(x, mode):
    """x (V, N, ...) fp64 -> pooled over the clip axis (run_video_qa.py:269-279)"""
    return {"mean": lambda: x.mean(1), "max": lambda: x.amax(1), "lse": lambda: torch.logsumexp(x, dim=1)}[mode]()


def top2_sets(m):
    return [frozenset(r.tolist()) for r in torch.topk(m, 2, dim=1)[1]]


def tells_pooling_from_clip0(itc):
    """itc (V, N, C) fp64: for every mode and both directions some row's top-2 by pooled sim is not its top-2 by clip 0"""
    first = itc[:, 0]
    return all(top2_sets(d(pool(itc, mode))) != top2_sets(d(first)) for mode in ("mean", "max", "lse") for d in (lambda m: m, lambda m: m.t()))


def clip_outputs(m, seed_name):
    batch = det_batch(V * N, T, seed_name=seed_name, with_mlm=False, with_mpm=False)
    ids, mask = batch["text_input_ids"][:C], batch["text_input_mask"][:C]
    logits, itc = [], []
    with torch.no_grad():
        for r in range(V * N):   # the whole model once per clip against all captions, as the driver's loop does
            out = m.forward_inference(dict(visual_inputs=batch["visual_inputs"][r:r + 1], text_input_ids=ids, text_input_mask=mask))
            logits.append(out["logits"].float().reshape(C, 2))
            itc.append(out["itc_scores"].float().reshape(C))
    return torch.stack(logits), torch.stack(itc)       # (12, 5, 2), (12, 5)


def main():
    am, _ = rh.import_reference()
    torch.set_num_threads(8)
    cfg, venc = rh.make_configs(num_frm=T)
    m = am.AlproForVideoTextRetrieval(cfg, venc)
    fill_state_dict_(m)
    m.eval()
    for seed_name in SEED_NAMES:
        logits, itc = clip_outputs(m, seed_name)
        if tells_pooling_from_clip0(itc.double().view(V, N, C)):
            break
        print("seed_name %r: pooled and first-clip candidates agree somewhere, trying the next" % seed_name)
    else:
        raise SystemExit("no seed name gives a fixture that tells pooling from the first clip")
    g = {"seed_name": np.array(seed_name), "clip_logits": mg.npf(logits), "clip_itc": mg.npf(itc)}
    ns = mg.reference_eval_functions()
    gt = {"t%d" % c: "v%d" % (c % V) for c in range(C)}
    for mode in ("mean", "max", "lse"):
        pl = pool(logits.double().view(V, N, C, 2), mode)
        sim = pool(itc.double().view(V, N, C), mode)
        score = torch.softmax(pl, dim=-1)[..., 1]
        recs = [dict(vid_id="v%d" % v, txt_id="t%d" % c, score=round(float(score[v, c]), 4), sim=round(float(sim[v, c]), 4)) for v in range(V) for c in range(C)]
        g["pooled_logits/" + mode], g["sim/" + mode], g["score/" + mode] = pl.numpy(), sim.numpy(), score.numpy()
        g["rec_score/" + mode] = np.array([r["score"] for r in recs]).reshape(V, C)
        g["rec_sim/" + mode] = np.array([r["sim"] for r in recs]).reshape(V, C)
        metrics = ns["eval_retrieval"](recs, gt, None)
        for d in ("text2video", "video2text"):
            for k, val in metrics[d].items():
                g["%s/%s/%s" % (mode, d, k)] = np.float64(val)
    np.savez_compressed(os.path.join(HERE, FNAME), **g)
    print(FNAME, os.path.getsize(os.path.join(HERE, FNAME)), "seed_name", seed_name)


if __name__ == "__main__":
    main()
