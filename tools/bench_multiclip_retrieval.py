"""Stage 1 of the multi-clip two-stage retrieval search against its restatement in torch, and what stage 2 is left with.

    python tools/bench_multiclip_retrieval.py [--videos 4000] [--captions 4000] [--clips 4] [--k 16] [--mode mean] [--reps 7] [--warmup 3]

Stage 1 of rerank_retrieval(num_clips=n): hip.sim_topk_clips in both directions (text -> video with the clips on the gallery side, video -> text
with the clips on the query side) against the torch restatement -- the (V*n, C) similarity matrix, pooled over the clips (mean / amax /
logsumexp), then torch.topk along both axes -- on the same device, in the same process, on fp32 unit-norm features.  Each time is the median
over `reps` windows of the wall time of a window of calls that ends in a device synchronise (~50 ms of calls per window); the two sides
are alternated.  The candidate sets are compared as well (they may differ where two pooled values are closer than fp32 rounding).
Stage 2 is not run: the tool counts the fusion sequences it would score -- the union of the two candidate sets, n clips each -- against the
V * C * n sequences of the all-pairs evaluation.  Prints ONE JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

POOL = {"mean": lambda x: x.mean(1), "max": lambda x: x.amax(1), "lse": lambda x: torch.logsumexp(x, dim=1)}


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def unit_rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 256, device="cuda", generator=g), dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4000)
    ap.add_argument("--captions", type=int, default=4000)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--mode", default="mean", choices=sorted(POOL))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_multiclip_retrieval measures on the GPU"
    from alpro_amd import hip
    V, C, n, k, scale = args.videos, args.captions, args.clips, args.k, 1.0 / 0.07
    vf, tf = unit_rows(V * n, 1), unit_rows(C, 2)

    def ours():
        return hip.sim_topk_clips(tf, vf, k, n, side="gallery", mode=args.mode, scale=scale), hip.sim_topk_clips(vf, tf, k, n, side="query", mode=args.mode, scale=scale)

    def base():
        pooled = POOL[args.mode](((vf @ tf.t()) * scale).view(V, n, C))     # (V, C)
        return torch.topk(pooled.t(), k, dim=1), torch.topk(pooled, k, dim=1)

    for _ in range(args.warmup):
        ours()
        base()
    calls = max(1, int(0.05 / max(window(ours, 2), window(base, 2))))
    to, tb = [], []
    for _ in range(args.reps):
        to.append(window(ours, calls))
        tb.append(window(base, calls))
    ((t2v_val, t2v_idx), (v2t_val, v2t_idx)), ((bt_val, bt_idx), (bv_val, bv_idx)) = ours(), base()
    same = min(float((t2v_idx.long().sort(1)[0] == bt_idx.sort(1)[0]).float().mean()), float((v2t_idx.long().sort(1)[0] == bv_idx.sort(1)[0]).float().mean()))
    err = max(float((t2v_val - bt_val).abs().max()), float((v2t_val - bv_val).abs().max()))
    dev = vf.device
    pairs = torch.unique(torch.cat([(t2v_idx.long() * C + torch.arange(C, device=dev)[:, None]).reshape(-1),
                                    (torch.arange(V, device=dev)[:, None] * C + v2t_idx.long()).reshape(-1)])).numel()
    mo, mb = statistics.median(to), statistics.median(tb)
    print(json.dumps(dict(device=torch.cuda.get_device_name(), videos=V, captions=C, clips=n, k=k, mode=args.mode, reps=args.reps, calls_per_window=calls,
                          sim_topk_clips_ms=round(mo * 1e3, 4), sim_topk_clips_ms_min=round(min(to) * 1e3, 4), sim_topk_clips_ms_max=round(max(to) * 1e3, 4),
                          torch_ms=round(mb * 1e3, 4), torch_ms_min=round(min(tb) * 1e3, 4), torch_ms_max=round(max(tb) * 1e3, 4),
                          torch_over_ours=round(mb / mo, 3), matrix_avoided_mb=round(V * n * C * 4 / 1e6, 1),
                          candidate_sets_equal=round(same, 6), max_abs_val_diff=err,
                          fusion_sequences_two_stage=int(pairs) * n, fusion_sequences_all_pairs=V * C * n,
                          fusion_fraction=round(pairs / float(V * C), 6))))


if __name__ == "__main__":
    main()
