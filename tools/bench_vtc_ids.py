"""The contrastive loss with video ids against the plain one and against a soft-target restatement in torch.

    python tools/bench_vtc_ids.py [--reps 7] [--warmup 3]

Forward + backward (d temp included) of hip.vtc_loss_ids_fwd / _bwd, of hip.vtc_loss_fwd / _bwd on the same features, and of the soft-target
cross entropy ALBEF and BLIP write in torch (sim_targets = match / match.sum(1), -sum(log_softmax(sim) * sim_targets), autograd backward), at
(B, G, E) = (64, 512, 256) -- the workload's shape on the last of eight ranks -- and (64, 64, 256) -- one rank -- with 0 %, 5 % and 100 % of the
pairs sharing their video with another pair.  fp32 unit-norm features, temp = 0.07, same device, same process.  Each number is the median over
`reps` windows of the wall time of a window of calls that ends in a device synchronise (the window holds enough calls for ~50 ms); the three
are alternated.  The ids loss is compared with the torch restatement as well.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SHAPES = ((64, 512, 256), (64, 64, 256))
DUPLICATES = (0.0, 0.05, 1.0)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def make_ids(G, frac, seed):
    """G gathered ids of which round(frac * G) (an even number, at least 2 when frac > 0) share theirs with one other pair; frac = 1: one video."""
    gids = 1000 + torch.arange(G, dtype=torch.int64)
    if frac >= 1.0:
        gids[:] = 7
    elif frac > 0:
        n = max(2, int(round(frac * G)) // 2 * 2)
        pick = torch.randperm(G, generator=torch.Generator().manual_seed(seed))[:n]
        gids[pick[1::2]] = gids[pick[0::2]]
    return gids


def torch_soft_target(v, t, gv, gt, temp, ids, gids, col0):
    B = v.shape[0]
    tc = temp.clamp(0.001, 0.5)
    sim_v2t, sim_t2v = v @ gt.t() / tc, t @ gv.t() / tc
    match = (gids[None, :] == ids[:, None]) & (ids[:, None] >= 0)
    match[torch.arange(B, device=v.device), col0 + torch.arange(B, device=v.device)] = True
    target = match.float() / match.sum(1, keepdim=True)
    lv = -(torch.log_softmax(sim_v2t, 1) * target).sum(1).mean()
    lt = -(torch.log_softmax(sim_t2v, 1) * target).sum(1).mean()
    return (lv + lt) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vtc_ids measures on the GPU"
    from alpro_amd import hip
    hip.load()
    res = dict(tool="bench_vtc_ids", device=torch.cuda.get_device_name(), reps=args.reps, unit="us per forward + backward, median of the windows", cases=[])
    dloss = torch.ones((), device="cuda")
    for B, G, E in SHAPES:
        col0 = G - B
        g = torch.Generator(device="cuda").manual_seed(B + G)
        gv, gt = (torch.nn.functional.normalize(torch.randn(G, E, device="cuda", generator=g), dim=1).contiguous() for _ in range(2))
        v, t = gv[col0:col0 + B].clone(), gt[col0:col0 + B].clone()
        temp = torch.full((1,), 0.07, device="cuda")
        for frac in DUPLICATES:
            gids = make_ids(G, frac, seed=G).cuda()
            ids = gids[col0:col0 + B].clone()

            def with_ids():
                loss, s1, s2, lse = hip.vtc_loss_ids_fwd(v, t, gv, gt, temp, ids, gids, col0)
                return loss, hip.vtc_loss_ids_bwd(v, t, gv, gt, temp, ids, gids, col0, s1, s2, lse, dloss)

            def plain():
                loss, s1, s2, lse = hip.vtc_loss_fwd(v, t, gv, gt, temp, col0)
                return loss, hip.vtc_loss_bwd(v, t, gv, gt, temp, col0, s1, s2, lse, dloss)

            def soft():
                leaves = [x.detach().requires_grad_(True) for x in (v, t, gv, gt, temp)]
                loss = torch_soft_target(*leaves, ids, gids, col0)
                return loss, torch.autograd.grad(loss, leaves)

            fns = (with_ids, plain, soft)
            for _ in range(args.warmup):
                for f in fns:
                    f()
            n = max(1, int(0.05 / max(window(f, 2) for f in fns)))
            times = [[] for _ in fns]
            for _ in range(args.reps):
                for k, f in enumerate(fns):
                    times[k].append(window(f, n))
            (li, gi), (lp, _), (ls, gs) = with_ids(), plain(), soft()
            us = lambda x: round(statistics.median(x) * 1e6, 2)  # noqa: E731
            res["cases"].append(dict(
                B=B, G=G, E=E, col0=col0, duplicate_fraction=frac, rows_with_more_than_one_positive=int(((gids[None, :] == ids[:, None]).sum(1) > 1).sum()),
                ids_us=us(times[0]), ids_us_min=round(min(times[0]) * 1e6, 2), ids_us_max=round(max(times[0]) * 1e6, 2),
                plain_us=us(times[1]), plain_us_min=round(min(times[1]) * 1e6, 2), plain_us_max=round(max(times[1]) * 1e6, 2),
                torch_soft_target_us=us(times[2]), calls_per_window=n,
                ids_over_plain=round(statistics.median(times[0]) / statistics.median(times[1]), 3),
                torch_over_ids=round(statistics.median(times[2]) / statistics.median(times[0]), 2),
                loss_ids=float(li), loss_plain=float(lp), loss_torch_soft_target=float(ls),
                max_abs_dv_vs_torch=float((gi[0] - gs[0]).abs().max()), max_abs_dgt_vs_torch=float((gi[3] - gs[3]).abs().max())))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
