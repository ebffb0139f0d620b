"""Stage 1 and the whole two-stage retrieval search against what the library offered before them.

    python tools/bench_sim_topk.py [--reps 7] [--warmup 3] [--rerank-n 1000] [--k 16] [--frames 2] [--skip-all-pairs] [--all-pairs-max-s S] [--sweep]

Part 1: hip.sim_topk against torch.matmul + torch.topk on the materialised (nq, ng) matrix, same device, same process, fp32 unit-norm
features, at (nq, ng, k) = (1000, 1000, 16), (1000, 100000, 16) and (1, 1000000, 128).  Each number is the median over `reps` windows of the
wall time of a window of calls that ends in a device synchronise (the window holds enough calls for ~50 ms); the two are alternated.  The
candidate sets are compared as well (they may differ where two similarities are closer than fp32 rounding).
Part 2: rerank_retrieval (k candidates per query in both directions, fusion + ITM on their union) against the all-pairs fusion loop of
score_all_pairs on the SAME cached features, n videos x n captions, fp16 operands (the benchmark dtype), AlproForVideoTextRetrieval with
closed-form weights, `frames` frames x 224^2, 40-token captions.  The all-pairs loop runs n^2 / 512 fusion mini-batches: it is timed once.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SHAPES = ((1000, 1000, 16), (1000, 100000, 16), (1, 1000000, 128))


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


def part1(args):
    from alpro_amd import hip
    scale = 1.0 / 0.07
    print("# part 1: hip.sim_topk vs torch.matmul + torch.topk (fp32, d = 256, scale = 1 / 0.07), median of %d windows" % args.reps)
    for nq, ng, k in SHAPES:
        q, g = unit_rows(nq, 1), unit_rows(ng, 2)

        def ours():
            return hip.sim_topk(q, g, k, scale=scale)

        def base():
            return torch.topk((q @ g.t()) * scale, k, dim=1)

        for _ in range(args.warmup):
            ours()
            base()
        n = max(1, int(0.05 / max(window(ours, 2), window(base, 2))))
        to, tb = [], []
        for _ in range(args.reps):
            to.append(window(ours, n))
            tb.append(window(base, n))
        (v, i), (bv, bi) = ours(), base()
        same = float((i.long().sort(1)[0] == bi.sort(1)[0]).float().mean())
        mo, mb = statistics.median(to), statistics.median(tb)
        flop, byts = 2.0 * nq * ng * 256, 4.0 * 256 * (nq + ng)
        print("nq=%d ng=%d k=%d: sim_topk %.3f ms (min %.3f, max %.3f; %.1f TFLOP/s, %.0f GB/s of inputs) | matmul+topk %.3f ms (min %.3f, max %.3f) | "
              "speedup %.2fx | matrix avoided %.1f MB | candidate sets equal %.4f, max |val - baseline| %.2e | %d calls per window"
              % (nq, ng, k, mo * 1e3, min(to) * 1e3, max(to) * 1e3, flop / mo / 1e12, byts / mo / 1e9, mb * 1e3, min(tb) * 1e3, max(tb) * 1e3, mb / mo,
                 nq * ng * 4 / 1e6, same, float((v - bv).abs().max()), n))
        del q, g


def sweep(args):
    """hip.sim_topk alone against k and chunk (chunk 0 = the library's choice): what a round of selection and what a partial pass costs."""
    from alpro_amd import hip
    print("# sweep: hip.sim_topk against k and chunk, medians of 5 windows of ~30 ms")
    for nq, ng, ks, chunks in ((1000, 100000, (1, 16, 64, 128), (0, 128, 256, 2048, 8192)), (1, 1000000, (1, 16, 128), (0, 2048, 8192, 32768)),
                               (1000, 1000, (1, 16), (0, 256, 512))):
        q, g = unit_rows(nq, 1), unit_rows(ng, 2)
        for k in ks:
            for ch in chunks:
                def f():
                    return hip.sim_topk(q, g, k, chunk=ch)
                for _ in range(args.warmup):
                    f()
                n = max(1, int(0.03 / window(f, 2)))
                print("nq=%d ng=%d k=%d chunk=%d: %.3f ms" % (nq, ng, k, ch, statistics.median(window(f, n) for _ in range(5)) * 1e3), flush=True)
        del q, g


def part2(args):
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import AlproForVideoTextRetrieval, _linear32
    from alpro_amd.retrieval_eval import encode_captions, encode_gallery, rerank_retrieval
    from tests.conftest import BERT_CFG
    from tests.golden.det_init import fill_state_dict_
    from tests.test_host_cpu import VENC, make_cfg
    n, k, T = args.rerank_n, args.k, args.frames
    m = AlproForVideoTextRetrieval(make_cfg(BERT_CFG), dict(VENC, num_frm=T))
    fill_state_dict_(m)
    m.eval().cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    ids = torch.randint(1000, 30000, (n, 40), device="cuda", generator=gen)
    ids[:, 0] = 101
    mask = torch.ones((n, 40), dtype=torch.long, device="cuda")
    mask[::3, 31:] = 0
    print("# part 2: %d videos x %d captions, k = %d, %d frames x 224^2, 40-token captions, fp16 operands, closed-form weights" % (n, n, k, T))
    with rt.use_compute_dtype("fp16"), torch.no_grad():
        t0 = time.perf_counter()
        ve, vf = [], []
        for s in range(0, n, 50):   # the clips are generated as they are encoded: the gallery never sits in memory as pixels
            e, f = encode_gallery(m, torch.randn(min(50, n - s), T, 3, 224, 224, device="cuda", generator=gen))
            ve.append(e)
            vf.append(f)
        ve, vf = torch.cat(ve), torch.cat(vf)
        te, tf = encode_captions(m, ids, mask)
        torch.cuda.synchronize()
        print("encoding every video and caption once: %.2f s" % (time.perf_counter() - t0))

        def rerank():
            return rerank_retrieval(m, ve, vf, te, tf, mask, k)

        out = rerank()
        tr = [window(rerank, 1) for _ in range(3)]
        pairs = int(torch.unique(torch.cat([(out["t2v_idx"].long() * n + torch.arange(n, device="cuda")[:, None]).reshape(-1),
                                             (torch.arange(n, device="cuda")[:, None] * n + out["v2t_idx"].long()).reshape(-1)])).numel())
        print("rerank_retrieval: median %.3f s (runs: %s), %d fusion passes (%.2f %% of %d)" % (statistics.median(tr), ", ".join("%.3f" % x for x in tr), pairs,
                                                                                                100.0 * pairs / (n * n), n * n))
        if args.skip_all_pairs:
            print("all-pairs loop: not measured (--skip-all-pairs)")
            return

        # score_all_pairs' pair loop (alpro_amd/retrieval_eval.py) on the cached features; the mini-batches are all alike, so when the loop would
        # outlast --all-pairs-max-s it stops at a synchronised checkpoint and the total is EXTRAPOLATED from the mini-batches it ran (said so below)
        pair_bsz, nb = 512, (n * n + 511) // 512
        score = torch.full((n * n,), float("nan"), dtype=torch.float32, device="cuda")
        ones = torch.ones(ve.shape[:2], dtype=mask.dtype, device="cuda")
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        for b in range(nb):
            idx = torch.arange(b * pair_bsz, min(n * n, (b + 1) * pair_bsz), device="cuda")
            vi, ci = idx // n, idx % n
            o = m._fusion(torch.cat([te[ci], ve[vi]], dim=1), torch.cat([mask[ci], ones[vi]], dim=1))
            score[b * pair_bsz:b * pair_bsz + idx.numel()] = torch.softmax(_linear32(o[:, 0, :], m.itm_head).float(), dim=1)[:, 1]
            done = b + 1
            if done % 25 == 0:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 > args.all_pairs_max_s:
                    break
        torch.cuda.synchronize()
        ta = time.perf_counter() - t0
        if done == nb:
            print("all-pairs loop (score_all_pairs on the cached features): %.2f s for %d fusion passes, one run | rerank speedup %.1fx" % (ta, n * n, ta / statistics.median(tr)))
        else:
            est = ta / done * nb
            print("all-pairs loop (score_all_pairs on the cached features): %.2f s for the first %d of %d mini-batches of 512 pairs (%.1f ms each), stopped there; "
                  "EXTRAPOLATED to all %d fusion passes: %.1f s | rerank speedup (extrapolated) %.1fx" % (ta, done, nb, ta / done * 1e3, n * n, est, est / statistics.median(tr)))
        got, want = out["v2t_score"].reshape(-1), score.view(n, n).gather(1, out["v2t_idx"].long()).reshape(-1)
        have = ~torch.isnan(want)
        print("candidate scores vs the all-pairs matrix (%d candidates inside the part that ran): max err %.2e" % (int(have.sum()), float((got - want)[have].abs().max()) if bool(have.any()) else float("nan")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rerank-n", type=int, default=1000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--skip-all-pairs", action="store_true")
    ap.add_argument("--skip-rerank", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="only the sweep of hip.sim_topk over k and chunk")
    ap.add_argument("--all-pairs-max-s", type=float, default=1e9, help="stop the all-pairs loop after this many seconds and extrapolate (default: run it all)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sim_topk measures on the GPU"
    print("# bench_sim_topk on %s" % torch.cuda.get_device_name())
    if args.sweep:
        return sweep(args)
    part1(args)
    if not args.skip_rerank:
        part2(args)


if __name__ == "__main__":
    main()
