"""hip.attn_probs against the only way the library offered before it to see an attention map: softmax(q k^T) in torch on the same qkv.

    python tools/bench_attn_probs.py [--reps 7] [--warmup 3]

Shapes (batch, L, H = 12): the text pass (64 x 40), the fusion pass of the retrieval model (64 x 237), a long caption's fusion pass (16 x 517) and
the grounding window of the 237-token pass (40 text rows x 196 patch keys).  fp16 operands (the benchmark dtype) and fp32.  Each number is the
median over `reps` windows of the wall time of a window of calls that ends in a device synchronise (enough calls for ~50 ms); the two sides are
alternated.  The torch side reads the same qkv buffer: q / k views per head, matmul in the operand dtype, then in fp32
the scale, the key bias and the softmax.  Recorded, never gated: profiles/attn_probs.txt.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SHAPES = ((64, 40, None), (64, 237, None), (16, 517, None), (64, 237, ((0, 40), (41, 237))))   # (batch, L, window)
H = 12


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_probs measures on the GPU"
    from alpro_amd import hip
    print("# bench_attn_probs on %s" % torch.cuda.get_device_name())
    print("# hip.attn_probs vs torch softmax(q k^T / 8 + bias) on the same qkv, H = 12, median of %d windows" % args.reps)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for dt in (torch.float16, torch.float32):
        for batch, L, win in SHAPES:
            qkv = torch.randn(batch * L, 3 * H * 64, device="cuda", generator=gen).to(dt)
            kb = torch.zeros(batch, L, device="cuda")
            kb[::3, L - L // 5:] = -10000.0
            _, lse = hip.attn(qkv, batch, L, H, 0.125, kb, want_lse=True)
            (qa, qb), (ka, kb_) = win if win is not None else ((0, L), (0, L))

            def ours():
                return hip.attn_probs(qkv, lse, batch, L, H, 0.125, kb, q_range=(qa, qb), k_range=(ka, kb_))

            def base():
                x = qkv.view(batch, L, 3, H, 64)
                q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 3, 1)
                s = torch.matmul(q, k).float() * 0.125 + kb[:, None, None, :]
                return torch.softmax(s, dim=-1)[:, :, qa:qb, ka:kb_]     # (the window of a torch map still costs the whole map)

            for _ in range(args.warmup):
                ours()
                base()
            n = max(1, int(0.05 / max(window(ours, 2), window(base, 2))))
            to, tb = [], []
            for _ in range(args.reps):
                to.append(window(ours, n))
                tb.append(window(base, n))
            err = float((ours() - base()).abs().max())
            mo, mb = statistics.median(to), statistics.median(tb)
            out_bytes = batch * H * (qb - qa) * (kb_ - ka) * 4
            print("%s batch=%d L=%d window=%s: attn_probs %.3f ms (min %.3f, max %.3f; %.0f GB/s of output) | torch %.3f ms (min %.3f, max %.3f) | speedup %.2fx | "
                  "output %.1f MB | max |ours - torch| %.2e | %d calls per window"
                  % (str(dt).split(".")[-1], batch, L, "full" if win is None else "q[%d:%d] k[%d:%d]" % (qa, qb, ka, kb_), mo * 1e3, min(to) * 1e3, max(to) * 1e3,
                     out_bytes / mo / 1e9, mb * 1e3, min(tb) * 1e3, max(tb) * 1e3, mb / mo, out_bytes / 1e6, err, n), flush=True)
            del qkv, lse


if __name__ == "__main__":
    main()
