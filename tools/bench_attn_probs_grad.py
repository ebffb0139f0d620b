"""hip.attn_probs_grad against the torch formulation of the same two maps on the same buffers: softmax(q k^T / 8 + bias), dctx . v^T, multiply.

    python tools/bench_attn_probs_grad.py [--reps 7] [--warmup 3] [--out profiles/attn_probs_grad.txt]

Shapes (batch, L, H = 12): the text pass (64 x 40), the fusion pass of the retrieval model (64 x 237) and the grounding window of the 237-token
pass (40 text rows x 196 patch keys).  fp16 operands (the benchmark dtype) and fp32.  Per shape the kernel is timed with both outputs
("grad", "cam") and with the Grad-CAM map alone ("cam", what grounding.text_to_patch_gradcam asks for).  Each number is the median over `reps`
windows of the wall time of a window of calls that ends in a device synchronise (enough calls for ~50 ms); the sides are alternated.  The torch
side reads the same qkv / dctx buffers: q / k / v and dctx views per head, both matmuls in the operand dtype, then in fp32 the scale, the key
bias, the softmax, the ReLU and the product -- and, as torch has to, it forms the whole (L, L) maps before it slices the window.
Recorded, never gated.  The lines are printed and, with --out, also written to that file.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SHAPES = ((64, 40, None), (64, 237, None), (64, 237, ((0, 40), (41, 237))))   # (batch, L, window)
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attn_probs_grad measures on the GPU"
    from alpro_amd import hip
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# bench_attn_probs_grad on %s" % torch.cuda.get_device_name())
    say("# hip.attn_probs_grad vs torch softmax(q k^T / 8 + bias), dctx v^T, P * relu(G) on the same buffers, H = 12, median of %d windows" % args.reps)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for dt in (torch.float16, torch.float32):
        for batch, L, win in SHAPES:
            qkv = torch.randn(batch * L, 3 * H * 64, device="cuda", generator=gen).to(dt)
            dctx = torch.randn(batch * L, H * 64, device="cuda", generator=gen).to(dt)
            kb = torch.zeros(batch, L, device="cuda")
            kb[::3, L - L // 5:] = -10000.0
            _, lse = hip.attn(qkv, batch, L, H, 0.125, kb, want_lse=True)
            (qa, qb), (ka, kb_) = win if win is not None else ((0, L), (0, L))

            def both():
                return hip.attn_probs_grad(qkv, dctx, lse, batch, L, H, 0.125, kb, q_range=(qa, qb), k_range=(ka, kb_), want=("grad", "cam"))

            def cam_only():
                return hip.attn_probs_grad(qkv, dctx, lse, batch, L, H, 0.125, kb, q_range=(qa, qb), k_range=(ka, kb_), want=("cam",))

            def base():
                x = qkv.view(batch, L, 3, H, 64)
                q, k, v = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 3, 1), x[:, :, 2].permute(0, 2, 3, 1)
                p = torch.softmax(torch.matmul(q, k).float() * 0.125 + kb[:, None, None, :], dim=-1)
                g = torch.matmul(dctx.view(batch, L, H, 64).permute(0, 2, 1, 3), v).float()
                return g[:, :, qa:qb, ka:kb_], (p * g.clamp(min=0))[:, :, qa:qb, ka:kb_]

            for _ in range(args.warmup):
                both()
                cam_only()
                base()
            n = max(1, int(0.05 / max(window(both, 2), window(base, 2))))
            t2, t1, tb = [], [], []
            for _ in range(args.reps):
                t2.append(window(both, n))
                t1.append(window(cam_only, n))
                tb.append(window(base, n))
            (g_o, c_o), (g_b, c_b) = both(), base()
            eg, ec = float((g_o - g_b).abs().max()), float((c_o - c_b).abs().max())
            m2, m1, mb = statistics.median(t2), statistics.median(t1), statistics.median(tb)
            out_bytes = batch * H * (qb - qa) * (kb_ - ka) * 4
            say("%s batch=%d L=%d window=%s: grad+cam %.3f ms (min %.3f, max %.3f; %.0f GB/s of output) | cam only %.3f ms (min %.3f, max %.3f) | "
                "torch %.3f ms (min %.3f, max %.3f) | speedup %.2fx (grad+cam), %.2fx (cam only) | output %.1f MB per map | "
                "max |ours - torch| grad %.2e cam %.2e | %d calls per window"
                % (str(dt).split(".")[-1], batch, L, "full" if win is None else "q[%d:%d] k[%d:%d]" % (qa, qb, ka, kb_), m2 * 1e3, min(t2) * 1e3, max(t2) * 1e3,
                   2 * out_bytes / m2 / 1e9, m1 * 1e3, min(t1) * 1e3, max(t1) * 1e3, mb * 1e3, min(tb) * 1e3, max(tb) * 1e3, mb / m2, mb / m1,
                   out_bytes / 1e6, eg, ec, n))
            del qkv, dctx, lse
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
