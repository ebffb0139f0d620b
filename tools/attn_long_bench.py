"""Micro-benchmark of full attention across the L = 256 seam: the whole-row kernels at L = 256 and the key-blocked kernels of
attention_long.hip at L = 257, 293, 517, 709 (192 sequences x 12 heads, head_dim 64, bf16 and fp16, key bias on, no dropout).

    python tools/attn_long_bench.py [--batch 192] [--iters 20] [--warmup 5]

Times come from HIP events around `iters` back-to-back calls after `warmup` calls of the same shape.  TF/s counts algorithmic FLOPs
(forward 4*B*H*L^2*64, backward 10*B*H*L^2*64: no padding, no recomputation); "peak" is the share of the 2.5 PF/s dense 16-bit MFMA rate.
torch.nn.functional.scaled_dot_product_attention at the same shapes is printed as a yardstick only (its backward through autograd)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from alpro_amd import hip  # noqa: E402

PEAK_16 = 2.5e15
H = 12


def timeit(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lengths", default="256,257,293,517,709")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attn_long_bench needs a GPU"
    hip.load()
    B = a.batch
    print("attention across the L = 256 seam: B=%d H=%d head_dim 64, key bias on, no dropout; %s" % (B, H, torch.cuda.get_device_name()))
    print("%-5s %-4s %-10s %10s %8s %7s   %10s %8s" % ("dtype", "L", "kernel", "fwd us", "TF/s", "peak", "bwd us", "TF/s"))
    g = torch.Generator(device="cuda").manual_seed(0)
    for dt, name in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        base = {}
        for L in (int(x) for x in a.lengths.split(",")):
            qkv = (torch.randn(B * L, 3 * H * 64, device="cuda", generator=g) * 0.7).to(dt)
            dout = torch.randn(B * L, H * 64, device="cuda", generator=g).to(dt)
            kb = torch.zeros(B, L, device="cuda")
            kb[:, L - L // 8:] = -10000.0
            out, lse = hip.attn(qkv, B, L, H, 0.125, kb, want_lse=True)
            tf = timeit(lambda: hip.attn(qkv, B, L, H, 0.125, kb, want_lse=True), a.iters, a.warmup)
            tb = timeit(lambda: hip.attn_bwd(qkv, out, dout, lse, B, L, H, 0.125, kb), a.iters, a.warmup)
            ff, fb = 4.0 * B * H * L * L * 64, 10.0 * B * H * L * L * 64
            kind = "whole-row" if L <= 256 else "long"
            rel = ""
            if L == 256:
                base = dict(f=tf, b=tb)
            elif base:
                rel = "   vs L=256: fwd %.2fx  bwd %.2fx" % (tf / base["f"], tb / base["b"])
            print("%-5s %-4d %-10s %10.1f %8.1f %6.1f%%   %10.1f %8.1f%s" % (name, L, kind, tf, ff / tf / 1e6, 100 * ff / tf / 1e6 / (PEAK_16 / 1e12), tb,
                                                                       fb / tb / 1e6, rel))
            # yardstick: torch SDPA on (B, H, L, 64) views of the same operands, with the same additive bias
            q, k, v = qkv.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
            q, k, v = q.contiguous().requires_grad_(True), k.contiguous().requires_grad_(True), v.contiguous().requires_grad_(True)
            mask = kb.to(dt)[:, None, None, :]
            sd = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=0.125)  # noqa: E731
            with torch.no_grad():
                ts = timeit(sd, a.iters, a.warmup)
            o = sd()
            do = dout.view(B, L, H, 64).transpose(1, 2)
            tsb = timeit(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True), a.iters, a.warmup)
            print("%-5s %-4d %-10s %10.1f %8.1f %6.1f%%   %10.1f %8.1f" % (name, L, "torch sdpa", ts, ff / ts / 1e6, 100 * ff / ts / 1e6 / (PEAK_16 / 1e12), tsb,
                                                                      fb / tsb / 1e6))
            del q, k, v, o


if __name__ == "__main__":
    main()
