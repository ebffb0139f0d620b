"""The visual encoder's attention-map output: hip.attn_temporal_probs against softmax(q k^T) in torch on the same qkv, and what asking
TimeSformer.forward_features for the maps and hidden states costs.

    python tools/bench_vit_attn_maps.py [--reps 7] [--warmup 3] > profiles/vit_attn_maps.txt

Kernel: groups = B*N = 8 x 196 and 64 x 196, T in {4, 8, 16}, H = 12, fp16 operands (the benchmark dtype) and fp32; the torch side reads the same
qkv buffer (q / k views per head, matmul in the operand dtype, then scale and softmax in fp32).  Encoder: ViT-B/16 at 224 px, B = 8 clips of 8
frames, fp16, eval mode: forward_features without flags, with the window frame_patch_attention asks for (last block only, (CLS query) x (patch
keys)), and with both flags (all 12 blocks: 1.4 GB of spatial maps).  Each number is the median over `reps` windows of the wall time of a window of
calls that ends in a device synchronise; the sides are alternated.  Recorded, never gated.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

GROUPS = (8 * 196, 64 * 196)
FRAMES = (4, 8, 16)
H = 12


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(fns, reps, warmup, budget=0.05):
    for _ in range(warmup):
        for f in fns:
            f()
    n = max(1, int(budget / max(window(f, 2) for f in fns)))
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(times, fns):
            t.append(window(f, n))
    return times, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vit_attn_maps measures on the GPU"
    from alpro_amd import config as rt, hip
    print("# bench_vit_attn_maps on %s" % torch.cuda.get_device_name())
    print("# hip.attn_temporal_probs vs torch softmax(q k^T / 8) on the same qkv, H = 12, median of %d windows" % args.reps)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for dt in (torch.float16, torch.float32):
        for groups in GROUPS:
            for T in FRAMES:
                rows = groups * T
                qkv = torch.randn(rows, 3 * H * 64, device="cuda", generator=gen).to(dt)
                _, lse = hip.attn_temporal(qkv, T, H, 0.125, want_lse=True)

                def ours():
                    return hip.attn_temporal_probs(qkv, lse, T, H, 0.125)

                def base():
                    x = qkv.view(groups, T, 3, H, 64)
                    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 3, 1)
                    return torch.softmax(torch.matmul(q, k).float() * 0.125, dim=-1)

                (to, tb), n = alternate((ours, base), args.reps, args.warmup)
                err = float((ours() - base()).abs().max())
                mo, mb = statistics.median(to), statistics.median(tb)
                out_bytes, in_bytes = groups * H * T * T * 4, rows * 2 * H * 64 * qkv.element_size()
                print("%s groups=%d T=%d: attn_temporal_probs %.3f ms (min %.3f, max %.3f; %.0f GB/s read + written) | torch %.3f ms (min %.3f, max %.3f) | "
                      "speedup %.2fx | output %.1f MB | max |ours - torch| %.2e | %d calls per window"
                      % (str(dt).split(".")[-1], groups, T, mo * 1e3, min(to) * 1e3, max(to) * 1e3, (out_bytes + in_bytes) / mo / 1e9, mb * 1e3, min(tb) * 1e3,
                         max(tb) * 1e3, mb / mo, out_bytes / 1e6, err, n), flush=True)
                del qkv, lse

    from alpro_amd.modeling.timesformer.vit import TimeSformer
    B, T, N = 8, 8, 196
    cfg = {"cls": "TimeSformer", "patch_size": 16, "attn_drop_rate": 0, "drop_rate": 0, "drop_path_rate": 0.1, "maxpool_kernel_size": 2,
           "use_maxpooling": False, "gradient_checkpointing": False, "img_size": 224, "num_frm": T}
    torch.manual_seed(0)
    enc = TimeSformer(cfg, input_format="RGB").eval().cuda()
    x = torch.randn(B, 3, T, 224, 224, device="cuda", generator=gen)
    print("# TimeSformer.forward_features, B = %d clips x %d frames x 224 px, fp16, eval mode, median of %d windows" % (B, T, args.reps))
    with rt.use_compute_dtype("fp16"), torch.no_grad():
        def plain():
            return enc.forward_features(x)

        def helper():
            return enc.forward_features(x, output_attentions=True, attn_layers=(-1,), attn_window=((0, 1), (1, 1 + N)))

        def both():
            return enc.forward_features(x, output_attentions=True, output_hidden_states=True)

        (tp, th, tb), n = alternate((plain, helper, both), args.reps, args.warmup, budget=0.2)
        same = torch.equal(plain(), both().features) and torch.equal(plain(), helper().features)
    o = both()
    extra = sum(t.numel() * 4 for t in o.hidden_states + o.spatial_attentions + o.temporal_attentions)
    for name, t in (("no flags", tp), ("frame_patch_attention's window, last block", th), ("both flags, all 12 blocks", tb)):
        print("%-44s %.3f ms (min %.3f, max %.3f)" % (name + ":", statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3))
    print("both flags return %.2f GB of maps and hidden states; features bitwise equal in all three: %s; %d calls per window" % (extra / 1e9, same, n), flush=True)


if __name__ == "__main__":
    main()
