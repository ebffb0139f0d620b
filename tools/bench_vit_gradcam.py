"""Grad-CAM of the visual encoder: hip.attn_temporal_probs_grad against the torch formulation of the same two maps on the same buffers, and the
two grounding helpers end to end beside pixel_gradient.

    python tools/bench_vit_gradcam.py [--reps 7] [--warmup 3] [--out profiles/vit_gradcam.txt]

1. hip.attn_temporal_probs_grad at B*N = 8 x 196 and 64 x 196 patch positions, T = 4 / 8 / 16 frames, H = 12, fp16 operands (the benchmark dtype)
   and fp32, with both outputs ("grad", "cam") and with the Grad-CAM map alone ("cam", what grounding.patch_temporal_gradcam asks for), against
   torch on the same qkv / dctx buffers: q / k / v and dctx views per head, both matmuls in the operand dtype, then in fp32 the scale, the
   softmax, the ReLU and the product.
2. grounding.frame_patch_gradcam, patch_temporal_gradcam and pixel_gradient on AlproForVideoTextRetrieval in eval mode, B = 8 pairs x 8 frames x
   224 px, fp16 operands (grad_scale 2^16), last block (the default) and all 12 blocks.
Each number is the median over `reps` windows of the wall time of a window of calls that ends in a device synchronise (enough calls for ~50 ms);
the sides are alternated.  Recorded, never gated.  The lines are printed and, with --out, also written to that file.
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


def alternate(fns, reps, warmup):
    """-> (per fn: list of window means, calls per window)"""
    for _ in range(warmup):
        for f in fns:
            f()
    n = max(1, int(0.05 / max(window(f, 2) for f in fns)))
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(window(f, n))
    return ts, n


def fmt(t):
    return "%.3f ms (min %.3f, max %.3f)" % (statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vit_gradcam measures on the GPU"
    from alpro_amd import config as rt, hip
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# bench_vit_gradcam on %s, median of %d windows of ~50 ms, sides alternated" % (torch.cuda.get_device_name(), args.reps))
    say("# 1. hip.attn_temporal_probs_grad vs torch softmax(q k^T / 8), dctx v^T, P * relu(G) on the same buffers, H = 12")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for dt in (torch.float16, torch.float32):
        for groups in GROUPS:
            for T in FRAMES:
                rows = groups * T
                qkv = torch.randn(rows, 3 * H * 64, device="cuda", generator=gen).to(dt)
                dctx = torch.randn(rows, H * 64, device="cuda", generator=gen).to(dt)
                _, lse = hip.attn_temporal(qkv, T, H, 0.125, want_lse=True)

                def both():
                    return hip.attn_temporal_probs_grad(qkv, dctx, lse, T, H, 0.125, want=("grad", "cam"))

                def cam_only():
                    return hip.attn_temporal_probs_grad(qkv, dctx, lse, T, H, 0.125, want=("cam",))

                def base():
                    x = qkv.view(groups, T, 3, H, 64)
                    q, k, v = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 3, 1), x[:, :, 2].permute(0, 2, 3, 1)
                    p = torch.softmax(torch.matmul(q, k).float() * 0.125, dim=-1)
                    g = torch.matmul(dctx.view(groups, T, H, 64).permute(0, 2, 1, 3), v).float()
                    return g, p * g.clamp(min=0)

                (t2, t1, tb), n = alternate((both, cam_only, base), args.reps, args.warmup)
                (g_o, c_o), (g_b, c_b) = both(), base()
                eg, ec = float((g_o - g_b).abs().max()), float((c_o - c_b).abs().max())
                m2, m1, mb = (statistics.median(t) for t in (t2, t1, tb))
                out_bytes = groups * H * T * T * 4
                in_bytes = rows * H * 64 * qkv.element_size()     # one third of qkv, or dctx
                say("%s groups=%d T=%d: grad+cam %s = %.0f GB/s (4 operand thirds + 2 maps) | cam only %s | torch %s | speedup %.2fx (grad+cam), %.2fx (cam only) | "
                    "output %.1f MB per map | max |ours - torch| grad %.2e cam %.2e | %d calls per window"
                    % (str(dt).split(".")[-1], groups, T, fmt(t2), (4 * in_bytes + 2 * out_bytes) / m2 / 1e9, fmt(t1), fmt(tb), mb / m2, mb / m1, out_bytes / 1e6,
                       eg, ec, n))
                del qkv, dctx, lse, g_o, c_o, g_b, c_b
    if not args.skip_model:
        from alpro_amd.grounding import frame_patch_gradcam, patch_temporal_gradcam, pixel_gradient
        from alpro_amd.modeling.alpro_models import AlproForVideoTextRetrieval
        from bench import BERT_CFG, VENC, Cfg, synth_batch
        say("# 2. the grounding helpers end to end: AlproForVideoTextRetrieval, eval mode, B = 8 pairs x 8 frames x 224 px, fp16 operands (grad_scale 2^16)")
        with rt.use_compute_dtype("fp16"):
            cfg = Cfg(dict(BERT_CFG, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
            torch.manual_seed(0)
            m = AlproForVideoTextRetrieval(cfg, dict(VENC, num_frm=8)).cuda().eval()
            batch = synth_batch(8, 8, "cuda", seed=0, full=False)
            ids, mask, clips = batch["text_input_ids"], batch["text_input_mask"], batch["visual_inputs"]
            every = tuple(range(12))

            def fwd_only():
                with torch.no_grad():
                    return m._forward_visual_embeds(clips)

            fns = (lambda: frame_patch_gradcam(m, ids, mask, clips), lambda: patch_temporal_gradcam(m, ids, mask, clips),
                   lambda: frame_patch_gradcam(m, ids, mask, clips, layers=every), lambda: patch_temporal_gradcam(m, ids, mask, clips, layers=every),
                   lambda: pixel_gradient(m, ids, mask, clips), fwd_only)
            ts, n = alternate(fns, args.reps, args.warmup)
            shapes = [tuple(f().shape) for f in fns[:5]]
            for name, t, shp in zip(("frame_patch_gradcam, last block", "patch_temporal_gradcam, last block", "frame_patch_gradcam, all 12 blocks",
                                     "patch_temporal_gradcam, all 12 blocks", "pixel_gradient"), ts, shapes):
                say("%-40s %s -> %s" % (name, fmt(t), shp))
            say("%-40s %s | %d calls per window" % ("for scale: the visual encoder's forward", fmt(ts[5]), n))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
