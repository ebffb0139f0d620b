"""The pixel gradient's cost: hip.unpatchify against F.fold and against hip.patchify, the retrieval model's backward with and without the input
gradient, and grounding.text_to_pixel_saliency end to end.

    python tools/bench_pixel_grad.py [--reps 7] [--warmup 3] [--out profiles/pixel_grad.txt]

1. hip.unpatchify at (512, 3, 224, 224) -- 64 clips of 8 frames -- from fp32 rows (what the model hands it: the fp32 output of drows @ W) and from
   fp16 rows, against F.fold on the same rows (torch wants them as (BT, C*256, N): the transposed view is part of its side) and against
   hip.patchify at the same shape, which moves the same bytes the other way.  GB/s counts the bytes read plus the bytes written.
2. AlproForVideoTextRetrieval, B = 8 pairs x 8 frames x 224 px, fp16 operands under a fixed loss scale, train mode: forward + backward of
   itm_loss + itc_loss with visual_inputs.requires_grad False and True (the difference is the patch embedding's data gradient: one gather_cast
   when the projection weight is frozen, one GEMM, one unpatchify, and the transpose's backward).
3. grounding.text_to_pixel_saliency(model.eval(), ...) on the same batch: text pass, visual pass, fusion pass, the data-only backward, the reduction.
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
import torch.nn.functional as F  # noqa: E402

SHAPE = (512, 3, 224, 224)


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
    assert torch.cuda.is_available(), "bench_pixel_grad measures on the GPU"
    from alpro_amd import config as rt, hip
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# bench_pixel_grad on %s, median of %d windows of ~50 ms, sides alternated" % (torch.cuda.get_device_name(), args.reps))
    BT, C, H, W = SHAPE
    gen = torch.Generator(device="cuda").manual_seed(5)
    img = torch.randn(SHAPE, device="cuda", generator=gen)
    for dt in (torch.float32, torch.float16):
        rows = hip.patchify(img, dt)
        out = torch.empty(SHAPE, device="cuda")
        cols = rows.view(BT, -1, C * 256).transpose(1, 2)

        def ours():
            return hip.unpatchify(rows, BT, C, H, W, out=out)

        def fold():
            return F.fold(cols, (H, W), 16, stride=16)

        def fwd():
            return hip.patchify(img, dt)

        (tu, tf, tp), n = alternate((ours, fold, fwd), args.reps, args.warmup)
        same = torch.equal(ours(), fold().float())
        nbytes = img.numel() * (4 + rows.element_size())
        mu, mf, mp_ = (statistics.median(t) for t in (tu, tf, tp))
        say("unpatchify %s rows -> %s fp32: hip.unpatchify %s = %.0f GB/s | F.fold %s = %.0f GB/s (%.2fx) | hip.patchify fp32 -> %s %s = %.0f GB/s "
            "(unpatchify / patchify time %.2f) | %.1f MB moved | equal to F.fold: %s | %d calls per window"
            % (str(dt).split(".")[-1], SHAPE, fmt(tu), nbytes / mu / 1e9, fmt(tf), nbytes / mf / 1e9, mf / mu, str(dt).split(".")[-1], fmt(tp),
               nbytes / mp_ / 1e9, mu / mp_, nbytes / 1e6, same, n))
        del rows, out, cols
    del img
    if not args.skip_model:
        from alpro_amd import amp
        from alpro_amd.grounding import text_to_pixel_saliency
        from alpro_amd.modeling.alpro_models import AlproForVideoTextRetrieval
        from bench import BERT_CFG, VENC, Cfg, synth_batch
        with rt.use_compute_dtype("fp16"):
            cfg = Cfg(dict(BERT_CFG, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
            torch.manual_seed(0)
            m = AlproForVideoTextRetrieval(cfg, dict(VENC, num_frm=8)).cuda().train()
            batch = synth_batch(8, 8, "cuda", seed=0, full=False)
            sc = amp.LossScaler(init_scale=4096.0, dynamic=False, device="cuda")
            rt.set_armed_loss_scaler(sc)

            def step(x_grad):
                def f():
                    b = dict(batch, visual_inputs=batch["visual_inputs"].detach().requires_grad_(x_grad))
                    o = m(b)
                    with rt.loss_scaling(sc):
                        ((o["itm_loss"] + o["itc_loss"]) * sc.scale.reshape(())).backward()
                    return b["visual_inputs"].grad
                return f

            (t0, t1), n = alternate((step(False), step(True)), args.reps, args.warmup)
            g = step(True)()
            m0, m1 = statistics.median(t0), statistics.median(t1)
            say("retrieval model B=8 x 8 frames x 224 px, fp16, train mode, forward + backward: without the input gradient %s | with it %s | "
                "difference %.3f ms = %.2f %% | visual_inputs.grad %s contiguous=%s finite=%s | %d calls per window"
                % (fmt(t0), fmt(t1), (m1 - m0) * 1e3, 100.0 * (m1 - m0) / m0, tuple(g.shape), g.is_contiguous(), bool(torch.isfinite(g).all()), n))
            for p in m.parameters():
                p.grad = None
            rt.set_armed_loss_scaler(None)
            m.eval()

            def sal():
                return text_to_pixel_saliency(m, batch["text_input_ids"], batch["text_input_mask"], batch["visual_inputs"])

            def fwd_only():
                with torch.no_grad():
                    return m.forward_inference(dict(visual_inputs=batch["visual_inputs"][:1], text_input_ids=batch["text_input_ids"],
                                                    text_input_mask=batch["text_input_mask"]))

            (ts, tfw), n = alternate((sal, fwd_only), args.reps, args.warmup)
            s = sal()
            say("text_to_pixel_saliency B=8 x 8 frames x 224 px, fp16 (grad_scale 2^16), eval mode, end to end: %s -> %s | for scale, forward_inference of one "
                "video against the 8 captions: %s | %d calls per window" % (fmt(ts), tuple(s.shape), fmt(tfw), n))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
