"""GPU: what freezing parameters (requires_grad = False) takes off a training step, A/B/A/B on one box in one call.

    python tools/frozen_bench.py [--steps 6] [--warmup 2] [--rounds 2] [--ln-reps 30] [--skip-steps] [--out profiles/frozen_bench.txt]

1. Steps, fp16 operands + dynamic loss scaling, FlatAdamW over the parameters that are trainable in the configuration, train mode (drop-path 0.1,
   BERT dropout 0.1):
     pretrain  AlproForPretrain, B = 64 pairs x 8 frames x 224^2 + 40 tokens (bench.py's flagship step)
     finetune  AlproForVideoTextRetrieval, B = 8 x 8 frames (loss = itm + itc)
   each with nothing frozen | the ViT's embedding + first 6 blocks frozen | the ViT wholly frozen.  The configurations alternate
   (all, half, all, vit) `rounds` times on the same model; a number is the wall time of `steps` steps ending in a device synchronise, and every
   frozen configuration is compared with the all-trainable step of the SAME call (the all-trainable step appears twice per round: its spread
   is the noise floor).  Frozen configurations did not run natively before, so there is no earlier number for them.
2. The data-only LayerNorm backward (dgamma = dbeta = None) against the column-sum kernel + its reduce launch at the step's norm2 shape
   (B = 64: 100416 rows, fp16 dy, FRAME emit), HIP-event timings, alternated."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def set_config(model, name):
    vit = model.visual_encoder.model
    for p in model.parameters():
        p.requires_grad_(True)
    if hasattr(model, "prompter"):           # the frozen teacher stays frozen
        for p in model.prompter.parameters():
            p.requires_grad_(False)
    if name == "half":
        for p in list(vit.patch_embed.parameters()) + [vit.cls_token, vit.pos_embed, vit.time_embed] + [q for b in vit.blocks[:6] for q in b.parameters()]:
            p.requires_grad_(False)
    elif name == "vit":
        for p in model.visual_encoder.parameters():
            p.requires_grad_(False)
    for p in model.parameters():
        p.grad = None


def bench_steps(tag, model, batch, loss_of, args, lines):
    from alpro_amd.optim import FlatAdamW
    order = ["all", "half", "all", "vit"]
    res = {"all": [], "half": [], "vit": []}
    peak = {}
    for _ in range(args.rounds):
        for name in order:
            set_config(model, name)
            opt = FlatAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.0, max_grad_norm=20.0)

            def step():
                opt.backward(loss_of(model(batch)))
                opt.step()
                opt.zero_grad()
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            res[name].append(timed(step, args.steps))
            peak[name] = torch.cuda.max_memory_allocated() / 2 ** 30
            del opt
    base = statistics.median(res["all"])
    for name in ("all", "half", "vit"):
        v = res[name]
        lines.append("%-9s %-5s median %8.2f ms  (%s)  vs all-trainable %+6.1f %%  peak %.1f GiB" %
                     (tag, name, statistics.median(v) * 1e3, ", ".join("%.2f" % (x * 1e3) for x in v), (statistics.median(v) / base - 1.0) * 100.0, peak[name]))
        print(lines[-1], flush=True)


def bench_ln(args, lines):
    from alpro_amd import hip
    B, T, N, D = 64, 8, 196, 768
    S = 1 + N * T
    rows = B * S
    g = torch.Generator().manual_seed(1)
    x = torch.randn(rows, D, generator=g).cuda()
    dy = torch.randn(rows, D, generator=g).cuda().half()
    gamma = (1.0 + 0.1 * torch.randn(D, generator=g)).cuda()
    scale = torch.ones(B * T, device="cuda")
    dx = torch.zeros(rows, D, device="cuda")
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    emit = dict(mode=hip.EMIT_FRAME, rows=B * T * (N + 1), dtype=torch.float16, T=T, N=N, scale=scale)
    forms = {"column_sums+reduce": lambda: hip.layernorm_bwd(dy, x, gamma, 1e-6, dx, dg, db, emit=emit),
             "data_only": lambda: hip.layernorm_bwd(dy, x, gamma, 1e-6, dx, None, None, emit=emit)}
    times = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.ln_reps):
        for name in ("column_sums+reduce", "data_only"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            forms[name]()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    base = statistics.median(times["column_sums+reduce"])
    for name, t in times.items():
        t = sorted(t)
        lines.append("layernorm_bwd norm2 shape (%d rows, fp16, FRAME emit) %-20s median %.4f ms  (min %.4f, p90 %.4f)  vs column sums %+.1f %%" %
                     (rows, name, statistics.median(t), t[0], t[len(t) * 9 // 10], (statistics.median(t) / base - 1.0) * 100.0))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ln-reps", type=int, default=30)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frozen_bench measures on the GPU"
    from alpro_amd import config as rt
    from bench import BERT_CFG, VENC, Cfg, synth_batch
    lines = ["# frozen_bench: %s; fp16 operands + loss scaling, FlatAdamW, train mode; %d rounds of (all, half, all, vit) x %d steps" %
             (torch.cuda.get_device_name(0), args.rounds, args.steps)]
    print(lines[0], flush=True)
    with rt.use_compute_dtype("fp16"):
        bench_ln(args, lines)
        if not args.skip_steps:
            from alpro_amd.modeling.alpro_models import AlproForPretrain, AlproForVideoTextRetrieval
            cfg = Cfg(dict(BERT_CFG, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
            torch.manual_seed(0)
            m = AlproForPretrain(cfg, dict(VENC, num_frm=8)).cuda().train()
            bench_steps("pretrain", m, synth_batch(64, 8, "cuda", seed=0, full=True),
                        lambda o: o["mlm_loss"] + o["itm_loss"] + o["itc_loss"] + o["mpm_loss"], args, lines)
            del m
            torch.cuda.empty_cache()
            m = AlproForVideoTextRetrieval(cfg, dict(VENC, num_frm=8)).cuda().train()
            bench_steps("finetune", m, synth_batch(8, 8, "cuda", seed=0, full=False), lambda o: o["itm_loss"] + o["itc_loss"], args, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
