"""GPU: what recomputing the ViT blocks' activations in backward (ALPRO_RECOMPUTE) costs and saves, A/B/A/B on one box in one call.

    python tools/recompute_bench.py [--steps 6] [--warmup 2] [--rounds 2] [--max-batch 256] [--limit 300] [--out profiles/recompute_bench.txt]

The pretraining step of bench.py (AlproForPretrain, 8 frames x 224^2 + 40 tokens, fp16 operands + dynamic loss scaling, FlatAdamW, train mode:
drop-path 0.1, BERT dropout 0.1):
  1. B = 64 with the switch off and on, alternated `rounds` times (off, on, off, on, ...);
  2. with the switch on only, B doubled (128, 256, ...) until an allocation fails or --max-batch is through.
Every configuration is one child process of this script (`--one B FLAG`) under its own `timeout`: it builds the model, runs `warmup` steps, then times
`steps` steps ending in a device synchronise and reports the step time and the peak of allocated and reserved memory.  A failed allocation is a result
(the child says so and ends with status 0); any other non-zero status -- a time limit included -- ends the whole call there.  This process never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOSS = ("mlm_loss", "itm_loss", "itc_loss", "mpm_loss")


def one(B, flag, steps, warmup):
    import torch
    assert torch.cuda.is_available(), "recompute_bench measures on the GPU"
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import AlproForPretrain
    from alpro_amd.optim import FlatAdamW
    from bench import BERT_CFG, VENC, Cfg, synth_batch
    res = dict(B=B, recompute=int(flag), device=torch.cuda.get_device_name(0))
    try:
        with rt.use_compute_dtype("fp16"), rt.use_recompute(flag):
            torch.manual_seed(0)
            m = AlproForPretrain(Cfg(dict(BERT_CFG, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)), dict(VENC, num_frm=8)).cuda().train()
            batch = synth_batch(B, 8, "cuda", seed=0, full=True)
            opt = FlatAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.0, max_grad_norm=20.0)

            def step():
                out = m(batch)
                opt.backward(sum(out[k] for k in LOSS))
                opt.step()
                opt.zero_grad()
            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            res.update(ms=(time.perf_counter() - t0) / steps * 1e3, peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30,
                       reserved_gib=torch.cuda.max_memory_reserved() / 2 ** 30)
    except RuntimeError as e:   # (torch.cuda.OutOfMemoryError is one; out of a backward pass it may arrive as the plain class)
        if "out of memory" not in str(e).lower():
            raise
        res.update(oom=str(e).split("\n")[0][:160])
    print("RESULT " + json.dumps(res), flush=True)


def child(B, flag, args):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), str(int(flag)),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(got[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, type=int, metavar=("B", "FLAG"), default=None)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one configuration, seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one[0], bool(args.one[1]), args.steps, args.warmup)
    lines, runs = [], {0: [], 1: []}
    status = 0

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write("\n".join(lines) + "\n")

    plan = [(args.batch, f) for _ in range(args.rounds) for f in (False, True)]
    B = args.batch * 2
    while B <= args.max_batch:
        plan.append((B, True))
        B *= 2
    for B, flag in plan:
        status, r = child(B, flag, args)
        if status != 0:
            say("B = %-4d recompute %d: child ended with status %d -- stopped here" % (B, flag, status))
            break
        if not lines:
            say("# recompute_bench: %s; pretraining step, 8 frames x 224^2 + 40 tokens, fp16 operands + loss scaling, FlatAdamW, train mode; %d steps after %d "
                "warm-up steps per configuration, one process each" % (r["device"], args.steps, args.warmup))
        if "oom" in r:
            say("B = %-4d recompute %d: allocation failed (%s)" % (B, flag, r["oom"]))
            break
        say("B = %-4d recompute %d: step %8.2f ms  (%.3f ms per pair)  peak allocated %6.1f GiB  reserved %6.1f GiB" %
            (B, flag, r["ms"], r["ms"] / B, r["peak_gib"], r["reserved_gib"]))
        if B == args.batch:
            runs[int(flag)].append(r)
    if runs[0] and runs[1]:
        off, on = (statistics.median(x["ms"] for x in runs[k]) for k in (0, 1))
        say("B = %d: switch on against off %+.1f %% step time (off %s ms, on %s ms), peak allocated %.1f -> %.1f GiB" %
            (args.batch, (on / off - 1.0) * 100.0, ", ".join("%.2f" % x["ms"] for x in runs[0]), ", ".join("%.2f" % x["ms"] for x in runs[1]),
             runs[0][-1]["peak_gib"], runs[1][-1]["peak_gib"]))
    write()
    sys.exit(status)


if __name__ == "__main__":
    main()
