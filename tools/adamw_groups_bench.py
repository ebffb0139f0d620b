"""GPU: the grouped optimizer pass (alpro_adamw_step_groups) against the one-group pass (alpro_adamw_step_lp) on the pretraining model's flat
size, fp16 mirror on, zero_grad folded in, clip on -- A/B/A/B in ONE process, HIP-event timings, medians and the A/A spread.

    python tools/adamw_groups_bench.py [--n 234190000] [--reps 40] [--out profiles/r10_adamw_groups.txt]

Bytes per parameter: 16 read + 12 written (+ 4 for the cleared gradient, + 2 for the mirror)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alpro_amd import hip  # noqa: E402


def segments(n, count):
    hp = dict(lr=1e-4, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.01, step_size=1.1e-4, correct_bias=True)
    ends = [(n * (k + 1) // count) // 4 * 4 + 4 * 37 for k in range(count - 1)] + [n]    # boundaries inside waves, not on 256-element marks
    return [dict(hp, end=e) for e in ends]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=234190000)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.n // 4 * 4
    p, m = torch.randn(n, device="cuda") * 0.03, torch.zeros(n, device="cuda")
    g, v = torch.randn(n, device="cuda") * 1e-3, torch.zeros(n, device="cuda")
    lp = torch.empty(n, dtype=torch.float16, device="cuda")
    norm = torch.zeros(1, device="cuda")
    hip.sumsq(g, norm)
    dyn = torch.tensor([1.0, 0.0, 5.0, 0.0], device="cuda")
    kw = dict(max_norm=20.0, grad_scale=1.0, dyn_state=dyn, grads_scaled=True, zero_grad=True, lp=lp)
    variants = {"one_group": lambda: hip.adamw_step(p, g, m, v, 1e-4, 0.9, 0.98, 1e-6, 0.01, 1.1e-4, norm, **kw)}
    for count in (1, 3, 16):
        variants["groups_%d" % count] = (lambda segs: (lambda: hip.adamw_step_groups(p, g, m, v, segs, norm, **kw)))(segments(n, count))
    times = {k: [] for k in variants}
    times["one_group_again"] = []       # the same launch a second time per round: the A/A spread
    order = ["one_group", "groups_1", "one_group_again", "groups_3", "one_group", "groups_16", "one_group_again"]
    for fn in variants.values():        # warm-up: code objects, the mirror
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name in order:
            fn = variants["one_group" if name == "one_group_again" else name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    nbytes = n * (16 + 12 + 4 + 2)
    lines = ["adamw pass on n = %d fp32 parameters, fp16 mirror, zero_grad, clip, loss-scaling step size; %d rounds of %s" % (n, a.reps, " ".join(order)),
             "device: %s" % torch.cuda.get_device_name(0)]
    base = statistics.median(times["one_group"])
    for name in ("one_group", "one_group_again", "groups_1", "groups_3", "groups_16"):
        t = sorted(times[name])
        med = statistics.median(t)
        lines.append("%-16s median %.4f ms  (min %.4f, p10 %.4f, p90 %.4f)  %.2f TB/s  vs one_group %+.2f %%" %
                     (name, med, t[0], t[len(t) // 10], t[len(t) * 9 // 10], nbytes / med / 1e9, (med / base - 1.0) * 100.0))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
