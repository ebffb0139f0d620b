"""GPU: the clip augmentation stages (alpro_augment_stage / alpro_augment_stats, csrc/augment.hip) at the pretraining input shape --
B = 64 clips of T = 4 frames, 288 x 288 decoded frames cropped to 224 x 224 on the read side -- one op at a time over the whole
batch, the two-stage chain [ShearX, Rotate] through TemporalConsistentRandomAugment, and the per-frame statistics launch.

    python tools/augment_bench.py [--B 64] [--T 4] [--frame 288] [--crop 224] [--level 8] [--reps 30] [--inner 10] [--out FILE]

The default level is 8, not the 5 of the reference's datasets: at level 5 the enhance factor is exactly 1, Sharpness is a copy by
definition and Brightness multiplies by one, so their level-5 times say nothing about the ops.

HIP-event timings of `inner` back-to-back launches, median over `reps` rounds, every variant in every round.  Bytes: what the stage has
to move -- the crop window read once and the output written once (Color reads each pixel's three channels from all three planes, the
geometric ops read four taps per pixel: re-reads that the caches serve); the bound is those bytes at the measured HBM copy rate."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alpro_amd import hip  # noqa: E402
from alpro_amd.input_gpu import TemporalConsistentRandomAugment, aug_op_args  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=4)
    ap.add_argument("--frame", type=int, default=288)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="HBM copy rate the bound is taken at, TB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, T, F, C = a.B, a.T, a.frame, a.crop
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (B, T, 3, F, F), generator=g, dtype=torch.uint8).cuda()
    rng = np.random.RandomState(0)
    offs = torch.tensor([(rng.randint(0, F - C + 1), rng.randint(0, F - C + 1)) for _ in range(B)], dtype=torch.int32, device="cuda")
    sums, tables = hip.augment_buffers(B, T, src.device)
    dst = torch.empty((B, T, 3, C, C), dtype=torch.uint8, device="cuda")
    window = B * T * 3 * C * C

    def stage_fn(code):
        ops = torch.full((B,), code, dtype=torch.int32, device="cuda")
        args = torch.tensor([aug_op_args(code, a.level)] * B, dtype=torch.float64, device="cuda")
        if code == hip.AUG_OPS["Contrast"]:
            hip.augment_stats(src, ops, args, sums, tables, crop=offs, out_hw=(C, C))
        return lambda: hip.augment_stage(src, ops, args, tables, dst=dst, crop=offs, out_hw=(C, C))

    variants, nbytes = {}, {}
    for name, code in hip.AUG_OPS.items():
        variants[name] = stage_fn(code)
        nbytes[name] = 2 * window
    c_ops = torch.full((B,), hip.AUG_OPS["Contrast"], dtype=torch.int32, device="cuda")
    c_args = torch.tensor([aug_op_args(hip.AUG_OPS["Contrast"], a.level)] * B, dtype=torch.float64, device="cuda")
    variants["stats (Contrast, every clip)"] = lambda: hip.augment_stats(src, c_ops, c_args, sums, tables, crop=offs, out_hw=(C, C))
    nbytes["stats (Contrast, every clip)"] = window + B * T * (256 + 24)
    aug = TemporalConsistentRandomAugment(N=2, M=a.level)
    chain_ops = np.array([[hip.AUG_OPS["ShearX"], hip.AUG_OPS["Rotate"]]] * B, dtype=np.int32)
    offs_host = [tuple(int(v) for v in o) for o in offs.cpu().numpy()]
    variants["chain [ShearX, Rotate] via __call__"] = lambda: aug(src, ops=chain_ops, crop_size=C, crop_offsets=offs_host)
    nbytes["chain [ShearX, Rotate] via __call__"] = 4 * window       # two stages, each one read and one write (plus the host's argument upload)

    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    lines = ["augmentation stages: B = %d, T = %d, %d x %d frames cropped to %d x %d, level %d; us per batch, median of %d rounds of %d launches"
             % (B, T, F, F, C, C, a.level, a.reps, a.inner), "device: %s; bound = bytes / %.2f TB/s" % (torch.cuda.get_device_name(0), a.hbm_tbs)]
    for name in variants:
        t = sorted(times[name])
        med = statistics.median(t)
        lines.append("%-38s %9.1f us  (min %.1f, p90 %.1f)  %7.2f MB  bound %6.1f us  %5.2f TB/s" %
                     (name, med, t[0], t[len(t) * 9 // 10], nbytes[name] / 1e6, nbytes[name] / a.hbm_tbs / 1e6, nbytes[name] / med / 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
