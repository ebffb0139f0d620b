"""GPU: the image-text stream's batch preparation (alpro_resized_crop, csrc/resample.hip, and prepare_pretrain_images) at the pretraining
input shape -- B = 64 decoded images of mixed sizes around 500 x 375 (both orientations), RandomResizedCrop boxes drawn as the dataset
draws them, resized to 256 x 256 -- as device time per batch:

    resized_crop                 the two resampling launches and the upload of their geometry and coefficient table
    resized_crop, table resident the two launches alone (the raw entry point on a table already on the device)
    prepare_pretrain_images      the whole branch: resized crop + flip, RandomAugment's stages, the repeat to num_frm frames, random erase + ImageNorm
    pack_images                  the host-to-device copy of the decoded pixels (pageable memory), for scale

    python tools/image_bench.py [--B 64] [--size 256] [--frames 4] [--reps 30] [--inner 10] [--out FILE]

HIP-event timings of `inner` back-to-back calls, median over `reps` rounds, every variant in every round, after three warm-up calls of
each.  The host work of a call (the fp64 coefficient table in numpy, drawing boxes) overlaps the device work of the call before it, so
the event time of a call whose device work is shorter than its host work is the HOST time; the wall line says which one a row shows.
If PIL is importable, the single-thread wall time of Image.crop().resize(BICUBIC) on the same images and boxes is recorded too."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alpro_amd import hip  # noqa: E402
from alpro_amd.input_gpu import RandomAugment, pack_images, prepare_pretrain_images, resample_table, sample_resized_crops  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
AUGS = ["Identity", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, S = a.B, a.size
    rng = np.random.RandomState(0)
    sizes = []
    for b in range(B):
        long_, short = 500 + rng.randint(-60, 61), 375 + rng.randint(-60, 61)
        sizes.append((short, long_) if b % 4 else (long_, short))          # (H, W): three landscape images to one portrait
    images = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes]
    boxes = sample_resized_crops(sizes, rng=np.random.RandomState(1))
    flips = [bool(b & 1) for b in range(B)]
    packed, _ = pack_images(images)
    max_h = max(bx[2] for bx in boxes)
    tmp = torch.empty(B * max_h * 3 * S, dtype=torch.uint8, device="cuda")
    dst = torch.empty((B, 1, 3, S, S), dtype=torch.uint8, device="cuda")
    host, _, ktaps = resample_table(sizes, boxes, flips, S)
    table = torch.from_numpy(host).cuda()
    lib, vp = hip.load(), ctypes.c_void_p
    aug = RandomAugment(2, 7, isPIL=True, augs=AUGS)
    aug_ops = aug.sample(B, rng=np.random.RandomState(2))

    def raw():
        rc = lib.alpro_resized_crop(vp(packed.data_ptr()), packed.numel(), vp(table.data_ptr()), vp(table.data_ptr() + B * 64), vp(tmp.data_ptr()),
                                    vp(dst.data_ptr()), B, S, max_h, ktaps, vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.alpro_hip_last_error().decode()

    variants = {
        "resized_crop": lambda: hip.resized_crop(packed, sizes, boxes, flips, S, dst=dst, tmp=tmp),
        "resized_crop, table resident": raw,
        "prepare_pretrain_images": lambda: prepare_pretrain_images((packed, sizes), MEAN, STD, crop_size=S, num_frm=a.frames, augment=aug, crop_boxes=boxes,
                                                                   flips=flips, aug_ops=aug_ops, rng=rng),
        "pack_images (host to device)": lambda: pack_images(images),
    }
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    raw()
    assert torch.equal(dst, hip.resized_crop(packed, sizes, boxes, flips, S)), "the raw entry point and the wrapper disagree"
    times, walls = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.inner)
            walls[name].append((t1 - t0) * 1e3 / a.inner)
    src_px = sum(bx[2] * bx[3] for bx in boxes)
    lines = ["image-text batch preparation: B = %d images of %d..%d x %d..%d pixels (%.1f MB packed), crops of %.0f %% of the pixels on average, to %d x %d, %d frames;"
             % (B, min(min(s) for s in sizes), max(min(s) for s in sizes), min(max(s) for s in sizes), max(max(s) for s in sizes), packed.numel() / 1e6,
                100.0 * src_px * 3 / packed.numel(), S, S, a.frames),
             "ms per batch, median of %d rounds of %d calls; device = HIP events around the calls, host = the time the calls took to ENQUEUE; ktaps %d, max h %d"
             % (a.reps, a.inner, ktaps, max_h), "device: %s" % torch.cuda.get_device_name(0)]
    for name in variants:
        t = sorted(times[name])
        lines.append("%-32s device %8.3f ms  (min %.3f, p90 %.3f)   host %8.3f ms" % (name, statistics.median(t), t[0], t[len(t) * 9 // 10],
                                                                                      statistics.median(walls[name])))
    try:
        from PIL import Image
        pil = [Image.fromarray(im) for im in images]
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for im, (top, left, h, w) in zip(pil, boxes):
                im.crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        lines.append("%-32s wall   %8.3f ms  (one thread, best of 3, PIL %s; crop + resize only, no flip, no ops)" % ("PIL crop().resize(BICUBIC)", best, Image.__version__))
        got = hip.resized_crop(packed, sizes, boxes, None, S).cpu().numpy()
        same = all(np.array_equal(got[b, 0].transpose(1, 2, 0), np.asarray(im.crop((l, t, l + w, t + h)).resize((S, S), Image.BICUBIC)))
                   for b, (im, (t, l, h, w)) in enumerate(zip(pil, boxes)))
        lines.append("device output equals PIL's on all %d images: %s" % (B, same))
    except ImportError:
        lines.append("PIL is not importable here: no host comparison")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
