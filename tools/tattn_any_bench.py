"""Micro- and model-level benchmark of temporal attention across frame counts: the block-diagonal kernels at T = 8, 16 (T divides 32) and
the windowed kernels of attention_temporal_any.hip at T = 6, 12, 24, 48, 96, 128, at equal row counts (rows = the largest multiple of T not
above 32 clips x 196 patches x 16 frames = 100352), 12 heads, head_dim 64; then the visual-encoder forward and a retrieval fine-tune step
(itm_loss + itc_loss, forward + backward, no optimizer) at T = 12 against T = 16, B = 8 clips, fp16 operands with precise [CLS] rows.

    python tools/tattn_any_bench.py [--iters 20] [--warmup 5] [--no-model]

Kernel times are HIP events around `iters` back-to-back calls after `warmup` calls, reported per 1M token rows.  GB/s counts the bytes the
kernel must move once (forward: q | k | v read, o written; backward: q | k | v, o, dO read, dq | dk | dv written; lse ignored)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from alpro_amd import hip  # noqa: E402

H = 12
ROWS = 32 * 196 * 16


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


def kernels(a):
    print("temporal attention per frame count: %d rows (T | rows), H=%d, head_dim 64; %s" % (ROWS, H, torch.cuda.get_device_name()))
    print("%-5s %4s %-14s %9s %11s %7s   %9s %11s %7s" % ("dtype", "T", "kernel", "fwd us", "us/1M rows", "GB/s", "bwd us", "us/1M rows", "GB/s"))
    g = torch.Generator(device="cuda").manual_seed(0)
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        base = None
        for T in (8, 16, 6, 12, 24, 48, 96, 128):
            rows = ROWS // T * T
            qkv = (torch.randn(rows, 3 * H * 64, device="cuda", generator=g) * 0.7).to(dt)
            dout = torch.randn(rows, H * 64, device="cuda", generator=g).to(dt)
            out, lse = hip.attn_temporal(qkv, T, H, 0.125, want_lse=True)
            tf = timeit(lambda: hip.attn_temporal(qkv, T, H, 0.125, want_lse=True), a.iters, a.warmup)
            tb = timeit(lambda: hip.attn_temporal_bwd(qkv, out, dout, lse, T, H, 0.125), a.iters, a.warmup)
            pf, pb = tf / rows * 1e6, tb / rows * 1e6
            bf, bb = rows * H * 64 * 2 * 4, rows * H * 64 * 2 * 8
            rel = ""
            if T == 16:
                base = (pf, pb)
            elif base and T != 8:
                rel = "   vs T=16 per row: fwd %.2fx  bwd %.2fx" % (pf / base[0], pb / base[1])
            kind = "block-diagonal" if 32 % T == 0 else "windowed"
            print("%-5s %4d %-14s %9.1f %11.1f %7.0f   %9.1f %11.1f %7.0f%s" % (name, T, kind, tf, pf, bf / tf / 1e3, tb, pb, bb / tb / 1e3, rel))
            del qkv, dout, out, lse


def model(a):
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import AlproForVideoTextRetrieval
    from tests.conftest import BERT_CFG
    from tests.golden.det_init import det_batch, fill_state_dict_
    from tests.test_host_cpu import VENC, make_cfg
    from tests.test_model_parity import arm_scale, backward
    B, Lt = 8, 40
    print("\nretrieval model, B=%d clips x 224^2, %d-token captions, fp16 operands + precise CLS rows" % (B, Lt))
    res = {}
    for T in (16, 12):
        torch.manual_seed(0)
        m = AlproForVideoTextRetrieval(make_cfg(BERT_CFG), dict(VENC, num_frm=T))
        fill_state_dict_(m)
        m.eval().cuda()
        batch = det_batch(B, T, Lt=Lt, seed_name="tattn_any_bench", with_mlm=False, with_mpm=False)
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
        vis = batch["visual_inputs"]
        pick = lambda w, n=1, *x, **k: w.argmax(dim=-1, keepdim=True)  # noqa: E731
        orig = torch.multinomial
        torch.multinomial = pick
        try:
            with rt.use_compute_dtype("fp16"):
                def enc():
                    with torch.no_grad():
                        m.visual_encoder.forward_features(vis.transpose(1, 2), return_all_tokens=True)

                def step():
                    for p in m.parameters():
                        p.grad = None
                    keep = arm_scale("fp16")
                    out = m(batch)
                    backward(out["itm_loss"] + out["itc_loss"], "fp16")
                    del keep
                te = timeit(enc, a.iters, a.warmup) / 1e3
                ts = timeit(step, max(3, a.iters // 4), 2) / 1e3
        finally:
            torch.multinomial = orig
        res[T] = (te, ts)
        print("T=%3d  visual encoder forward %8.2f ms (%6.3f ms/frame)   fine-tune step %8.2f ms (%6.3f ms/frame)" % (T, te, te / T, ts, ts / T))
        del m
        torch.cuda.empty_cache()
    print("T=12 vs T=16 per frame: encoder forward %.3fx, fine-tune step %.3fx" % ((res[12][0] / 12) / (res[16][0] / 16), (res[12][1] / 12) / (res[16][1] / 16)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tattn_any_bench needs a GPU"
    hip.load()
    kernels(a)
    if not a.no_model:
        model(a)


if __name__ == "__main__":
    main()
