"""bench.py --dump-outputs: what the last timed step returned, written as DIR/<name>.npy (float32 / float64, fixed samples of large
outputs) so that two builds can be compared output for output; and a plain run stays lean (the extra passes are behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_writes_float_arrays_and_fixed_samples(tmp_path):
    import bench
    n = bench.DUMP_MAX_ELEMS
    g = torch.Generator().manual_seed(5)
    outs = {"loss": torch.tensor(1.5), "scores": torch.randn(7, 3, generator=g).to(torch.bfloat16), "labels": torch.arange(5),
            "big": torch.arange(3 * n, dtype=torch.float32), "absent": None}
    params = [torch.randn(10, generator=g), torch.randn(50, 100, generator=g)]
    bench.dump_outputs(str(tmp_path / "a"), outs, params)
    bench.dump_outputs(str(tmp_path / "b"), outs, params)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert sorted(a) == ["big", "labels", "loss", "params_sample", "scores"]
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
        np.testing.assert_array_equal(v, b[k])          # the same sample every time
    assert a["loss"].shape == (1,) and a["loss"][0] == 1.5
    np.testing.assert_array_equal(a["scores"], outs["scores"].float().reshape(-1).numpy())
    np.testing.assert_array_equal(a["labels"], np.arange(5, dtype=np.float64))
    big = a["big"]                                      # a sample of 3n: n of its elements, in index order
    assert big.shape == (n,) and np.all(np.diff(big) >= 0) and big.min() >= 0 and big.max() < 3 * n and len(np.unique(big)) > n // 2
    assert a["params_sample"].shape == (10 + bench.DUMP_PARAM_SAMPLE,)
    np.testing.assert_array_equal(a["params_sample"][:10], params[0].numpy())    # whole tensors when they are small enough


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """Two plain single-GPU runs with the same arguments: exactly --steps timed steps reported, none of the --full extras, and bitwise the
    same dumped outputs (deterministic reductions are the default) -- within the 64 MB the dump may take."""
    dumps, lines = [], []
    for run in ("a", "b"):
        d = tmp_path / run
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2", "--frames", "2", "--steps", "2", "--warmup", "1",
               "--dump-outputs", str(d)]
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, out.stdout[-2000:]
        lines.append(json.loads(js[0]))
        dumps.append(_load_dir(d))
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    for r in lines:
        assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
        assert r["metric"] and r["unit"] == "pairs/s" and r["higher_is_better"] is True and r["dtype"] == "fp16"
        assert not {"roofline", "kernel_ms_per_step", "cpu_baseline"} & set(r) and r["parity"]["measured_in_this_run"] is False
    a, b = dumps
    assert {"loss", "itc_loss", "itm_scores", "mlm_scores", "mpm_logits", "params_sample"} <= set(a) and sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.all(np.isfinite(a[k])), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
