"""GPU: the HIP path's pixel gradient against the REFERENCE's own TimeSformer and autograd (tests/golden/vit_pixel_grad_*.npz, written by
tests/golden/make_golden_pixel_grad.py): both small geometries, the three pooling modes, exact fp32 mode and fp16 under a scaled backward.
Limits as in tests/test_pixel_grad_gpu.py (a fraction of the largest reference magnitude: fp32 2e-4, fp16 1e-2); outputs, where the fixture
holds them, within the limits tests/test_pool_modes_parity.py applies to encoder outputs."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.golden.make_golden_pixel_grad import MODES, fixture_name, out_modes
from tests.golden.make_golden_pool_modes import GEOMETRIES, fixture_name as pool_fixture_name
from tests.test_pixel_grad_gpu import TOL, cases, run  # noqa: F401  (cases: the module-scoped fixture)
from tests.test_pool_modes_parity import OUT_TOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pooling", MODES)
@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_pixel_gradient_vs_reference(cases, mode, geo, pooling):
    enc, x, _ = cases(geo)
    g = np.load(os.path.join(GOLDEN, fixture_name(GEOMETRIES[geo])))
    assert np.array_equal(g["x"].astype(np.float32), x.cpu().numpy())
    out, dx, _, _ = run(enc, x, pooling, mode)
    want = g[pooling + "/dx"].astype(np.float64)
    top = float(np.abs(want).max())
    err = float(np.abs(dx.double().cpu().numpy() - want).max())
    if pooling in out_modes(GEOMETRIES[geo]):
        ref_out = g[pooling + "/out"]
    else:   # (the 'spatial' and 'none' outputs at img 64 did not fit beside the gradients: the pool-modes fixture of the same encoder and clips has them)
        ref_out = np.load(os.path.join(GOLDEN, pool_fixture_name(GEOMETRIES[geo])))[pooling + "/out"]
    e_out = float(np.abs(out.double().cpu().numpy() - ref_out).max())
    print("\n[pixel gradient vs reference %s img%d %s] max |dx| %.3e err %.3e = %.3e of it (limit %.0e); output err %.2e (limit %.0e)"
          % (mode, GEOMETRIES[geo]["img"], pooling, top, err, err / top, TOL[mode], e_out, OUT_TOL[mode]))
    assert bool(torch.isfinite(dx).all()) and err <= TOL[mode] * top
    assert e_out <= OUT_TOL[mode]
