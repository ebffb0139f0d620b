"""GPU: TimeSformer.forward_features(output_attentions=True, output_hidden_states=True) against what the hooks see on the reference's own
TimeSformer (tests/golden/vit_attn_*.npz, written by tests/golden/make_golden_vit_attn.py): every temporal map, the spatial maps of blocks 0, 5, 11,
three token rows of all 13 hidden states, and the features -- in exact fp32 mode and in fp16 with the precise CLS chain (fp16's default).

Maps: 2e-4 (fp32) / 8e-4 (fp16) of the reference map's largest element.  Hidden rows and features: the limits tests/test_model_parity.py applies to
the encoder output, as tests/test_pool_modes_parity.py reads them."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.golden.det_init import fill_state_dict_
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips
from tests.golden.make_golden_vit_attn import DEPTH, SPATIAL_BLOCKS, fixture_name, hidden_rows
from tests.test_host_cpu import VENC
from tests.test_pool_modes_parity import OUT_TOL          # fp32 1e-3, fp16 6e-3 (from tests/test_model_parity.py)

pytestmark = pytest.mark.gpu

MAP_TOL = {"fp32": 2e-4, "fp16": 8e-4}


@pytest.fixture(scope="module")
def cases():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    built = {}

    def get(i):
        if i not in built:
            geo = GEOMETRIES[i]
            enc = fill_state_dict_(TimeSformer(dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0), input_format="RGB"))
            built[i] = (enc.eval().cuda(), pool_clips(geo).cuda(), np.load(os.path.join(GOLDEN, fixture_name(geo))))
        return built[i]
    return get


def _err(got, ref):
    return float(np.abs(got.detach().float().cpu().numpy().astype(np.float64) - np.asarray(ref, dtype=np.float64)).max())


@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_maps_hidden_rows_and_features_vs_reference(cases, mode, geo):
    from alpro_amd import config as rt
    enc, x, g = cases(geo)
    G = GEOMETRIES[geo]
    B, T, N = G["B"], G["T"], (G["img"] // 16) ** 2
    with rt.use_compute_dtype(mode), torch.no_grad():
        out = enc.forward_features(x, output_attentions=True, output_hidden_states=True)
    assert len(out.temporal_attentions) == DEPTH == len(out.spatial_attentions) and len(out.hidden_states) == DEPTH + 1
    worst = {}
    fails = []
    for i in range(DEPTH):
        for kind, maps in (("temporal", out.temporal_attentions), ("spatial", out.spatial_attentions)):
            if kind == "spatial" and i not in SPATIAL_BLOCKS:
                continue
            ref = g["%s/%d" % (kind, i)]
            assert tuple(maps[i].shape) == ref.shape and maps[i].dtype == torch.float32
            e, lim = _err(maps[i], ref), MAP_TOL[mode] * float(np.abs(ref).max())
            if e / lim > worst.get(kind, (0, 0, 0))[0]:
                worst[kind] = (e / lim, e, lim, i)
            if e > lim:
                fails.append((kind, i, e, lim))
    rows = list(hidden_rows(N, T))
    hid = torch.stack([h[:, rows] for h in out.hidden_states])
    assert tuple(hid.shape) == g["hidden_rows"].shape == (DEPTH + 1, B, 3, 768)
    e_hid = [_err(hid[i], g["hidden_rows"][i]) for i in range(DEPTH + 1)]
    e_feat = _err(out.features, g["features"])
    print("\n[vit attn parity %s img%d T%d] worst temporal map err %.2e of limit %.2e (block %d); worst spatial map err %.2e of limit %.2e (block %d); "
          "hidden rows max err %.2e (state %d), features %.2e, limit %.1e"
          % (mode, G["img"], T, worst["temporal"][1], worst["temporal"][2], worst["temporal"][3], worst["spatial"][1], worst["spatial"][2], worst["spatial"][3],
             max(e_hid), int(np.argmax(e_hid)), e_feat, OUT_TOL[mode]))
    assert not fails, fails
    assert max(e_hid) <= OUT_TOL[mode], e_hid
    assert e_feat <= OUT_TOL[mode]
