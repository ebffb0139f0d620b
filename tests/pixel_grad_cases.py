"""Case builders for alpro_unpatchify (CPU torch only, not collected): the shapes of tests/movement_cases.py's patchify cases, rows whose every
element names its own place, and the reference -- F.fold, the inverse of the F.unfold that movement_cases.patchify_ref is.

A 16-bit source holds (linear index mod 127) - 64, exact in bf16 and fp16; an fp32 source holds the linear index itself (below 2^24).  This is
patchify_image's recipe applied to the rows, with the prime 127 for its 129: in the IMAGE two vertical neighbours on either side of a patch border
are W/16 rows less 240 elements apart, which 129 divides at W = 48 (3 * 768 - 240 = 16 * 129).  With 127 every pixel differs from its right and
its lower neighbour in all five shapes (tests/test_pixel_grad_cpu.py asserts it), so a shifted, transposed or repeated write cannot pass."""
import torch
import torch.nn.functional as F

from tests.gemm_cases import F32, F64
from tests.movement_cases import PATCHIFY_SHAPES

SHAPES = PATCHIFY_SHAPES   # (BT, C, H, W): (1,3,16,16), (1,1,16,16), (2,3,16,64), (2,3,64,16), (3,3,32,48)


def rows_shape(shape):
    BT, C, H, W = shape
    return BT * (H // 16) * (W // 16), C * 256


def unpatchify_rows(shape, dt):
    """The (BT * N, C * 256) source in dtype dt with row-identifying values."""
    R, K = rows_shape(shape)
    v = torch.arange(R * K).view(R, K)
    v = v if dt == F32 else v % 127 - 64
    out = v.to(dt)
    assert torch.equal(out.to(F64), v.to(F64))
    return out


def unpatchify_ref(rows, BT, C, H, W):
    """(BT, C, H, W) fp32: F.fold of the rows with the patch index moved behind (F.unfold's layout (BT, C*256, N)), widened exactly."""
    N = (H // 16) * (W // 16)
    cols = rows.to(F64).view(BT, N, C * 256).transpose(1, 2)
    return F.fold(cols, output_size=(H, W), kernel_size=16, stride=16).to(F32)


# ------------------------------------------------------------------------------------------------ the fp64 oracle of the pixel gradient
POOLINGS = ("temporal", "spatial", "none")
_ORACLE = {}


def oracle_pool(y, mode, B, T):
    """The encoder's (B, 1 + N*T, D) fp64 output rows, patch (n, t) at row 1 + n*T + t -> forward_features' value (vit.py:484-499)."""
    D = y.shape[-1]
    cls, p = y[:, :1], y[:, 1:].reshape(B, -1, T, D).permute(0, 2, 1, 3)   # (B, T, N, D)
    if mode == "spatial":
        return torch.cat([cls, p.mean(2)], 1)
    return torch.cat([cls.unsqueeze(1).expand(B, T, 1, D), p], 2)


def oracle_pixel_grads(enc, x, T):
    """enc: a TimeSformer (any device; its parameters are read as fp64 on the CPU), x (B, C, T, H, W) -> {mode: (out, dx)} in fp64 from
    oracle.alpro_oracle with autograd to x, under loss = (out * pool_probe(mode, out.shape)).sum().  'temporal' is the oracle's own
    timesformer_forward_features; the two frame-resolved poolings pool the rows of its vit_forward_features."""
    from oracle import alpro_oracle as orc
    from tests.golden.make_golden_pool_modes import pool_probe
    p = {"enc." + k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
    B = x.shape[0]
    res = {}
    for mode in POOLINGS:
        x64 = x.detach().cpu().double().requires_grad_(True)
        if mode == "temporal":
            out = orc.timesformer_forward_features(x64, p, "enc", T)
        else:
            out = oracle_pool(orc.vit_forward_features(x64, p, "enc.model"), mode, B, T)
        (out * pool_probe(mode, out.shape).double()).sum().backward()
        res[mode] = (out.detach(), x64.grad)
    return res


def oracle_case(i):
    """Geometry i of make_golden_pool_modes.GEOMETRIES -> (CPU encoder with det_init weights in eval mode, clips, {mode: (out64, dx64)}), once."""
    if i not in _ORACLE:
        from alpro_amd.modeling.timesformer.vit import TimeSformer
        from tests.golden.det_init import fill_state_dict_
        from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips
        from tests.test_host_cpu import VENC
        geo = GEOMETRIES[i]
        enc = TimeSformer(dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0), input_format="RGB")
        fill_state_dict_(enc)
        enc.eval()
        x = pool_clips(geo)
        with torch.enable_grad():
            _ORACLE[i] = (enc, x, oracle_pixel_grads(enc, x, geo["T"]))
    return _ORACLE[i]
