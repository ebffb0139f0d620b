"""Stress inputs, fp64 references, fp32 emulators and derived allowances for the row-wise kernels: the LayerNorm family, the softmax
cross-entropy and the AdamW step epilogue.  Shared by tests/test_hip_rowwise_stress.py (GPU) and tests/test_rowwise_cases_cpu.py (CPU
self-check); not collected itself, and nothing here touches a GPU.

Every input lies on a grid that fp32 holds exactly (16-bit operands are pre-rounded to their dtype), so a kernel and its fp64 reference
see the same operands.  The emulators restate the kernels' fp32 arithmetic in torch on the CPU (alpro_amd/csrc/row768.hpp ln_stats /
ln_affine, backward.hip row_grad, loss.hip xent_kernel, optim.hip adamw_kernel); `fault=` plants one bug at a time.  The allowance
constants below come from the fault-free emulators against fp64 (tests/test_rowwise_cases_cpu.py re-measures them on every run), never
from a kernel's output.
"""
import math

import torch

F32, F64 = torch.float32, torch.float64
LN_D = 768
U24 = 2.0 ** -24          # half an fp32 ulp at 1: the unit of the conditioning terms


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def on_grid(x, step):
    """Round to multiples of `step` (a power of two); exact in fp32 while |x| < step * 2^24."""
    y = (torch.round(x.double() / step) * step).float()
    assert float(y.abs().max()) < step * 2 ** 24
    return y


# ------------------------------------------------------------------------------------------------ LayerNorm rows
LN_REGIMES = ("gauss", "offset", "outlier", "scale_span", "flat", "mixed")
# eps the regime is run under: BERT's 1e-12 where a row is (near) constant, ViT's 1e-6 elsewhere (scale_span's smallest rows have a variance
# of 6e-6: there 1e-6 is a tenth of the denominator and a kernel that drops it shows)
LN_EPS = {"gauss": 1e-6, "offset": 1e-6, "outlier": 1e-6, "scale_span": 1e-6, "flat": 1e-12, "mixed": 1e-12}
# outlier channels: column 767 (lane 63, last group, last element), column 3 (lane 0, first 4-column group), 581 = 2*256 + 17*4 + 1 (last
# group of lane 17), then three more; row r carries the first 2 + r % 5 of them
OUTLIER_COLS = (767, 3, 581, 300, 131, 515)
_MIX = ("offset", "flat", "outlier", "scale_span", "gauss")


def _ln_rows_one(rows, regime, g, row0=0):
    r = torch.arange(row0, row0 + rows)
    z = torch.randn(rows, LN_D, generator=g)
    u = torch.rand(rows, 4, generator=g)
    if regime == "gauss":
        return on_grid(z * 2.5 + 0.4, 2.0 ** -10)
    if regime == "offset":
        mean = (55 + 145 * u[:, :1]) * torch.where(u[:, 1:2] < 0.5, -1.0, 1.0)
        return on_grid(mean + (0.1 + 0.8 * u[:, 2:3]) * z, 2.0 ** -10)
    if regime == "outlier":
        x = on_grid(z, 2.0 ** -10)
        mag = on_grid((60 + 140 * torch.rand(rows, len(OUTLIER_COLS), generator=g)) * torch.where(torch.rand(rows, len(OUTLIER_COLS), generator=g) < 0.5, -1.0, 1.0), 2.0 ** -10)
        for k, c in enumerate(OUTLIER_COLS):
            has = (2 + r % 5) > k
            x[:, c] = torch.where(has, mag[:, k], x[:, c])
        return x
    if regime == "scale_span":
        return on_grid(z * 2.5 + 0.4, 2.0 ** -10) * (2.0 ** ((r % 21) - 10).float())[:, None]
    if regime == "flat":
        mean = on_grid(0.9 + 0.2 * u[:, :1], 2.0 ** -10)
        x = mean + on_grid(z * 2.0 ** -10, 2.0 ** -16)
        const = (r % 4 == 1)[:, None]
        return torch.where(const, mean.expand(rows, LN_D), x).contiguous()
    raise ValueError(regime)


def ln_rows(rows, regime, seed=0):
    """-> fp32 (rows, 768) token rows of the named regime (LN_REGIMES); `mixed` takes row r from _MIX[r % 5]."""
    g = _gen(1000 + seed)
    if regime != "mixed":
        return _ln_rows_one(rows, regime, g)
    parts = {k: _ln_rows_one(rows, k, g) for k in _MIX}
    out = torch.empty(rows, LN_D)
    for i, k in enumerate(_MIX):
        out[i::5] = parts[k][i::5]
    return out


def ln_params(seed=0):
    """gamma, beta as the existing tests draw them, on the 2^-12 grid."""
    g = _gen(2000 + seed)
    return on_grid(1 + 0.1 * torch.randn(LN_D, generator=g), 2.0 ** -12), on_grid(0.1 * torch.randn(LN_D, generator=g), 2.0 ** -12)


def delta_rows(rows, dt, seed=0, scale=1.0):
    """A branch output / incoming gradient in the operand dtype: Gaussian, pre-rounded to dt."""
    return (torch.randn(rows, LN_D, generator=_gen(3000 + seed)) * scale).to(dt)


def ln_ref(x, gamma, beta, eps):
    """fp64: -> y, mean, rstd of the rows of x."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (x - mean) * rstd * gamma.double() + beta.double(), mean.squeeze(-1), rstd.squeeze(-1)


def ln_bwd_ref(x, dy, gamma, eps):
    """fp64: -> dx rows, per-row dgamma terms dy * xhat (sum over rows = dgamma; dbeta = dy.sum(0))."""
    x, dy, g = x.double(), dy.double(), gamma.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    d = dy * g
    return rstd * (d - d.mean(-1, keepdim=True) - xh * (d * xh).mean(-1, keepdim=True)), dy * xh


# The fp32 two-pass statistics are ill-conditioned where max|x| * rstd is large, whatever the kernel does: the mean of 768 fp32 values
# carries an error of a few 2^-24 * max|x|, and every normalised value inherits it times rstd.  a = C * 2^-24 * max|x_row| * rstd_row
# (rstd from the fp64 reference) is that error in units of xhat; the allowances are the project's tolerances plus:
#   y:      a * max|gamma|                     mean: a / rstd              rstd: rstd * a^2  (var' = var + dmean^2)
#   dx:     a * rstd * max|dy_row * gamma|     dgamma[c]: sum over rows of a_row * |dy[row, c]|
# C: the smallest power of two the fault-free emulator passes with in both of its summation orders, times 4 for the orders it does not
# implement.  Measured by tests/test_rowwise_cases_cpu.py::test_rowwise_emulators_pass_and_measure_the_allowance_constants over every
# regime and row count, as the error beyond the plain tolerance / (2^-24 * max|x| * rstd * max|gamma|): forward 2.01 in the kernels' lane
# order and 20.2 in the sequential order (`offset` rows: 767 running sums near 768 * mean) -> 32 * 4 = 128; backward dx 0.09 (lane) and
# 1.60 (sequential) -> 2 * 4 = 8.  The sequential order sets the forward constant, so with `gauss` rows (max|x| * rstd about 4.5) the
# forward term is 128 * 6e-8 * 4.5 * 1.3 = 4.5e-5: above the existing 1e-5, not below it as hoped.  tests/test_hip_ops.py keeps the
# plain 1e-5 check of that regime.
LN_C = 128.0
LN_BWD_C = 8.0
# loss_rows = lse - x[label] with lse = max + log(sum): one rounding of a value as large as max|logit|, another in the subtraction.  Worst
# emulator error beyond 1e-5 / (2^-24 * max|logit_row|) = 0.535 (offset, V = 2, both orders) -> 1 * 4 = 4.
XENT_C = 4.0


def ln_a(x, eps, c=LN_C):
    """(rows,) fp64: the conditioning unit a = c * 2^-24 * max|x_row| * rstd_row of the rows of x (the LayerNorm INPUT, after any add)."""
    x = x.double()
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + eps)
    return c * U24 * x.abs().amax(-1) * rstd, rstd


def ln_fwd_extra(x, gamma, eps, c=LN_C):
    """(rows, 1) absolute allowance on top of the dtype's tolerance for LayerNorm(x) rows."""
    a, _ = ln_a(x, eps, c)
    return (a * float(gamma.abs().max()))[:, None]


def ln_stats_extra(x, eps, c=LN_C):
    """-> (mean allowance, rstd allowance), (rows,) each, on top of the existing 1e-5 pair."""
    a, rstd = ln_a(x, eps, c)
    return a / rstd, rstd * a * a


def ln_dx_extra(x, dy, gamma, eps, c=LN_BWD_C):
    a, rstd = ln_a(x, eps, c)
    return (a * rstd * (dy.double() * gamma.double()).abs().amax(-1))[:, None]


def ln_dgamma_extra(x, dy, eps, c=LN_BWD_C):
    a, _ = ln_a(x, eps, c)
    return (a[:, None] * dy.double().abs()).sum(0)


def excess(got, ref, rtol, atol, extra=0.0):
    """max of err / allowed (<= 1 passes); inf if got is not finite where ref is."""
    got, ref = got.detach().cpu().double(), ref.double()
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref).abs() / (atol + rtol * ref.abs() + extra)).max())


def check(got, ref, rtol, atol, extra=0.0, what=""):
    r = excess(got, ref, rtol, atol, extra)
    assert r <= 1.0, "%s: worst error is %.3g x the allowance" % (what, r)


# ---- token-row algebra of the divided space-time block (vit.py), shared by references and emulators; dtype-agnostic
def frame_gather(t, B, T, N):
    """(B, 1 + N*T, D) -> (B*T*(N+1), D): per frame the clip's CLS row, then its N patch rows (MAP_FRAME_TOKENS)."""
    D = t.shape[-1]
    xs = t[:, 1:].reshape(B, N, T, D).permute(0, 2, 1, 3)
    return torch.cat([t[:, :1].unsqueeze(1).expand(B, T, 1, D), xs], 2).reshape(-1, D)


def pre_mlp_add(x, delta, B, T, N, div=None):
    """x (B, S, D) + delta in frame-token order: patches scattered back, the CLS row gets the frame mean (sum / div, div = T)."""
    D = x.shape[-1]
    dd = delta.view(B, T, N + 1, D)
    out = x.clone()
    cls = dd[:, 0, 0].clone()
    for t in range(1, T):          # frame order, as the kernel adds them
        cls = cls + dd[:, t, 0]
    out[:, 0] = out[:, 0] + cls * (x.new_tensor(1.0) / (div or T))
    out[:, 1:] = out[:, 1:] + dd[:, :, 1:].permute(0, 2, 1, 3).reshape(B, N * T, D)
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm emulators (fp32)
def _lanes(x):
    """(R, 768) -> (R, 64, 12): lane l holds columns i*256 + l*4 + j at index 4*i + j (ln_load)."""
    return x.view(-1, 3, 64, 4).permute(0, 2, 1, 3).reshape(-1, 64, 12)


def _unlanes(v):
    return v.view(-1, 64, 3, 4).permute(0, 2, 1, 3).reshape(-1, LN_D)


_XOR = {o: torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)}


def wave_sum(s):
    """common.hpp wave_sum on (..., 64): the xor butterfly, 32 first."""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _XOR[o]]
    return s[..., 0]


def row_sum(v, order, skip_last_lane=False):
    """Sum over the 768 columns of lane-layout values v (R, 64, 12) in fp32.  order 'lane': 12 values per lane in register order, then the
    butterfly (the kernels); 'seq': columns 0..767 one after the other."""
    if skip_last_lane:
        v = v.clone()
        v[:, 63] = 0
    if order == "lane":
        s = v[..., 0].clone()
        for k in range(1, 12):
            s = s + v[..., k]
        return wave_sum(s)
    c = _unlanes(v)
    s = c[:, 0].clone()
    for k in range(1, LN_D):
        s = s + c[:, k]
    return s


def emu_ln(x, gamma, beta, eps, order="lane", fault=None):
    """ln_stats + ln_affine in fp32 -> y, mean, rstd.  fault: 'var_e2' (variance as E[x^2] - mean^2), 'no_eps', 'skip_last_lane' (lane
    63's twelve columns left out of both sums)."""
    assert x.dtype == F32
    inv = torch.tensor(1.0 / LN_D, dtype=F32)
    v = _lanes(x)
    skip = fault == "skip_last_lane"
    mean = row_sum(v, order, skip) * inv
    if fault == "var_e2":
        var = row_sum(v * v, order, skip) * inv - mean * mean
    else:
        d = v - mean[:, None, None]
        var = row_sum(d * d, order, skip) * inv
    rstd = torch.rsqrt(var + (0.0 if fault == "no_eps" else torch.tensor(eps, dtype=F32)))
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    return y, mean, rstd


def emu_ln_grid(x, gamma, beta, eps, nwaves, fault=None):
    """layernorm_fwd_kernel's grid-stride walk: wave w takes rows w, w + nwaves, ...; 'one_trip': every wave stops after its first row.
    Rows nobody wrote stay at the 7.0 the output buffer was filled with."""
    y = torch.full_like(x, 7.0)
    rows = x.shape[0] if fault != "one_trip" else min(x.shape[0], nwaves)
    y[:rows] = emu_ln(x[:rows], gamma, beta, eps)[0]
    return y


def ln_fwd_waves(rows):
    """Waves of the forward LayerNorm kernels' grid: grid_for(rows, 4, 256 * 32) workgroups of 4 (core.hip)."""
    return min((rows + 3) // 4, 256 * 32) * 4


def emu_ln_bwd(x, dy, gamma, eps, order="lane"):
    """backward.hip row_grad in fp32 -> dx rows, per-row dgamma terms."""
    inv = torch.tensor(1.0 / LN_D, dtype=F32)
    v, d = _lanes(x), _lanes(dy.float())
    g = _lanes(gamma.expand(x.shape[0], LN_D).contiguous())
    mean = row_sum(v, order) * inv
    xc = v - mean[:, None, None]
    rstd = torch.rsqrt(row_sum(xc * xc, order) * inv + torch.tensor(eps, dtype=F32))
    xh = xc * rstd[:, None, None]
    ag = d * xh
    dg = d * g
    s1 = row_sum(dg, order) * inv
    s2 = row_sum(dg * xh, order) * inv
    fin = rstd[:, None, None] * (dg - s1[:, None, None] - xh * s2[:, None, None])
    return _unlanes(fin), _unlanes(ag)


# ------------------------------------------------------------------------------------------------ cross-entropy
XENT_REGIMES = ("gauss", "peaked", "late_max", "offset", "wide")
XENT_V = (2, 3, 64, 65, 511, 513, 1500, 1501, 3129, 30522)


def xent_inputs(M, V, regime, seed=0):
    """-> logits (M, V) fp32 on the 2^-8 grid (exact up to 3e4 + spread), labels (M,) int64.  Labels always include column 0 and V - 1."""
    g = _gen(4000 + seed + 7 * V + M)
    z = torch.randn(M, V, generator=g)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0] = V - 1
    if M > 1:
        labels[1] = 0
    rows = torch.arange(M)
    if regime == "gauss":
        x = z * 2
    elif regime == "peaked":       # one column 60 above the rest: the label in even rows, another column in the odd ones
        x = z * 2
        top = torch.where(rows % 2 == 0, labels, (labels + 1 + torch.randint(0, V - 1, (M,), generator=g)) % V)
        x[rows, top] = x.amax(-1) + 60
    elif regime == "late_max":     # the row maximum in the last column (the scalar tail when V is odd), 100 above the rest: a maximum that
        x = z * 2                  # missed it would overflow exp
        x[:, V - 1] = x.amax(-1) + 100
    elif regime == "offset":
        x = z * 2 + 3e4
    elif regime == "wide":         # spread +-80: most exp underflow; every third row has its label at the row minimum
        x = (torch.rand(M, V, generator=g) * 2 - 1) * 80
        x[rows, x.argmax(-1)] = 80.0
    else:
        raise ValueError(regime)
    x = on_grid(x, 2.0 ** -8)
    if regime == "wide":
        labels = torch.where(rows % 3 == 2, x.argmin(-1), labels)
    return x, labels


def xent_ref(logits, labels, ignore_index=-100):
    """fp64 -> loss_rows (0 for ignored rows), d loss_rows / d logits (softmax - onehot; 0 for ignored rows), number of valid rows."""
    x = logits.double()
    valid = labels != ignore_index
    lse = torch.logsumexp(x, -1)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    loss = torch.where(valid, lse - x.gather(1, lab[:, None]).squeeze(1), torch.zeros_like(lse))
    grad = torch.exp(x - lse[:, None])
    grad[torch.arange(x.shape[0]), lab] -= 1
    return loss, grad * valid[:, None].double(), int(valid.sum())


def xent_loss_extra(logits, c=XENT_C):
    return c * U24 * logits.double().abs().amax(-1)


def emu_xent(logits, labels, grad_scale, order="lane", fault=None):
    """loss.hip xent_kernel in fp32 (valid labels only): 256 threads, thread t reads the pairs at 2t + 512k, an odd row ends in a scalar
    tail.  -> loss_rows, gradient (M, V) fp32.  fault: 'no_max' (no maximum subtracted), 'max_pairs' (maximum over the paired part of an
    odd row only), 'label_off' (label column + 1)."""
    x = logits
    M, V = x.shape
    rows = torch.arange(M)
    if fault == "no_max":
        mx = torch.zeros(M)
    elif fault == "max_pairs" and V % 2 == 1 and V > 1:
        mx = x[:, :V - 1].amax(-1)
    else:
        mx = x.amax(-1)
    e = torch.exp(x - mx[:, None])
    if order == "lane":
        K = (V + 511) // 512
        ep = torch.zeros(M, K * 512)
        ep[:, :V] = e
        ep = ep.view(M, K, 256, 2)
        pair = ep[..., 0] + ep[..., 1]
        s = pair[:, 0].clone()
        for k in range(1, K):
            s = s + pair[:, k]
        w = wave_sum(s.view(M, 4, 64))
        s = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    else:
        s = e[:, 0].clone()
        for k in range(1, V):
            s = s + e[:, k]
    lse = mx + torch.log(s)
    lab = (labels + 1) % V if fault == "label_off" else labels
    loss = lse - x[rows, lab]
    grad = torch.exp(x - lse[:, None])
    grad[rows, lab] -= 1
    return loss, grad * torch.tensor(grad_scale, dtype=F32)


def grad_tol(dt):
    """(rtol, atol) of the xent gradient: the dtype's relative tolerance; absolute 1e-8 (fp32, the existing test's), 1e-7 (bf16, the existing
    test's), 2^-25 (fp16: half its smallest subnormal, the rounding step of the format near zero)."""
    from tests.test_hip_ops import OUT_TOL
    return OUT_TOL[dt][0], {torch.float32: 1e-8, torch.bfloat16: 1e-7, torch.float16: 2.0 ** -25}[dt]


def xent_grad_excess(got, ref_grad, scale, dt, logits):
    """got: the kernel's (M, V) gradient in dt; ref_grad fp64 unscaled.  The softmax is exp(x - lse): it inherits lse's absolute error --
    the loss allowance -- as a relative error of the softmax, which the label column's softmax - 1 does not shrink with; so that term
    enters as (loss allowance) * softmax * scale.  Past fp16's range both sides must agree on the infinity (an element within rtol of the
    largest finite value may fall either way)."""
    rtol, atol = grad_tol(dt)
    ref = ref_grad * scale
    got = got.detach().cpu().double()
    cond = (1e-5 + xent_loss_extra(logits))[:, None] * torch.softmax(logits.double(), -1) * abs(scale)
    if dt == torch.float16:
        big = ref.abs() >= 65504.0 * (1 - rtol)
        over = ref.abs() >= 65520.0 * (1 + rtol)
        if (over & ~(torch.isinf(got) & (torch.sign(got) == torch.sign(ref)))).any():
            return float("inf")
        got = torch.where(big & torch.isinf(got), ref, got)
        ref = torch.where(over, got, ref)
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref).abs() / (atol + rtol * ref.abs() + cond)).max())


# ------------------------------------------------------------------------------------------------ AdamW
ADAMW_S = 256 * 16 * 256 * 4   # elements one capped trip of adamw_kernel covers: optim.hip grid_for caps the grid at 256 * 16 workgroups of 256
                               # threads, one float4 each per chunk = 4 194 304
ADAMW_SMALL = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025)
ADAMW_BIG = (ADAMW_S - 1, ADAMW_S, ADAMW_S + 1, ADAMW_S + 5, 2 * ADAMW_S - 4, 2 * ADAMW_S, 2 * ADAMW_S + 1024 * 3 + 7, 3 * ADAMW_S - 1)


def adamw_inputs(n, seed=0):
    """p, g, m, v fp32 (n,): |g| log-uniform over 1e-6 .. 1e3, v log-uniform over 1e-30 .. 1e-1, every 11th element g = 0 and v = 0."""
    gen = _gen(5000 + seed + n % 9973)
    p = torch.randn(n, generator=gen)
    g = 10.0 ** (torch.rand(n, generator=gen) * 9 - 6) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    m = torch.randn(n, generator=gen) * 1e-3
    v = 10.0 ** (torch.rand(n, generator=gen) * 29 - 30)
    z = torch.arange(n) % 11 == 3
    return p, torch.where(z, torch.zeros(()), g), m, torch.where(z, torch.zeros(()), v)


def f32(x):
    """The value a C float argument takes."""
    return float(torch.tensor(x, dtype=F32))


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step_size, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, dyn=None, grads_scaled=True,
              correct_bias=True, dtype=F64, wd_first=False):
    """The reference optimizer's update (HF-style AdamW after clip_grad_norm_, as tests/test_hip_bwd_ops.py restates it) with the kernel's
    scalar plumbing, on the float values the kernel receives.  dtype F64: the reference; F32: the emulator's arithmetic."""
    lr, b1, b2, eps, wd, step_size, max_norm, grad_scale = (f32(a) for a in (lr, b1, b2, eps, wd, step_size, max_norm, grad_scale))
    coef = grad_scale
    if dyn is not None:
        if grads_scaled:
            coef = coef / float(dyn[0])
        t = float(dyn[2]) + 1.0
        step_size = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if correct_bias else lr
    if gnorm_sq is not None and max_norm > 0:
        coef = coef * min(max_norm / (math.sqrt(float(gnorm_sq)) * coef + f32(1e-6)), 1.0)
    T = lambda a: torch.tensor(a, dtype=dtype)  # noqa: E731
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    if wd_first and wd > 0:
        p = p - T(lr) * T(wd) * p
    gr = g * T(coef)
    m = m * T(b1) + (T(1.0) - T(b1)) * gr
    v = v * T(b2) + (T(1.0) - T(b2)) * gr * gr
    p = p - T(step_size) * (m / (v.sqrt() + T(eps)))
    if wd > 0 and not wd_first:
        p = p - T(lr) * T(wd) * p
    return p, m, v


def adamw_coverage(n, fault=None):
    """Which elements adamw_kernel's chunk walk updates (bool (n,)): thread t starts at 4t, takes two float4 chunks `stride` apart per trip
    and finishes ragged chunks element by element.  fault: 'drop_tail' (a chunk of fewer than 4 elements is left out), 'skip_second' (the
    finishing loop stops before the second chunk)."""
    grid = max(1, min((n // 4 + 255) // 256, 256 * 16))
    stride = grid * 256 * 4
    done = torch.zeros(n + 8, dtype=torch.bool)
    i = torch.arange(grid * 256, dtype=torch.int64) * 4

    def mark(q, cnt):
        for k in range(4):
            sel = q[cnt > k] + k
            assert not done[sel].any(), "an element is updated twice"
            done[sel] = True

    while bool((i < n).any()):
        i = i[i < n]
        j = i + stride
        full = j + 4 <= n
        mark(i[full], torch.full_like(i[full], 4))
        mark(j[full], torch.full_like(j[full], 4))
        qs = [i[~full]] if fault == "skip_second" else [i[~full], j[~full]]
        for q in qs:
            q = q[q < n]
            cnt = torch.clamp(n - q, max=4)
            if fault == "drop_tail":
                cnt = torch.where(cnt < 4, torch.zeros_like(cnt), cnt)
            mark(q, cnt)
        i = i + 2 * stride
    assert not done[n:].any()
    return done[:n]


def emu_adamw(p, g, m, v, *args, fault=None, **kw):
    """adamw_kernel in fp32: the update where the chunk walk reaches, the inputs elsewhere.  fault: adamw_coverage's, or 'wd_first'
    (weight decay applied before the moment update)."""
    pn, mn, vn = adamw_ref(p, g, m, v, *args, dtype=F32, wd_first=fault == "wd_first", **kw)
    done = adamw_coverage(p.numel(), fault if fault != "wd_first" else None)
    return torch.where(done, pn, p), torch.where(done, mn, m), torch.where(done, vn, v)


def adamw_excess(got, ref, inputs, b1=0.9, b2=0.98):
    """max err / allowed over p, m, v.  p: the existing test's (1e-5, 1e-6).  m, v: 1e-5 relative plus four fp32 roundings of the larger
    term of the moment's two-term sum (m' = b1 m + (1 - b1) g can cancel), which is what the format allows."""
    p0, g0, m0, v0 = (t.double() for t in inputs)
    worst = excess(got[0], ref[0], 1e-5, 1e-6)
    worst = max(worst, excess(got[1], ref[1], 1e-5, 1e-45, 4 * U24 * torch.maximum(m0.abs() * b1, (ref[1] - m0 * f32(b1)).abs())))
    return max(worst, excess(got[2], ref[2], 1e-5, 1e-45))
