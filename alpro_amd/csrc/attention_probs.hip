// Attention probabilities of the text / fusion encoder, materialised on request (BertModel.forward output_attentions; xbert.py:323,343 returns
// the softmax of every layer): P[b, h, q, k] = exp(scale * <q_bhq, k_bhk> + key_bias[b, k] - lse[b, h, q]) for a window q0 <= q < q0 + nq,
// k0 <= k < k0 + nk of the (L, L) map, fp32.  alpro_attn_fwd and the long path are flash-style and never hold P; they leave lse (batch, H, L),
// the natural-log normaliser over ALL L keys, so a window is a slice of the full map, not a renormalised one.  Pre-dropout probabilities.
//
// One pass, no K / V residency, no LDS: a workgroup (4 waves) owns one (sequence, head, 32-query tile of the window).  Every wave keeps the
// tile's 32 query rows in registers as MFMA operands (lane l: row l & 31, the 16-byte chunks of k-slice l >> 5) and walks the window's 32-key
// tiles wave-interleaved; the key rows come straight from global memory in the same chunk order.
//
// Orientation: the wave forms S^T -- keys are the A operand, queries the B operand.  In the 32x32 accumulator a lane holds ONE column (l & 31)
// and the rows (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r, so with keys on the rows the registers 4g .. 4g + 3 of a lane are four
// CONSECUTIVE keys of one query: one 16-byte store along k per register group when the tile is full and nk is a multiple of 4 (the row starts
// of `out` are then 16-byte aligned); lane halves write adjacent 16-byte pieces.  S (queries on the rows) would put consecutive keys on
// consecutive lanes: 4-byte stores.  Ragged tiles (the last key tile, nk not a multiple of 4, query rows past nq) take masked 4-byte stores.
//
// 16-bit operands: v_mfma_f32_32x32x16_{bf16,f16}; fp32 (exact mode): v_mfma_f32_32x32x2_f32, exact products, fp32 accumulation.
// s = fma(acc, scale, bias) is ONE fp32 rounding; a = min(s - lse, 0) and p = min(exp2(a * log2 e), 1): the exponential only ever sees a
// non-positive argument (s - lse <= 0 up to the rounding of s and of lse), so p <= 1 and never inf / NaN for finite inputs.
// No atomics, no workspace, no scratch; every output element has exactly one writer and a fixed arithmetic order: bitwise reproducible.
#include <limits.h>

#include "common.hpp"

namespace alpro {
namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_TILE = 32;   // queries per workgroup, keys per wave step

template <typename T, bool HAS_BIAS>
__global__ __launch_bounds__(AP_THREADS) void attn_probs_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                                const float* __restrict__ key_bias, float* __restrict__ out, int L, int H,
                                                                float scale, int q0, int nq, int k0, int nk, int nqt) {
  constexpr int NCH = 64 / Chunk<T>::N / 2;   // 16-byte chunks of a 64-wide head row per lane: 4 (16-bit), 8 (fp32)
  constexpr float LOG2E = 1.4426950408889634f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int b = bh / H, h = bh - b * H;
  const int64_t ld = (int64_t)3 * H * 64;
  const int qi = qt * AP_TILE + l31;               // query of this lane, relative to the window; rows past nq repeat the last one and store nothing
  const int qrow = q0 + min(qi, nq - 1);
  const u32x4* qp = (const u32x4*)(qkv + ((int64_t)b * L + qrow) * ld + h * 64);
  u32x4 qf[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) qf[i] = qp[2 * i + hh];
  const float lq = lse[((int64_t)b * H + h) * L + qrow];
  float* orow = out + ((int64_t)bh * nq + min(qi, nq - 1)) * nk;
  const bool qok = qi < nq;
  const bool vec = (nk & 3) == 0;                  // row starts of `out` are 16-byte aligned
  const float* kbp = HAS_BIAS ? key_bias + (int64_t)b * L + k0 : nullptr;
  const int nkt = (nk + AP_TILE - 1) / AP_TILE;
  for (int kt = wave; kt < nkt; kt += AP_THREADS / 64) {
    const int kj = min(kt * AP_TILE + l31, nk - 1);   // keys past nk repeat the last one; masked at the store
    const u32x4* kp = (const u32x4*)(qkv + ((int64_t)b * L + k0 + kj) * ld + (H + h) * 64);
    u32x4 kf[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) kf[i] = kp[2 * i + hh];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) mma_chunk<T>(acc, kf[i], qf[i]);
    // register r: key kt * 32 + (r & 3) + 8 (r >> 2) + 4 hh of the window, query l31 of the tile
    const bool full = vec && (kt + 1) * AP_TILE <= nk;   // wave-uniform
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = kt * AP_TILE + 8 * g + 4 * hh;
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bias = HAS_BIAS ? kbp[min(kb + j, nk - 1)] : 0.f;
        const float a = fminf(fmaf(acc[4 * g + j], scale, bias) - lq, 0.f);
        p[j] = fminf(__builtin_amdgcn_exp2f(a * LOG2E), 1.f);
      }
      if (full) {
        if (qok) *(f32x4*)(orow + kb) = f32x4{p[0], p[1], p[2], p[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (qok && kb + j < nk) orow[kb + j] = p[j];
      }
    }
  }
}

template <typename T>
int launch_probs(const void* qkv, const float* lse, const float* key_bias, float* out, int batch, int L, int H, float scale, int q0, int nq, int k0,
                 int nk, hipStream_t st) {
  const int nqt = (nq + AP_TILE - 1) / AP_TILE;
  const dim3 grid((unsigned)(batch * H * nqt));
  if (key_bias)
    hipLaunchKernelGGL((attn_probs_kernel<T, true>), grid, dim3(AP_THREADS), 0, st, (const T*)qkv, lse, key_bias, out, L, H, scale, q0, nq, k0, nk, nqt);
  else
    hipLaunchKernelGGL((attn_probs_kernel<T, false>), grid, dim3(AP_THREADS), 0, st, (const T*)qkv, lse, key_bias, out, L, H, scale, q0, nq, k0, nk, nqt);
  return check_launch("alpro_attn_probs");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_probs(const void* qkv, const float* lse, const float* key_bias, float* out, int dtype, int batch, int L, int H, float scale,
                                int q0, int nq, int k0, int nk, void* stream) {
  // every check in front of the first HIP call: the refusals are testable without a device
  ALPRO_CHECK(dtype == ALPRO_F32 || dtype == ALPRO_BF16 || dtype == ALPRO_F16, "alpro_attn_probs: dtype=%d (ALPRO_F32, ALPRO_BF16 or ALPRO_F16)", dtype);
  ALPRO_CHECK(L >= 1 && L <= ALPRO_ATTN_MAX_L, "alpro_attn_probs: L=%d unsupported (1..%d = ALPRO_ATTN_MAX_L)", L, ALPRO_ATTN_MAX_L);
  ALPRO_CHECK(batch >= 1 && H >= 1, "alpro_attn_probs: batch=%d H=%d (need >= 1)", batch, H);
  ALPRO_CHECK(q0 >= 0 && nq >= 1 && nq <= L - q0, "alpro_attn_probs: query window q0=%d nq=%d outside 0 <= q0, 1 <= nq, q0 + nq <= L=%d", q0, nq, L);
  ALPRO_CHECK(k0 >= 0 && nk >= 1 && nk <= L - k0, "alpro_attn_probs: key window k0=%d nk=%d outside 0 <= k0, 1 <= nk, k0 + nk <= L=%d", k0, nk, L);
  ALPRO_CHECK((int64_t)batch * H * ((nq + AP_TILE - 1) / AP_TILE) <= INT_MAX, "alpro_attn_probs: batch=%d x H=%d x nq=%d needs more than 2^31 - 1 workgroups",
              batch, H, nq);
  ALPRO_CHECK(qkv != nullptr, "alpro_attn_probs: null qkv");
  ALPRO_CHECK(lse != nullptr, "alpro_attn_probs: null lse");
  ALPRO_CHECK(out != nullptr, "alpro_attn_probs: null out");
  ALPRO_CHECK(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0, "alpro_attn_probs: qkv and out must be 16-byte aligned");
  ALPRO_CHECK(((uintptr_t)lse % 4) == 0 && ((uintptr_t)key_bias % 4) == 0, "alpro_attn_probs: lse and key_bias must be 4-byte aligned");
  ALPRO_DISPATCH_DTYPE(dtype, T, return launch_probs<T>(qkv, lse, key_bias, out, batch, L, H, scale, q0, nq, k0, nk, (hipStream_t)stream));
  return ALPRO_OK;
}
