// Gradient of a score w.r.t. the attention probabilities of the text / fusion encoder, and the Grad-CAM map built from it, materialised on
// request (BertModel.forward attn_grads; the reference reaches the same tensor with a register_hook on attention_probs, xbert.py:325-327):
//   G[b, h, q, k]   = grad_scale * <dctx[b*L + q, h*64 : h*64 + 64], v[b*L + k, h, :]>     d(score) / d(P), P the softmax BEFORE dropout, eval mode
//   P[b, h, q, k]   = alpro_attn_probs' value, same arithmetic in the same order (attention_probs.hip)
//   CAM[b, h, q, k] = P * max(G, 0)                                                        one fp32 multiply
// for a window q0 <= q < q0 + nq, k0 <= k < k0 + nk of the (L, L) map, fp32.  alpro_attn_bwd is flash-style: it recomputes P tile by tile and
// forms dP = dO V^T in registers, neither ever reaches memory; this is its sibling for the one caller that wants to SEE them.
//
// Form: attention_probs.hip with a second product.  A workgroup (4 waves) owns one (sequence, head, 32-query tile of the window); every wave
// keeps the tile's 32 q rows AND its 32 dctx rows in registers as B operands (lane l: row l & 31, the 16-byte chunks of k-slice l >> 5) and
// walks the window's 32-key tiles wave-interleaved; per key tile the k rows and the v rows come straight from global memory as A operands and
// feed two accumulator sets, S^T and G^T.  Same orientation as attention_probs.hip: registers 4g .. 4g + 3 of a lane are four CONSECUTIVE keys
// of one query, so each output leaves as one 16-byte store per register group when the tile is full and nk is a multiple of 4, and as masked
// 4-byte stores otherwise.  A null output (grad_out or cam_out) is skipped behind a wave-uniform test; without cam_out S^T is not formed at all.
//
// 16-bit operands: v_mfma_f32_32x32x16_{bf16,f16}; fp32 (exact mode): v_mfma_f32_32x32x2_f32, exact products, fp32 accumulation.
// A masked key has P ~ 0 and G whatever the dot product gives, as on the reference's hook.  No LDS, no workspace, no atomics, no scratch; every
// output element has exactly one writer and a fixed arithmetic order: bitwise reproducible.
#include <limits.h>

#include "common.hpp"

namespace alpro {
namespace {

constexpr int APG_THREADS = 256;
constexpr int APG_TILE = 32;   // queries per workgroup, keys per wave step

template <typename T, bool HAS_BIAS>
__global__ __launch_bounds__(APG_THREADS) void attn_probs_grad_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx, const float* __restrict__ lse,
                                                                      const float* __restrict__ key_bias, float* __restrict__ grad_out,
                                                                      float* __restrict__ cam_out, int L, int H, float scale, float grad_scale, int q0,
                                                                      int nq, int k0, int nk, int nqt) {
  constexpr int NCH = 64 / Chunk<T>::N / 2;   // 16-byte chunks of a 64-wide head row per lane: 4 (16-bit), 8 (fp32)
  constexpr float LOG2E = 1.4426950408889634f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int b = bh / H, h = bh - b * H;
  const int64_t ld = (int64_t)3 * H * 64;
  const bool want_cam = cam_out != nullptr, want_grad = grad_out != nullptr;   // wave-uniform (kernel arguments)
  const int qi = qt * APG_TILE + l31;              // query of this lane, relative to the window; rows past nq repeat the last one and store nothing
  const int qrow = q0 + min(qi, nq - 1);
  const u32x4* dp = (const u32x4*)(dctx + ((int64_t)b * L + qrow) * ((int64_t)H * 64) + h * 64);
  u32x4 df[NCH], qf[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) df[i] = dp[2 * i + hh];
  float lq = 0.f;
  if (want_cam) {
    const u32x4* qp = (const u32x4*)(qkv + ((int64_t)b * L + qrow) * ld + h * 64);
#pragma unroll
    for (int i = 0; i < NCH; ++i) qf[i] = qp[2 * i + hh];
    lq = lse[((int64_t)b * H + h) * L + qrow];
  }
  const int64_t ooff = ((int64_t)bh * nq + min(qi, nq - 1)) * nk;   // row start in either output
  const bool qok = qi < nq;
  const bool vec = (nk & 3) == 0;                  // row starts of the outputs are 16-byte aligned
  const float* kbp = HAS_BIAS ? key_bias + (int64_t)b * L + k0 : nullptr;
  const int nkt = (nk + APG_TILE - 1) / APG_TILE;
  for (int kt = wave; kt < nkt; kt += APG_THREADS / 64) {
    const int kj = min(kt * APG_TILE + l31, nk - 1);   // keys past nk repeat the last one; masked at the store
    const T* krow = qkv + ((int64_t)b * L + k0 + kj) * ld + (H + h) * 64;
    const u32x4* vp = (const u32x4*)(krow + (int64_t)H * 64);
    u32x4 vf[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) vf[i] = vp[2 * i + hh];
    f32x16 accg, accs;
#pragma unroll
    for (int r = 0; r < 16; ++r) accg[r] = accs[r] = 0.f;
    if (want_cam) {
      const u32x4* kp = (const u32x4*)krow;
      u32x4 kf[NCH];
#pragma unroll
      for (int i = 0; i < NCH; ++i) kf[i] = kp[2 * i + hh];
#pragma unroll
      for (int i = 0; i < NCH; ++i) mma_chunk<T>(accs, kf[i], qf[i]);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) mma_chunk<T>(accg, vf[i], df[i]);
    // register r: key kt * 32 + (r & 3) + 8 (r >> 2) + 4 hh of the window, query l31 of the tile
    const bool full = vec && (kt + 1) * APG_TILE <= nk;   // wave-uniform
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = kt * APG_TILE + 8 * g + 4 * hh;
      float gr[4], cam[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) gr[j] = accg[4 * g + j] * grad_scale;
      if (want_cam) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bias = HAS_BIAS ? kbp[min(kb + j, nk - 1)] : 0.f;
          const float a = fminf(fmaf(accs[4 * g + j], scale, bias) - lq, 0.f);
          const float p = fminf(__builtin_amdgcn_exp2f(a * LOG2E), 1.f);
          cam[j] = p * fmaxf(gr[j], 0.f);
        }
      }
      if (full) {
        if (qok && want_grad) *(f32x4*)(grad_out + ooff + kb) = f32x4{gr[0], gr[1], gr[2], gr[3]};
        if (qok && want_cam) *(f32x4*)(cam_out + ooff + kb) = f32x4{cam[0], cam[1], cam[2], cam[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (qok && kb + j < nk && want_grad) grad_out[ooff + kb + j] = gr[j];
          if (qok && kb + j < nk && want_cam) cam_out[ooff + kb + j] = cam[j];
        }
      }
    }
  }
}

template <typename T>
int launch_probs_grad(const void* qkv, const void* dctx, const float* lse, const float* key_bias, float* grad_out, float* cam_out, int batch, int L, int H,
                      float scale, float grad_scale, int q0, int nq, int k0, int nk, hipStream_t st) {
  const int nqt = (nq + APG_TILE - 1) / APG_TILE;
  const dim3 grid((unsigned)(batch * H * nqt));
  if (key_bias)
    hipLaunchKernelGGL((attn_probs_grad_kernel<T, true>), grid, dim3(APG_THREADS), 0, st, (const T*)qkv, (const T*)dctx, lse, key_bias, grad_out, cam_out, L, H,
                       scale, grad_scale, q0, nq, k0, nk, nqt);
  else
    hipLaunchKernelGGL((attn_probs_grad_kernel<T, false>), grid, dim3(APG_THREADS), 0, st, (const T*)qkv, (const T*)dctx, lse, key_bias, grad_out, cam_out, L, H,
                       scale, grad_scale, q0, nq, k0, nk, nqt);
  return check_launch("alpro_attn_probs_grad");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_probs_grad(const void* qkv, const void* dctx, const float* lse, const float* key_bias, float* grad_out, float* cam_out, int dtype,
                                     int batch, int L, int H, float scale, float grad_scale, int q0, int nq, int k0, int nk, void* stream) {
  // every check in front of the first HIP call: the refusals are testable without a device
  ALPRO_CHECK(dtype == ALPRO_F32 || dtype == ALPRO_BF16 || dtype == ALPRO_F16, "alpro_attn_probs_grad: dtype=%d (ALPRO_F32, ALPRO_BF16 or ALPRO_F16)", dtype);
  ALPRO_CHECK(L >= 1 && L <= ALPRO_ATTN_MAX_L, "alpro_attn_probs_grad: L=%d unsupported (1..%d = ALPRO_ATTN_MAX_L)", L, ALPRO_ATTN_MAX_L);
  ALPRO_CHECK(batch >= 1 && H >= 1, "alpro_attn_probs_grad: batch=%d H=%d (need >= 1)", batch, H);
  ALPRO_CHECK(q0 >= 0 && nq >= 1 && nq <= L - q0, "alpro_attn_probs_grad: query window q0=%d nq=%d outside 0 <= q0, 1 <= nq, q0 + nq <= L=%d", q0, nq, L);
  ALPRO_CHECK(k0 >= 0 && nk >= 1 && nk <= L - k0, "alpro_attn_probs_grad: key window k0=%d nk=%d outside 0 <= k0, 1 <= nk, k0 + nk <= L=%d", k0, nk, L);
  ALPRO_CHECK((int64_t)batch * H * ((nq + APG_TILE - 1) / APG_TILE) <= INT_MAX,
              "alpro_attn_probs_grad: batch=%d x H=%d x nq=%d needs more than 2^31 - 1 workgroups", batch, H, nq);
  ALPRO_CHECK(qkv != nullptr, "alpro_attn_probs_grad: null qkv");
  ALPRO_CHECK(dctx != nullptr, "alpro_attn_probs_grad: null dctx");
  ALPRO_CHECK(lse != nullptr, "alpro_attn_probs_grad: null lse");
  ALPRO_CHECK(grad_out != nullptr || cam_out != nullptr, "alpro_attn_probs_grad: null grad_out and null cam_out (ask for at least one)");
  ALPRO_CHECK(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)dctx % 16) == 0 && ((uintptr_t)grad_out % 16) == 0 && ((uintptr_t)cam_out % 16) == 0,
              "alpro_attn_probs_grad: qkv, dctx, grad_out and cam_out must be 16-byte aligned");
  ALPRO_CHECK(((uintptr_t)lse % 4) == 0 && ((uintptr_t)key_bias % 4) == 0, "alpro_attn_probs_grad: lse and key_bias must be 4-byte aligned");
  ALPRO_DISPATCH_DTYPE(dtype, T,
                       return launch_probs_grad<T>(qkv, dctx, lse, key_bias, grad_out, cam_out, batch, L, H, scale, grad_scale, q0, nq, k0, nk, (hipStream_t)stream));
  return ALPRO_OK;
}
