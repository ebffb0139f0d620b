// Gradient of a score w.r.t. the attention probabilities of the text / fusion encoder, and the Grad-CAM map built from it, materialised on
// request (BertModel.forward attn_grads; the reference reaches the same tensor with a register_hook on attention_probs, xbert.py:325-327):
//   G[b, h, q, k]   = grad_scale * <dctx[b*L + q, h*64 : h*64 + 64], v[b*L + k, h, :]>     d(score) / d(P), P the softmax BEFORE dropout, eval mode
//   P[b, h, q, k]   = alpro_attn_probs' value: map_prob of the same s = fma(acc, scale, bias) from the same map_tile (attn_map.hpp)
//   CAM[b, h, q, k] = P * max(G, 0)                                                        one fp32 multiply
// for a window q0 <= q < q0 + nq, k0 <= k < k0 + nk of the (L, L) map, fp32.  alpro_attn_bwd is flash-style: it recomputes P tile by tile and
// forms dP = dO V^T in registers, neither ever reaches memory; this is its sibling for the one caller that wants to SEE them.
//
// Form: attention_probs.hip with a second product (layout and orientation: attn_map.hpp).  Every wave keeps the tile's 32 q rows AND its 32 dctx
// rows in registers as B operands; per key tile the k rows and the v rows come straight from global memory as A operands and feed two
// accumulator sets, S^T and G^T.  A null output (grad_out or cam_out) is skipped behind a wave-uniform test; without cam_out S^T is not formed at
// all.  The two outputs leave under ONE branch on the full-tile test, G in front of CAM (two calls of map_store4 -- two branches per register
// group -- measured slower in the fp32 instantiation).  A masked key has P ~ 0 and G whatever the dot product gives, as on the reference's hook.
#include "attn_map.hpp"

namespace alpro {
namespace {

template <typename T, bool HAS_BIAS>
__global__ __launch_bounds__(MAP_THREADS) void attn_probs_grad_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx, const float* __restrict__ lse,
                                                                      const float* __restrict__ key_bias, float* __restrict__ grad_out,
                                                                      float* __restrict__ cam_out, int L, int H, float scale, float grad_scale, int q0,
                                                                      int nq, int k0, int nk, int nqt) {
  constexpr int NCH = MAP_NCH<T>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int b = bh / H, h = bh - b * H;
  const int64_t ld = (int64_t)3 * H * 64;
  const bool want_cam = cam_out != nullptr, want_grad = grad_out != nullptr;   // wave-uniform (kernel arguments)
  const int qi = qt * MAP_TILE + l31;              // query of this lane, relative to the window; rows past nq repeat the last one and store nothing
  const int qrow = q0 + min(qi, nq - 1);
  u32x4 df[NCH], qf[NCH];
  map_load_row(df, dctx + ((int64_t)b * L + qrow) * ((int64_t)H * 64) + h * 64, hh);
  float lq = 0.f;
  if (want_cam) {
    map_load_row(qf, qkv + ((int64_t)b * L + qrow) * ld + h * 64, hh);
    lq = lse[((int64_t)b * H + h) * L + qrow];
  }
  const int64_t ooff = ((int64_t)bh * nq + min(qi, nq - 1)) * nk;   // row start in either output
  const bool qok = qi < nq;
  const bool vec = (nk & 3) == 0;                  // row starts of the outputs are 16-byte aligned
  const float* kbp = HAS_BIAS ? key_bias + (int64_t)b * L + k0 : nullptr;
  const int nkt = (nk + MAP_TILE - 1) / MAP_TILE;
  for (int kt = wave; kt < nkt; kt += MAP_WAVES) {
    const int kj = min(kt * MAP_TILE + l31, nk - 1);   // keys past nk repeat the last one; masked at the store
    const T* krow = qkv + ((int64_t)b * L + k0 + kj) * ld + (H + h) * 64;
    u32x4 vf[NCH], kf[NCH];
    map_load_row(vf, krow + (int64_t)H * 64, hh);
    f32x16 accg, accs = {};   // (defined on the path without cam_out too)
    if (want_cam) {
      map_load_row(kf, krow, hh);
      map_tile<T>(accs, kf, qf);
    }
    map_tile<T>(accg, vf, df);
    // register r: key kt * 32 + (r & 3) + 8 (r >> 2) + 4 hh of the window, query l31 of the tile
    const bool full = vec && (kt + 1) * MAP_TILE <= nk;   // wave-uniform
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = kt * MAP_TILE + 8 * g + 4 * hh;
      float gr[4], cam[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) gr[j] = accg[4 * g + j] * grad_scale;
      if (want_cam) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bias = HAS_BIAS ? kbp[min(kb + j, nk - 1)] : 0.f;
          cam[j] = map_prob(fmaf(accs[4 * g + j], scale, bias), lq) * fmaxf(gr[j], 0.f);
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
  const int nqt = (nq + MAP_TILE - 1) / MAP_TILE;
  auto kernel = key_bias ? attn_probs_grad_kernel<T, true> : attn_probs_grad_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(batch * H * nqt)), dim3(MAP_THREADS), 0, st, (const T*)qkv, (const T*)dctx, lse, key_bias, grad_out, cam_out, L, H,
                     scale, grad_scale, q0, nq, k0, nk, nqt);
  return check_launch("alpro_attn_probs_grad");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_probs_grad(const void* qkv, const void* dctx, const float* lse, const float* key_bias, float* grad_out, float* cam_out, int dtype,
                                     int batch, int L, int H, float scale, float grad_scale, int q0, int nq, int k0, int nk, void* stream) {
  if (int rc = map_window_check("alpro_attn_probs_grad", true, dtype, batch, L, H, q0, nq, k0, nk, qkv, dctx, lse, key_bias, grad_out, cam_out)) return rc;
  ALPRO_DISPATCH_DTYPE(dtype, T,
                       return launch_probs_grad<T>(qkv, dctx, lse, key_bias, grad_out, cam_out, batch, L, H, scale, grad_scale, q0, nq, k0, nk, (hipStream_t)stream));
  return ALPRO_OK;
}
