// Gradient of a score w.r.t. the temporal attention probabilities of the visual encoder, and the Grad-CAM map built from it, materialised on
// request (TimeSformer.forward_features attn_grads; the reference reaches the same tensor with retain_grad() on the input of
// temporal_attn.attn_drop, vit.py:92-93 on the (b h w) t m view of vit.py:147).  For group g = rows g*T .. g*T + T - 1, all fp32, (rows / T, H, T, T):
//   G[g, h, q, k]   = grad_scale * <dctx[gT + q, h*64 : h*64 + 64], v[gT + k, h, :]>       d(score) / d(P), P the softmax BEFORE dropout
//   P[g, h, q, k]   = alpro_attn_temporal_probs' value: map_prob of the same s = acc * scale from the same map_tile (attn_map.hpp)
//   CAM[g, h, q, k] = P * max(G, 0)                                                        one fp32 multiply
// alpro_attn_temporal_bwd is flash-style: P and dP = dO V^T stay in registers; this is its sibling for the one caller that wants to SEE them.
//
// Form: attention_temporal_probs.hip's two forms (the item maps tp_items / tile coordinates are shared through attn_map.hpp), each with a
// second accumulator set: the v rows are the A operand and the dctx rows the B operand of G^T, beside the k and q rows of S^T, so both sets
// have the keys on the accumulator rows and registers 4g .. 4g + 3 are four consecutive keys of one query in either.  A null output is skipped
// behind a wave-uniform test; without cam_out neither the q / k thirds nor lse are read and S^T is not formed.  As in attention_probs_grad.hip
// the two outputs leave under ONE branch per register group, G in front of CAM.
#include "attn_map.hpp"

namespace alpro {
namespace {

// T divides 32; sh = log2 T.  items = units * H, unit-major (tprobs_unit_kernel's map).
template <typename T>
__global__ __launch_bounds__(MAP_THREADS) void tprobs_grad_unit_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx, const float* __restrict__ lse,
                                                                       float* __restrict__ grad_out, float* __restrict__ cam_out, int64_t rows, int sh, int H,
                                                                       float scale, float grad_scale, int64_t items) {
  constexpr int NCH = MAP_NCH<T>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
  const int64_t item = (int64_t)blockIdx.x * MAP_WAVES + wave;
  if (item >= items) return;                   // wave-uniform
  const int64_t u = item / H;
  const int h = (int)(item - u * H);
  const int Tn = 1 << sh;
  const int64_t ld = (int64_t)3 * H * 64;
  const bool want_cam = cam_out != nullptr, want_grad = grad_out != nullptr;   // wave-uniform (kernel arguments)
  const int64_t grow = u * 32 + l31;           // this lane's row: key / v row l31 of the A operands and query / dctx row l31 of the B operands
  const bool rok = grow < rows;                // (rows past the end repeat the last one and store nothing)
  const int64_t lrow = rok ? grow : rows - 1;
  u32x4 df[NCH], vf[NCH], qf[NCH], kf[NCH];
  map_load_row(df, dctx + lrow * ((int64_t)H * 64) + h * 64, hh);
  map_load_row(vf, qkv + lrow * ld + (2 * H + h) * 64, hh);
  f32x16 accg, accs = {};   // (defined on the path without cam_out too)
  float lq = 0.f;
  if (want_cam) {
    map_load_row(qf, qkv + lrow * ld + h * 64, hh);
    map_load_row(kf, qkv + lrow * ld + (H + h) * 64, hh);
    map_tile<T>(accs, kf, qf);
    lq = lse[(u * H + h) * 32 + (rok ? l31 : (int)(rows - 1 - u * 32))];
  }
  map_tile<T>(accg, vf, df);
  // register r: key (r & 3) + 8 (r >> 2) + 4 hh of the unit, query l31
  const int qg = l31 >> sh;                    // group of the query inside the unit
  const int64_t ooff = ((((u * 32) >> sh) + qg) * H + h) * ((int64_t)Tn * Tn) + (int64_t)(l31 & (Tn - 1)) * Tn;   // row start in either output
  if (sh >= 2) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = 8 * g + 4 * hh;
      if (rok && (kb >> sh) == qg) {
        float gr[4], cam[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gr[j] = accg[4 * g + j] * grad_scale;
        if (want_grad) *(f32x4*)(grad_out + ooff + (kb & (Tn - 1))) = f32x4{gr[0], gr[1], gr[2], gr[3]};
        if (want_cam) {
#pragma unroll
          for (int j = 0; j < 4; ++j) cam[j] = map_prob(accs[4 * g + j] * scale, lq) * fmaxf(gr[j], 0.f);
          *(f32x4*)(cam_out + ooff + (kb & (Tn - 1))) = f32x4{cam[0], cam[1], cam[2], cam[3]};
        }
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (rok && (kk >> sh) == qg) {
        const float gr = accg[r] * grad_scale;
        if (want_grad) grad_out[ooff + (kk & (Tn - 1))] = gr;
        if (want_cam) cam_out[ooff + (kk & (Tn - 1))] = map_prob(accs[r] * scale, lq) * fmaxf(gr, 0.f);
      }
    }
  }
}

// any T; nt = (T + 31) / 32 tiles per side.  items = groups * H * nt * nt, group-major, then head, query tile, key tile (tprobs_tile_kernel's map).
template <typename T>
__global__ __launch_bounds__(MAP_THREADS) void tprobs_grad_tile_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx, const float* __restrict__ lse,
                                                                       float* __restrict__ grad_out, float* __restrict__ cam_out, int Tn, int nt, int H,
                                                                       float scale, float grad_scale, int64_t items) {
  constexpr int NCH = MAP_NCH<T>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
  const int64_t item = (int64_t)blockIdx.x * MAP_WAVES + wave;
  if (item >= items) return;                   // wave-uniform
  const int kt = (int)(item % nt), qt = (int)((item / nt) % nt);
  const int64_t gh = item / (nt * nt);
  const int64_t grp = gh / H;
  const int h = (int)(gh - grp * H);
  const int64_t ld = (int64_t)3 * H * 64;
  const bool want_cam = cam_out != nullptr, want_grad = grad_out != nullptr;   // wave-uniform (kernel arguments)
  const int qi = qt * 32 + l31, kj = kt * 32 + l31;      // rows past T repeat the last one of the group and are masked at the store
  const int64_t qrow = grp * Tn + min(qi, Tn - 1), krow = grp * Tn + min(kj, Tn - 1);
  u32x4 df[NCH], vf[NCH], qf[NCH], kf[NCH];
  map_load_row(df, dctx + qrow * ((int64_t)H * 64) + h * 64, hh);
  map_load_row(vf, qkv + krow * ld + (2 * H + h) * 64, hh);
  f32x16 accg, accs = {};   // (defined on the path without cam_out too)
  float lq = 0.f;
  if (want_cam) {
    map_load_row(qf, qkv + qrow * ld + h * 64, hh);
    map_load_row(kf, qkv + krow * ld + (H + h) * 64, hh);
    map_tile<T>(accs, kf, qf);
    lq = lse[((qrow >> 5) * H + h) * 32 + (qrow & 31)];
  }
  map_tile<T>(accg, vf, df);
  const int64_t ooff = (gh * Tn + min(qi, Tn - 1)) * Tn;   // row start in either output
  const bool qok = qi < Tn;
  const bool full = (Tn & 3) == 0 && (kt + 1) * 32 <= Tn;   // wave-uniform; row starts of the outputs are 16-byte aligned
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int kb = kt * 32 + 8 * g + 4 * hh;
    float gr[4], cam[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gr[j] = accg[4 * g + j] * grad_scale;
    if (want_cam) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cam[j] = map_prob(accs[4 * g + j] * scale, lq) * fmaxf(gr[j], 0.f);
    }
    if (full) {
      if (qok && want_grad) *(f32x4*)(grad_out + ooff + kb) = f32x4{gr[0], gr[1], gr[2], gr[3]};
      if (qok && want_cam) *(f32x4*)(cam_out + ooff + kb) = f32x4{cam[0], cam[1], cam[2], cam[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (qok && kb + j < Tn && want_grad) grad_out[ooff + kb + j] = gr[j];
        if (qok && kb + j < Tn && want_cam) cam_out[ooff + kb + j] = cam[j];
      }
    }
  }
}

template <typename T>
int launch_tprobs_grad(const void* qkv, const void* dctx, const float* lse, float* grad_out, float* cam_out, int64_t rows, int Tn, int H, float scale,
                       float grad_scale, hipStream_t st) {
  const int64_t items = tp_items(rows, Tn, H);
  const dim3 grid((unsigned)((items + MAP_WAVES - 1) / MAP_WAVES));
  if (32 % Tn == 0) {
    int sh = 0;
    while ((1 << sh) < Tn) ++sh;
    hipLaunchKernelGGL((tprobs_grad_unit_kernel<T>), grid, dim3(MAP_THREADS), 0, st, (const T*)qkv, (const T*)dctx, lse, grad_out, cam_out, rows, sh, H, scale,
                       grad_scale, items);
  } else {
    hipLaunchKernelGGL((tprobs_grad_tile_kernel<T>), grid, dim3(MAP_THREADS), 0, st, (const T*)qkv, (const T*)dctx, lse, grad_out, cam_out, Tn, (Tn + 31) / 32, H,
                       scale, grad_scale, items);
  }
  return check_launch("alpro_attn_temporal_probs_grad");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_temporal_probs_grad(const void* qkv, const void* dctx, const float* lse, float* grad_out, float* cam_out, int dtype, int64_t rows,
                                              int T, int H, float scale, float grad_scale, void* stream) {
  if (int rc = map_temporal_check("alpro_attn_temporal_probs_grad", dtype, rows, T, H)) return rc;
  if (rows == 0) return ALPRO_OK;
  ALPRO_CHECK(qkv != nullptr, "alpro_attn_temporal_probs_grad: null qkv");
  ALPRO_CHECK(dctx != nullptr, "alpro_attn_temporal_probs_grad: null dctx");
  ALPRO_CHECK(lse != nullptr, "alpro_attn_temporal_probs_grad: null lse");
  ALPRO_CHECK(grad_out != nullptr || cam_out != nullptr, "alpro_attn_temporal_probs_grad: null grad_out and null cam_out (ask for at least one)");
  ALPRO_CHECK(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)dctx % 16) == 0 && ((uintptr_t)grad_out % 16) == 0 && ((uintptr_t)cam_out % 16) == 0,
              "alpro_attn_temporal_probs_grad: qkv, dctx, grad_out and cam_out must be 16-byte aligned");
  ALPRO_CHECK(((uintptr_t)lse % 4) == 0, "alpro_attn_temporal_probs_grad: lse must be 4-byte aligned");
  ALPRO_DISPATCH_DTYPE(dtype, T_, return launch_tprobs_grad<T_>(qkv, dctx, lse, grad_out, cam_out, rows, T, H, scale, grad_scale, (hipStream_t)stream));
  return ALPRO_OK;
}
