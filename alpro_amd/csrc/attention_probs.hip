// Attention probabilities of the text / fusion encoder, materialised on request (BertModel.forward output_attentions; xbert.py:323,343 returns
// the softmax of every layer): P[b, h, q, k] = exp(scale * <q_bhq, k_bhk> + key_bias[b, k] - lse[b, h, q]) for a window q0 <= q < q0 + nq,
// k0 <= k < k0 + nk of the (L, L) map, fp32 (layout, orientation and the probability: attn_map.hpp).  lse (batch, H, L) is over ALL L keys, so a
// window is a slice of the full map, not a renormalised one.  s = fma(acc, scale, bias) is ONE fp32 rounding.
//
// A workgroup (4 waves) owns one (sequence, head, 32-query tile of the window).  Every wave keeps the tile's 32 query rows in registers as the B
// operand and walks the window's 32-key tiles wave-interleaved; the key rows come straight from global memory as the A operand.
#include "attn_map.hpp"

namespace alpro {
namespace {

template <typename T, bool HAS_BIAS>
__global__ __launch_bounds__(MAP_THREADS) void attn_probs_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                                 const float* __restrict__ key_bias, float* __restrict__ out, int L, int H,
                                                                 float scale, int q0, int nq, int k0, int nk, int nqt) {
  constexpr int NCH = MAP_NCH<T>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int b = bh / H, h = bh - b * H;
  const int64_t ld = (int64_t)3 * H * 64;
  const int qi = qt * MAP_TILE + l31;              // query of this lane, relative to the window; rows past nq repeat the last one and store nothing
  const int qrow = q0 + min(qi, nq - 1);
  u32x4 qf[NCH];
  map_load_row(qf, qkv + ((int64_t)b * L + qrow) * ld + h * 64, hh);
  const float lq = lse[((int64_t)b * H + h) * L + qrow];
  float* orow = out + ((int64_t)bh * nq + min(qi, nq - 1)) * nk;
  const bool qok = qi < nq;
  const bool vec = (nk & 3) == 0;                  // row starts of `out` are 16-byte aligned
  const float* kbp = HAS_BIAS ? key_bias + (int64_t)b * L + k0 : nullptr;
  const int nkt = (nk + MAP_TILE - 1) / MAP_TILE;
  for (int kt = wave; kt < nkt; kt += MAP_WAVES) {
    const int kj = min(kt * MAP_TILE + l31, nk - 1);   // keys past nk repeat the last one; masked at the store
    u32x4 kf[NCH];
    map_load_row(kf, qkv + ((int64_t)b * L + k0 + kj) * ld + (H + h) * 64, hh);
    f32x16 acc;
    map_tile<T>(acc, kf, qf);
    // register r: key kt * 32 + (r & 3) + 8 (r >> 2) + 4 hh of the window, query l31 of the tile
    const bool full = vec && (kt + 1) * MAP_TILE <= nk;   // wave-uniform
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = kt * MAP_TILE + 8 * g + 4 * hh;
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = map_prob(fmaf(acc[4 * g + j], scale, HAS_BIAS ? kbp[min(kb + j, nk - 1)] : 0.f), lq);
      map_store4(orow, p, qok, kb, nk, full);
    }
  }
}

template <typename T>
int launch_probs(const void* qkv, const float* lse, const float* key_bias, float* out, int batch, int L, int H, float scale, int q0, int nq, int k0,
                 int nk, hipStream_t st) {
  const int nqt = (nq + MAP_TILE - 1) / MAP_TILE;
  auto kernel = key_bias ? attn_probs_kernel<T, true> : attn_probs_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(batch * H * nqt)), dim3(MAP_THREADS), 0, st, (const T*)qkv, lse, key_bias, out, L, H, scale, q0, nq, k0, nk, nqt);
  return check_launch("alpro_attn_probs");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_probs(const void* qkv, const float* lse, const float* key_bias, float* out, int dtype, int batch, int L, int H, float scale,
                                int q0, int nq, int k0, int nk, void* stream) {
  if (int rc = map_window_check("alpro_attn_probs", false, dtype, batch, L, H, q0, nq, k0, nk, qkv, nullptr, lse, key_bias, out, nullptr)) return rc;
  ALPRO_DISPATCH_DTYPE(dtype, T, return launch_probs<T>(qkv, lse, key_bias, out, batch, L, H, scale, q0, nq, k0, nk, (hipStream_t)stream));
  return ALPRO_OK;
}
