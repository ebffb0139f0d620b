// What the kernels that MATERIALISE attention maps share (attention_probs.hip: text / fusion maps; attention_probs_grad.hip: their gradient and Grad-CAM;
// attention_temporal_probs.hip: the visual encoder's temporal maps; attention_temporal_probs_grad.hip: their gradient and Grad-CAM).  The forward / backward kernels are flash-style and never hold P; they leave
// lse, the natural-log normaliser over all keys of a row, so a map is p = exp(s - lse) of a score s recomputed here -- pre-dropout probabilities.
//
// Layout: no LDS, no K / V residency.  Every operand is a 64-wide head row straight from global memory as MFMA operand chunks: lane l holds row
// l & 31 and the 16-byte chunks of k-slice hh = l >> 5 (map_load_row).  16-bit operands: v_mfma_f32_32x32x16_{bf16,f16}; fp32 (exact mode):
// v_mfma_f32_32x32x2_f32, exact products, fp32 accumulation.
//
// Orientation: a wave forms S^T -- keys are the A operand, queries the B operand (map_tile).  In the 32x32 accumulator a lane holds ONE column
// (l & 31) and the rows (r & 3) + 8 (r >> 2) + 4 hh in register r, so with keys on the rows the registers 4g .. 4g + 3 of a lane are four
// CONSECUTIVE keys of one query: one 16-byte store along k per register group when the tile is full and the row length is a multiple of 4 (the
// row starts of the output are then 16-byte aligned); lane halves write adjacent 16-byte pieces.  S (queries on the rows) would put consecutive
// keys on consecutive lanes: 4-byte stores.  Ragged tiles (the last key tile, a row length that is no multiple of 4) take masked 4-byte stores
// (map_store4).
//
// p = min(exp2(min(s - lse, 0) * log2 e), 1) (map_prob): the exponential only ever sees a non-positive argument (s - lse <= 0 up to the rounding
// of s and of lse), so p <= 1 and never inf / NaN for finite inputs.  No atomics, no workspace, no scratch; every output element has exactly one
// writer and a fixed arithmetic order: bitwise reproducible.
#pragma once
#include <limits.h>

#include "common.hpp"

namespace alpro {

constexpr int MAP_THREADS = 256;
constexpr int MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_TILE = 32;   // queries and keys of one MFMA tile
template <typename T> constexpr int MAP_NCH = 64 / Chunk<T>::N / 2;   // 16-byte chunks of a 64-wide head row per lane: 4 (16-bit), 8 (fp32)

template <typename T> __device__ __forceinline__ void map_load_row(u32x4 (&f)[MAP_NCH<T>], const T* row, int hh) {
#pragma unroll
  for (int i = 0; i < MAP_NCH<T>; ++i) f[i] = ((const u32x4*)row)[2 * i + hh];
}

// acc = A B^T of two 32-row operands: register r of lane l is A's row (r & 3) + 8 (r >> 2) + 4 (l >> 5) against B's row l & 31
template <typename T> __device__ __forceinline__ void map_tile(f32x16& acc, const u32x4 (&a)[MAP_NCH<T>], const u32x4 (&b)[MAP_NCH<T>]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int i = 0; i < MAP_NCH<T>; ++i) mma_chunk<T>(acc, a[i], b[i]);
}

// THE probability of a score s (formed by the caller, one fp32 rounding) under the row's normaliser
__device__ __forceinline__ float map_prob(float s, float lse) {
  return fminf(__builtin_amdgcn_exp2f(fminf(s - lse, 0.f) * 1.4426950408889634f), 1.f);
}

// four consecutive keys kb .. kb + 3 of a row of n keys; ok: this lane's row exists; full (wave-uniform): the whole tile is inside the row and
// the row is 16-byte aligned
__device__ __forceinline__ void map_store4(float* row, const float (&v)[4], bool ok, int kb, int n, bool full) {
  if (full) {
    if (ok) *(f32x4*)(row + kb) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok && kb + j < n) row[kb + j] = v[j];
  }
}

// The argument checks of the windowed entry points (fn: the one that was called; grad: alpro_attn_probs_grad, with dctx and two optional
// outputs).  Host only, no HIP call: the refusals are testable without a device.
inline int map_window_check(const char* fn, bool grad, int dtype, int batch, int L, int H, int q0, int nq, int k0, int nk, const void* qkv, const void* dctx,
                            const float* lse, const float* key_bias, const float* out, const float* cam_out) {
  ALPRO_CHECK(dtype == ALPRO_F32 || dtype == ALPRO_BF16 || dtype == ALPRO_F16, "%s: dtype=%d (ALPRO_F32, ALPRO_BF16 or ALPRO_F16)", fn, dtype);
  ALPRO_CHECK(L >= 1 && L <= ALPRO_ATTN_MAX_L, "%s: L=%d unsupported (1..%d = ALPRO_ATTN_MAX_L)", fn, L, ALPRO_ATTN_MAX_L);
  ALPRO_CHECK(batch >= 1 && H >= 1, "%s: batch=%d H=%d (need >= 1)", fn, batch, H);
  ALPRO_CHECK(q0 >= 0 && nq >= 1 && nq <= L - q0, "%s: query window q0=%d nq=%d outside 0 <= q0, 1 <= nq, q0 + nq <= L=%d", fn, q0, nq, L);
  ALPRO_CHECK(k0 >= 0 && nk >= 1 && nk <= L - k0, "%s: key window k0=%d nk=%d outside 0 <= k0, 1 <= nk, k0 + nk <= L=%d", fn, k0, nk, L);
  ALPRO_CHECK((int64_t)batch * H * ((nq + MAP_TILE - 1) / MAP_TILE) <= INT_MAX, "%s: batch=%d x H=%d x nq=%d needs more than 2^31 - 1 workgroups", fn, batch,
              H, nq);
  ALPRO_CHECK(qkv != nullptr, "%s: null qkv", fn);
  ALPRO_CHECK(!grad || dctx != nullptr, "%s: null dctx", fn);
  ALPRO_CHECK(lse != nullptr, "%s: null lse", fn);
  ALPRO_CHECK(grad || out != nullptr, "%s: null out", fn);
  ALPRO_CHECK(out != nullptr || cam_out != nullptr, "%s: null grad_out and null cam_out (ask for at least one)", fn);
  ALPRO_CHECK(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)dctx % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)cam_out % 16) == 0,
              "%s: %s must be 16-byte aligned", fn, grad ? "qkv, dctx, grad_out and cam_out" : "qkv and out");
  ALPRO_CHECK(((uintptr_t)lse % 4) == 0 && ((uintptr_t)key_bias % 4) == 0, "%s: lse and key_bias must be 4-byte aligned", fn);
  return ALPRO_OK;
}

// Work items of the temporal map kernels (attention_temporal_probs.hip, attention_temporal_probs_grad.hip), one wave each: T dividing 32 -> a
// (32-row unit, head); any other T -> a (group, head, 32-query tile, 32-key tile)
inline int64_t tp_items(int64_t rows, int T, int H) {
  if (32 % T == 0) return ((rows + 31) / 32) * H;
  const int64_t nt = (T + 31) / 32;
  return (rows / T) * H * nt * nt;
}

// The shape checks of the temporal entry points (fn: the one that was called), in front of their rows == 0 return.  Host only, no HIP call.
inline int map_temporal_check(const char* fn, int dtype, int64_t rows, int T, int H) {
  ALPRO_CHECK(dtype == ALPRO_F32 || dtype == ALPRO_BF16 || dtype == ALPRO_F16, "%s: dtype=%d (ALPRO_F32, ALPRO_BF16 or ALPRO_F16)", fn, dtype);
  ALPRO_CHECK(T >= 1 && T <= ALPRO_ATTN_MAX_T, "%s: num_frm=%d unsupported (1..%d = ALPRO_ATTN_MAX_T)", fn, T, ALPRO_ATTN_MAX_T);
  ALPRO_CHECK(rows >= 0 && rows % T == 0, "%s: rows=%lld not a non-negative multiple of T=%d", fn, (long long)rows, T);
  ALPRO_CHECK(H >= 1, "%s: H=%d (need >= 1)", fn, H);
  ALPRO_CHECK((tp_items(rows, T, H) + MAP_WAVES - 1) / MAP_WAVES <= INT_MAX, "%s: rows=%lld x H=%d at T=%d needs more than 2^31 - 1 workgroups", fn,
              (long long)rows, H, T);
  return ALPRO_OK;
}

}  // namespace alpro
