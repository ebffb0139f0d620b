// The 768-wide row as one wave holds it (core.hip, backward.hip): 12 fp32 per lane, v[4 * i + e] = column i * 256 + lane * 4 + e, moved as three
// 16-byte accesses (8-byte for 16-bit storage).  The loads and stores, the LayerNorm statistics, the row maps and the per-row dropout mask live
// here once: the forward and the backward regenerate the same mask from the same index only as long as both use row_drop_keep.
#pragma once
#include "common.hpp"

namespace alpro {

constexpr int LN_D = 768, LN_V = 3;

// column of element i of a lane's 12
__device__ __forceinline__ int row_col(int lane, int i) { return (i >> 2) * 256 + lane * 4 + (i & 3); }

__device__ __forceinline__ void ln_load(const float* row, int lane, float (&v)[12]) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    const float4 f = *(const float4*)(row + i * 256 + lane * 4);
    v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
  }
}
// row += v (plain read-modify-write: the single writer of a scatter's destination row)
__device__ __forceinline__ void ln_accum_row(float* row, int lane, const float (&v)[12]) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    float4* p = (float4*)(row + i * 256 + lane * 4);
    const float4 c = *p;
    *p = make_float4(c.x + v[4 * i], c.y + v[4 * i + 1], c.z + v[4 * i + 2], c.w + v[4 * i + 3]);
  }
}
// streamed-once rows (token rows, x, dy, the gradient stream): non-temporal
__device__ __forceinline__ void ln_load_nt(const float* row, int lane, float (&v)[12]) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    const f32x4 f = __builtin_nontemporal_load((const f32x4*)(row + i * 256 + lane * 4));
    v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
  }
}
// a streamed-once row in storage type T (fp32 or 16-bit)
template <typename T> __device__ __forceinline__ void ln_load_t(const T* row, int lane, float (&v)[12]) {
  if constexpr (sizeof(T) == 4) {
    ln_load_nt((const float*)row, lane, v);
  } else {
#pragma unroll
    for (int i = 0; i < LN_V; ++i) {
      const u32x2 u = __builtin_nontemporal_load((const u32x2*)(row + i * 256 + lane * 4));
      const uint32_t w0 = u.x, w1 = u.y;
      v[4 * i] = to_f32(T{(uint16_t)(w0 & 0xffffu)}); v[4 * i + 1] = to_f32(T{(uint16_t)(w0 >> 16)});
      v[4 * i + 2] = to_f32(T{(uint16_t)(w1 & 0xffffu)}); v[4 * i + 3] = to_f32(T{(uint16_t)(w1 >> 16)});
    }
  }
}
// v += w * (a streamed-once row in storage type T)
template <typename T>
__device__ __forceinline__ void add_delta_row(const T* drow, int lane, float (&v)[12], float w) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 f = __builtin_nontemporal_load((const f32x4*)(drow + i * 256 + lane * 4));
      v[4 * i] += w * f.x; v[4 * i + 1] += w * f.y; v[4 * i + 2] += w * f.z; v[4 * i + 3] += w * f.w;
    } else {
      const u32x2 u = __builtin_nontemporal_load((const u32x2*)(drow + i * 256 + lane * 4));
      const uint32_t ux = u.x, uy = u.y;
      v[4 * i] += w * to_f32(T{(uint16_t)(ux & 0xFFFFu)});
      v[4 * i + 1] += w * to_f32(T{(uint16_t)(ux >> 16)});
      v[4 * i + 2] += w * to_f32(T{(uint16_t)(uy & 0xFFFFu)});
      v[4 * i + 3] += w * to_f32(T{(uint16_t)(uy >> 16)});
    }
  }
}

__device__ __forceinline__ void ln_stats(const float (&v)[12], float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i) s += v[i];
  mean = wave_sum(s) * (1.0f / LN_D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const float d = v[i] - mean;
    q += d * d;
  }
  rstd = rsqrtf(wave_sum(q) * (1.0f / LN_D) + eps);
}
__device__ __forceinline__ void ln_affine(float (&v)[12], float mean, float rstd, const float* gamma, const float* beta, int lane) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    const float4 g = *(const float4*)(gamma + i * 256 + lane * 4), b = *(const float4*)(beta + i * 256 + lane * 4);
    v[4 * i] = (v[4 * i] - mean) * rstd * g.x + b.x;
    v[4 * i + 1] = (v[4 * i + 1] - mean) * rstd * g.y + b.y;
    v[4 * i + 2] = (v[4 * i + 2] - mean) * rstd * g.z + b.z;
    v[4 * i + 3] = (v[4 * i + 3] - mean) * rstd * g.w + b.w;
  }
}

// fp32: non-temporal; 16-bit: plain
template <typename T>
__device__ __forceinline__ void ln_store(T* row, int lane, const float (&v)[12]) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    if constexpr (sizeof(T) == 4) {
      __builtin_nontemporal_store(f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]}, (f32x4*)(row + i * 256 + lane * 4));
    } else {
      T* p = row + i * 256 + lane * 4;
      u32x2 u;
      u.x = pack2(v[4 * i], v[4 * i + 1], (T*)0);
      u.y = pack2(v[4 * i + 2], v[4 * i + 3], (T*)0);
      *(u32x2*)p = u;  // plain, not non-temporal: 154 MB at the benchmark size stay in the Infinity Cache for the GEMM that reads them next
                       // (step 174.1 -> 171.4 ms together with gather_cast; the same change on GEMM / attention outputs LOSES 5 ms)
    }
  }
}
// row = sc * v, plain for fp32 too (the LayerNorm backward's emitted operand rows)
template <typename T>
__device__ __forceinline__ void ln_store_scaled(T* p, int lane, const float (&v)[12], float sc) {
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    T* q = p + i * 256 + lane * 4;
    if constexpr (sizeof(T) == 4) {
      *(f32x4*)q = f32x4{v[4 * i] * sc, v[4 * i + 1] * sc, v[4 * i + 2] * sc, v[4 * i + 3] * sc};
    } else {
      u32x2 u;
      u.x = pack2(v[4 * i] * sc, v[4 * i + 1] * sc, (T*)0);
      u.y = pack2(v[4 * i + 2] * sc, v[4 * i + 3] * sc, (T*)0);
      *(u32x2*)q = u;  // plain store: the wgrad / dgrad GEMMs read it next out of the Infinity Cache (like alpro_gather_cast)
    }
  }
}

// The source row of output row m under the row maps of alpro_hip.h (the forward gathers, the backward scatters).
struct SrcRow {
  int64_t row;
  bool shared;  // the source row is gathered by several output rows (CLS under FRAME_TOKENS): scatter atomically
};
__device__ __forceinline__ SrcRow ln_src_row(int mode, int p0, int p1, int64_t m) {
  SrcRow s;
  s.shared = false;
  if (mode == ALPRO_MAP_IDENTITY) { s.row = m; return s; }
  if (mode == ALPRO_MAP_SKIP_CLS) { s.row = m + m / p0 + 1; return s; }
  const int T = p0, N = p1;  // FRAME_TOKENS gather
  const int64_t bt = m / (N + 1);
  const int j = (int)(m - bt * (N + 1));
  const int64_t b = bt / T;
  const int t = (int)(bt - b * T);
  const int64_t base = b * (1 + (int64_t)N * T);
  s.shared = j == 0;
  s.row = j == 0 ? base : base + 1 + (int64_t)(j - 1) * T + t;
  return s;
}

// Dropout keep-mask of element i of row `row`: a function of (seed, row * 768 + column) alone.
// Per element, the 12-element loop stays at the caller: a helper that owns the loop is unrolled before it is inlined and compiles to other
// code (profiles/r12_rowwise_isa.txt).
__device__ __forceinline__ bool row_drop_keep(uint32_t seed, int64_t row, int lane, int i, uint32_t thresh24) {
  return drop_keep(seed, (uint64_t)row * LN_D + (uint64_t)row_col(lane, i), thresh24);
}

}  // namespace alpro
