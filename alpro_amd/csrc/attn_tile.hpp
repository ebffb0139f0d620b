// What the attention translation units (attention.hip, attention_bwd.hip, attention_long.hip, attention_temporal_any.hip) share: the per-dtype
// tile geometry, the "U" LDS tile layout (one swizzle for row reads AND transposed reads), the transposed A-operand loader built on
// ds_read_b64_tr_b16, and the accumulator -> output-row store.  Head dim 64, wave64, MFMA 32x32; a 16-byte chunk is the unit of every LDS image.
// The forward's own K and V images (k_swz / v_swz, attention.hip) are different layouts and stay in that file.
#pragma once
#include "common.hpp"

namespace alpro {
namespace {

constexpr int HD = 64;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.69314718055994531f;

typedef short s16x4 __attribute__((ext_vector_type(4)));

// Storage dtype T: bf16 / f16 (K = 16 MFMA) or f32 (K = 2 MFMA, exact mode).  Per-file constants (staged-image sizes, ring depths) go on a
// struct that derives from this one.
template <typename T> struct TileCfg {
  static constexpr int E = sizeof(T);
  static constexpr int CN = 16 / E;        // elements per 16-byte chunk
  static constexpr int RB = HD * E;        // bytes per head row
  static constexpr int CPR = RB / 16;      // chunks per head row (8 or 16)
  static constexpr int KS = CPR / 2;       // MFMA chunk-steps over head_dim (two lane halves per step)
  static constexpr int CPT = 16 / CN;      // P chunks per 32-row tile (2 or 4)
};

// ---- the U tile: row-major (row, 64) with the 16-byte chunk index swizzled by the row ----------------------------------------------------
// 16-bit rows (128 B): chunk ^= bit1(row) << 2 | (row >> 2) & 3.  That is a bijection of (row >> 1) & 7, so the ds_read_b128 row fragments of
// an MFMA operand (consecutive rows, one chunk column) are conflict-free, AND it moves rows r and r + 2 into different 64-byte windows, so the
// 4-row gathers of the transposed read are conflict-free too: one image serves both access kinds.  32-bit rows (256 B): chunk ^= row & 15.
template <typename T> __device__ __forceinline__ int u_swz(int row, int chunk) {
  if (TileCfg<T>::CPR == 8) return chunk ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
  return chunk ^ (row & 15);
}
// byte offset of chunk `chunk` of row `row`; every store into and every read from a U tile goes through it
template <typename T> __device__ __forceinline__ int tile_off(int row, int chunk) { return row * TileCfg<T>::RB + (u_swz<T>(row, chunk) << 4); }

// ---- hardware transpose read ---------------------------------------------------------------------------------------------------------------
// ds_read_b64_tr_b16 semantics (probed on gfx950, tools/probe_tr.hip): within each 16-lane group, lane l receives element (l & 3) of the
// 8-byte piece addressed by lane (l >> 2) + 4j, j = 0..3.  Lane p of a group therefore points at row krow0 + (p >> 2), d-quad (p & 3) of its
// group's 16-wide d block (`seg`), and every lane gets 4 consecutive rows of its own d column.  All 64 lanes must be active.
__device__ __forceinline__ u32x2 ds_read_tr16(const char* a) {
  const s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
  return __builtin_bit_cast(u32x2, r);
}
// rows krow0 .. krow0+3 of column dt*32 + (lane & 31) of a 16-bit U tile
__device__ __forceinline__ u32x2 tr_quad(const char* tile, int krow0, int lane, int dt) {
  const int p = lane & 15, seg = dt * 2 + ((lane >> 4) & 1);
  const int row = krow0 + (p >> 2);
  const int ch = seg * 2 + ((p >> 1) & 1);
  typedef bf16_t T16;   // the layout depends on sizeof(T) only
  // (tile_off()'s terms added to the pointer one by one: with the integer sum formed first, tattn_any_bwd_kernel came out 4 VGPRs larger)
  return ds_read_tr16(tile + row * TileCfg<T16>::RB + (u_swz<T16>(row, ch) << 4) + ((p & 1) << 3));
}

// transposed A-operand chunk of a U tile: element (k, i) = tile[row0 + krow(cc, g, k)][dt*32 + (lane & 31)], the k order being the
// accumulator-register order of the matching B operand (regs cc*CN .. cc*CN+CN-1)
template <typename T> __device__ __forceinline__ u32x4 load_t_chunk(const char* tile, int row0, int cc, int lane, int dt);
template <> __device__ __forceinline__ u32x4 load_t_chunk<float>(const char* tile, int row0, int cc, int lane, int dt) {
  const int d = dt * 32 + (lane & 31), r = row0 + 8 * cc + 4 * (lane >> 5);
  uint32_t v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = *(const uint32_t*)(tile + tile_off<float>(r + e, d >> 2) + ((d & 3) << 2));
  return mk4(v[0], v[1], v[2], v[3]);
}
template <typename T> __device__ __forceinline__ u32x4 load_t_chunk16(const char* tile, int row0, int cc, int lane, int dt) {
  const int g = lane >> 5;
  const u32x2 a = tr_quad(tile, row0 + 16 * cc + 4 * g, lane, dt);      // regs 8cc..8cc+3
  const u32x2 b = tr_quad(tile, row0 + 16 * cc + 8 + 4 * g, lane, dt);  // regs 8cc+4..8cc+7
  const uint32_t ax = a.x, ay = a.y, bx = b.x, by = b.y;
  return mk4(ax, ay, bx, by);
}
template <> __device__ __forceinline__ u32x4 load_t_chunk<bf16_t>(const char* tile, int row0, int cc, int lane, int dt) { return load_t_chunk16<bf16_t>(tile, row0, cc, lane, dt); }
template <> __device__ __forceinline__ u32x4 load_t_chunk<f16_t>(const char* tile, int row0, int cc, int lane, int dt) { return load_t_chunk16<f16_t>(tile, row0, cc, lane, dt); }

// ---- dropout mask indices of the block-diagonal temporal kernels (32 % Tn == 0: a 32-row unit holds whole frame groups) ------------------------
// Contract of alpro_attn_fwd with batch = rows / Tn, L = Tn: index ((grp H + h) Tn + q) Tn + k, grp = row / Tn, formed in 64 bits.  For the unit at
// row r0 and the token of lane ql:  as a QUERY against local key `key`:  temporal_drop_base(...) + key;  as a KEY against local query `qq`:
// temporal_drop_base_key(...) + qq * Tn.  Tokens of other groups get an index that means nothing -- their probability is 0.
__device__ __forceinline__ uint64_t temporal_drop_base(int64_t r0, int ql, int Tn, int H, int h) {
  const int lg = ql / Tn;
  return (((uint64_t)(r0 / Tn + lg) * H + h) * Tn + (uint64_t)(ql - lg * Tn)) * Tn - (uint64_t)(lg * Tn);
}
__device__ __forceinline__ uint64_t temporal_drop_base_key(int64_t r0, int ql, int Tn, int H, int h) {
  const int lg = ql / Tn;
  return (((uint64_t)(r0 / Tn + lg) * H + h) * Tn - (uint64_t)(lg * Tn)) * Tn + (uint64_t)(ql - lg * Tn);
}

// ---- accumulators -> global ----------------------------------------------------------------------------------------------------------------
// store 4 consecutive values d0..d0+3 of one row
template <typename T> __device__ __forceinline__ void store_quad(T* dst, const float* v) {
  if constexpr (sizeof(T) == 4) {
    *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    u32x2 u;
    u.x = pack2(v[0], v[1], (T*)0);
    u.y = pack2(v[2], v[3], (T*)0);
    *(u32x2*)dst = u;
  }
}
// accumulator pair (2 d-tiles, C layout: column = row of this lane, rows = d) -> one row of 64 values
template <typename T> __device__ __forceinline__ void store_row64(T* row, const f32x16 (&o)[2], int lane) {
  const int g = lane >> 5;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const float v[4] = {o[dt][4 * rq], o[dt][4 * rq + 1], o[dt][4 * rq + 2], o[dt][4 * rq + 3]};
      store_quad<T>(row + dt * 32 + 8 * rq + 4 * g, v);
    }
}

}  // namespace
}  // namespace alpro
