// Temporal attention over a frame count T that does NOT divide 32 (3 <= T <= ALPRO_ATTN_MAX_T, head_dim 64): the path alpro_attn_temporal_fwd /
// alpro_attn_temporal_bwd take when a frame group may cross a 32-row boundary.  T | 32 keeps the block-diagonal kernels of attention.hip /
// attention_bwd.hip, bit for bit.
//
// Unit = 32 consecutive rows r0 .. r0+31 x one head, as in those kernels; one wave per unit, four independent waves per workgroup, LDS
// wave-private, units handed out grid-stride.  The unit's rows touch the frame groups of the WINDOW
//     [floor(r0 / T) T, min(rows, ceil((r0 + 32) / T) T))      (at most 32 + 2 (T - 1) rows: <= 3 tiles of 32 below T = 32, <= 9 at T = 128)
// and a window row and a unit row see each other iff they share a group (absolute row / T).  The mask is symmetric, so one window serves
// both directions:
//   forward   lane = query of the unit; the window's keys in 32-row tiles (K fragments straight from global, V staged in LDS for the transposed
//             read), online softmax in the log2 domain.  lse ((rows + 31) / 32, H, 32), row c * 32 + r of head h at [c, h, r], as the divisor
//             kernels write it.
//   backward  one launch, two phases per unit, no atomics, no workspace (bitwise reproducible); every (row, head) of dqkv written once:
//             dQ     lane = query of the unit, over the window's keys:    dS^T = P^T o (dP^T - delta) * scale,  dQ^T += K^T dS^T
//             dK/dV  lane = key of the unit, over the window's queries:   dV^T += dO^T P,  dK^T += Q^T dS
//             P is recomputed from Q, K and lse; delta = rowsum(dO o O) -- from registers for the unit's queries, while staging for the window's.
// MFMA forms: 32x32x16 (bf16 / f16) and 32x32x2 f32, as in the other attention kernels.  LDS images are U tiles (attn_tile.hpp).
#include "common.hpp"
#include "attn_tile.hpp"

namespace alpro {
namespace {

template <typename T> struct TCfg : TileCfg<T> {
  static constexpr int NLD = 32 * TileCfg<T>::CPR / 64;  // chunks of one staged 32-row tile per lane
  static constexpr int IMG = 32 * TileCfg<T>::RB;        // bytes of one staged tile
};

// The wave's LDS traffic so far has completed, and the compiler moves no memory access across this point.  A wave's DS operations execute
// in order, so this is all the ordering a wave-private tile needs (write -> read and read -> next write).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// rows row0 .. row0+31 of one head's 64 columns (row stride ld elements) -> LDS tile; rows >= rend zero-filled
template <typename T> __device__ __forceinline__ void stage_tile(char* tile, const T* src, int64_t ld, int64_t row0, int64_t rend, int lane) {
  typedef TCfg<T> C;
  u32x4 v[C::NLD];
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int c = lane + 64 * i, row = c / C::CPR, ch = c - row * C::CPR;
    v[i] = row0 + row < rend ? *(const u32x4*)(src + (row0 + row) * ld + ch * C::CN) : mk4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int c = lane + 64 * i, row = c / C::CPR, ch = c - row * C::CPR;
    *(u32x4*)(tile + tile_off<T>(row, ch)) = v[i];
  }
}

// the unit's window: rows [w0, w1) (every frame group one of the unit's rows r0 .. rend-1 belongs to)
__device__ __forceinline__ void tattn_window(int64_t r0, int64_t rows, int Tn, int64_t& rend, int64_t& w0, int64_t& w1) {
  rend = min(rows, r0 + 32);
  w0 = r0 / Tn * Tn;
  w1 = min(rows, (rend + Tn - 1) / Tn * Tn);
}

#define ALPRO_TDROP 0
#define ALPRO_TKERNEL(name) name##_kernel
#define ALPRO_TDROP_PARAMS
#include "attention_temporal_any_kernels.hpp"
#undef ALPRO_TDROP
#undef ALPRO_TKERNEL
#undef ALPRO_TDROP_PARAMS
#define ALPRO_TDROP 1
#define ALPRO_TKERNEL(name) name##_drop_kernel
#define ALPRO_TDROP_PARAMS , float drop_p, uint32_t drop_seed
#include "attention_temporal_any_kernels.hpp"
#undef ALPRO_TDROP
#undef ALPRO_TKERNEL
#undef ALPRO_TDROP_PARAMS



int64_t tattn_grid(int64_t units) {
  const int64_t grid = (units + 3) / 4;
  return grid < 256 * 8 ? grid : 256 * 8;
}

template <typename T>
int launch_tattn_any_fwd(const void* qkv, void* out, int64_t rows, int Tn, int H, float scale, float* lse, float drop_p, uint32_t drop_seed, hipStream_t st) {
  const size_t lds = 4 * (size_t)TCfg<T>::IMG;
  const int64_t units = ((rows + 31) / 32) * H;
  static DeviceOnce once, once_drop;
  set_lds_once(once, tattn_any_fwd_kernel<T>, lds);
  set_lds_once(once_drop, tattn_any_fwd_drop_kernel<T>, lds);
  if (drop_seed)
    hipLaunchKernelGGL((tattn_any_fwd_drop_kernel<T>), dim3((unsigned)tattn_grid(units)), dim3(256), lds, st, (const T*)qkv, (T*)out, rows, Tn, H, scale, units, lse,
                       drop_p, drop_seed);
  else
    hipLaunchKernelGGL((tattn_any_fwd_kernel<T>), dim3((unsigned)tattn_grid(units)), dim3(256), lds, st, (const T*)qkv, (T*)out, rows, Tn, H, scale, units, lse);
  return check_launch("alpro_attn_temporal_fwd (T not dividing 32)");
}

template <typename T>
int launch_tattn_any_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int64_t rows, int Tn, int H, float scale,
                         float drop_p, uint32_t drop_seed, hipStream_t st) {
  const size_t lds = 4 * (2 * (size_t)TCfg<T>::IMG + 64 * sizeof(float));
  const int64_t units = ((rows + 31) / 32) * H;
  static DeviceOnce once, once_drop;
  set_lds_once(once, tattn_any_bwd_kernel<T>, lds);
  set_lds_once(once_drop, tattn_any_bwd_drop_kernel<T>, lds);
  if (drop_seed)
    hipLaunchKernelGGL((tattn_any_bwd_drop_kernel<T>), dim3((unsigned)tattn_grid(units)), dim3(256), lds, st, (const T*)qkv, (const T*)out, (const T*)dout, lse,
                       (T*)dqkv, rows, Tn, H, scale, units, drop_p, drop_seed);
  else
    hipLaunchKernelGGL((tattn_any_bwd_kernel<T>), dim3((unsigned)tattn_grid(units)), dim3(256), lds, st, (const T*)qkv, (const T*)out, (const T*)dout, lse,
                     (T*)dqkv, rows, Tn, H, scale, units);
  return check_launch("alpro_attn_temporal_bwd (T not dividing 32)");
}

}  // namespace

// entry points of alpro_attn_temporal_fwd / alpro_attn_temporal_bwd for 32 % T != 0, T <= ALPRO_ATTN_MAX_T (arguments checked by the callers)
// (drop_seed == 0: dropout off)
int attn_temporal_any_fwd(const void* qkv, void* out, int dtype, int64_t rows, int T, int H, float scale, float* lse, float drop_p, uint32_t drop_seed,
                          hipStream_t st) {
  ALPRO_DISPATCH_DTYPE(dtype, T_, return launch_tattn_any_fwd<T_>(qkv, out, rows, T, H, scale, lse, drop_p, drop_seed, st));
  return ALPRO_OK;
}
int attn_temporal_any_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int64_t rows, int T, int H,
                          float scale, float drop_p, uint32_t drop_seed, hipStream_t st) {
  ALPRO_DISPATCH_DTYPE(dtype, T_, return launch_tattn_any_bwd<T_>(qkv, out, dout, lse, dqkv, rows, T, H, scale, drop_p, drop_seed, st));
  return ALPRO_OK;
}

}  // namespace alpro
