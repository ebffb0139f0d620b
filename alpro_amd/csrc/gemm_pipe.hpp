// Pieces shared by the phase-scheduled GEMM kernels on v_mfma_f32_16x16x32 fragments: gemm_nt256q_kernel (gemm_nt256q_kernels.hpp) and
// gemm_qkv_tattn_kernel (gemm_tattn.hip).  One copy of each; the LDS-DMA issue with an SGPR base sits next to dma16 in common.hpp.
#pragma once
#include "common.hpp"
namespace alpro {
namespace {
constexpr int ROWB = 128;   // bytes per LDS row of every GEMM kernel: one K-tile = 64 16-bit / 32 fp32 elements

template <typename T> struct Mma16;   // D = A(16 x 32) B(32 x 16) + C on packed 16-byte operand fragments
template <> struct Mma16<bf16_t> {
  static __device__ __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
};
template <> struct Mma16<f16_t> {
  static __device__ __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};

// the barrier between a LOAD and an MFMA segment: nothing is scheduled across it
__device__ __forceinline__ void phase_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// Four staged 8-byte units q[j] = (rows 0-3 of the lane's four) x (column pair member: .x/.y = column 2j, .z/.w = column 2j + 1), 16 bits
// each -> the 16-byte piece (8 columns) of row r
__device__ __forceinline__ u32x4 units_to_row(const u32x4 (&q)[4], int r) {
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t a = (r & 2) ? q[j].y : q[j].x, b = (r & 2) ? q[j].w : q[j].z;   // column 2j / 2j + 1, rows (r & 2), (r & 2) + 1
    o[j] = __builtin_amdgcn_perm(b, a, (r & 1) ? 0x07060302u : 0x05040100u);
  }
  return o;
}
}  // namespace
}  // namespace alpro
