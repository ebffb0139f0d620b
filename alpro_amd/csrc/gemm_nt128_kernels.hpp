// NT GEMM with fused epilogue for gfx950:  C = epilogue(A[M,K] * W[N,K]^T).
//
// Tile 128x128 per 256-thread workgroup (4 waves, 2x2, each 64x64 = 2x2 MFMA 32x32 accumulators),
// K-tile = 128 BYTES per row (64 bf16/f16 or 32 f32), so staging, LDS image and fragment reads are
// identical for every storage dtype; only mma_chunk<T> differs (common.hpp).
//  * global -> registers -> LDS double buffer, next tile's loads issued before the MFMAs of the
//    current one (one barrier per K-tile);
//  * LDS rows are 128 B; the 16-B chunk index is XOR-swizzled with (row >> 1) & 7 so that every
//    ds_read_b128 lane group of a fragment read hits 16 distinct 16-B slots of the 256-B bank row;
//  * workgroup -> tile map is XCD-aware: each XCD (blockIdx % 8) walks a contiguous range of tiles
//    with the N tiles of one A row-panel adjacent, so the panel is fetched into one L2 only.
#pragma once
#include "gemm_epilogue.hpp"
namespace alpro {
namespace {
constexpr int BM = 128, BN = 128, NT = 256;
constexpr int TILE_BYTES = BM * ROWB;  // 16 KiB per operand per buffer

template <typename T, int ACT, int MAP>
__device__ __forceinline__ void gemm_nt_tile(const alpro_gemm_desc_t& g, const int bid, char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ntn = (g.N + BN - 1) / BN, ntm = (g.M + BM - 1) / BM;
  const int nblk = ntn * ntm;
  if (bid >= nblk) return;  // (batched launches size the grid for the largest job)
  // XCD-aware, bijective remap of blockIdx -> logical tile
  int tile;
  {
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int m0 = tm * BM, n0 = tn * BN;

  const char* Ab = (const char*)g.A;
  const char* Wb = (const char*)g.W;
  const int64_t lda_b = g.lda * (int64_t)sizeof(T), ldw_b = g.ldw * (int64_t)sizeof(T);

  // staging: 1024 16-B chunks per operand tile, 4 per thread
  const char* a_src[4];
  const char* w_src[4];
  int st_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + i * NT, row = c >> 3, ch = c & 7;
    const int am = min(m0 + row, g.M - 1), wn = min(n0 + row, g.N - 1);
    a_src[i] = Ab + am * lda_b + ch * 16;
    w_src[i] = Wb + wn * ldw_b + ch * 16;
    st_off[i] = lds_off(row, ch);
  }
  // fragment read offsets (bytes within an operand tile) for k-step s: XOR of chunk index is per row
  int a_row[2], b_row[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_row[i] = wr * 64 + i * 32 + (lane & 31);
    b_row[i] = wc * 64 + i * 32 + (lane & 31);
  }
  const int khalf = lane >> 5;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = (g.K * (int)sizeof(T)) / ROWB;
  u32x4 ra[4], rw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = *(const u32x4*)(a_src[i]);
    rw[i] = *(const u32x4*)(w_src[i]);
  }
  char* bufA = smem;
  char* bufW = smem + 2 * TILE_BYTES;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *(u32x4*)(bufA + st_off[i]) = ra[i];
    *(u32x4*)(bufW + st_off[i]) = rw[i];
  }
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // issue the next tile's global loads before this tile's MFMAs (the last iteration re-reads its own,
    // L1-resident tile: keeping the loads unconditional keeps the staging registers out of scratch)
    {
      const int64_t ko = (int64_t)min(kt + 1, nk - 1) * ROWB;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = *(const u32x4*)(a_src[i] + ko);
        rw[i] = *(const u32x4*)(w_src[i] + ko);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // loads stay ahead of the MFMAs (hipcc would sink them to the ds_write)
    const char* cA = bufA + cur * TILE_BYTES;
    const char* cW = bufW + cur * TILE_BYTES;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *(const u32x4*)(cA + lds_off(a_row[i], 2 * s + khalf));
        fb[i] = *(const u32x4*)(cW + lds_off(b_row[i], 2 * s + khalf));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mma_chunk<T>(acc[i][j], fa[i], fb[j]);
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      char* nA = bufA + (cur ^ 1) * TILE_BYTES;
      char* nW = bufW + (cur ^ 1) * TILE_BYTES;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *(u32x4*)(nA + st_off[i]) = ra[i];
        *(u32x4*)(nW + st_off[i]) = rw[i];
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue (the trailing __syncthreads of the K loop guarantees nobody still reads the staging tiles)
  float* stage = (float*)(smem + wave * (64 * 64 * 4));
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, lane), col = lane & 31;
    stage[row * 64 + col] = acc[0][0][r];
    stage[row * 64 + 32 + col] = acc[0][1][r];
    stage[(32 + row) * 64 + col] = acc[1][0][r];
    stage[(32 + row) * 64 + 32 + col] = acc[1][1][r];
  }
  wave_lds_handoff();
  const int mb = m0 + wr * 64, nb = n0 + wc * 64;
  float bias[4];
  load_bias4(g, nb + (lane & 15) * 4, bias);
  if (epi_fast_ok(g, mb, 64, nb)) {
#pragma unroll
    for (int c = 0; c < 4; ++c) epi_rows16<T, ACT, MAP, true>(g, stage + c * 16 * 64, mb + c * 16, nb, lane, bias);
  } else {
#pragma unroll 1
    for (int c = 0; c < 4; ++c) epi_rows16<T, ACT, MAP, false>(g, stage + c * 16 * 64, mb + c * 16, nb, lane, bias);
  }
}

template <typename T, int ACT, int MAP>
__global__ __launch_bounds__(NT, 2) void gemm_nt_kernel(const alpro_gemm_desc_t g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_nt_tile<T, ACT, MAP>(g, blockIdx.x, smem);
}

// Many small independent GEMMs in ONE launch (round 3): blockIdx.y = job, descriptors in device memory.  The merged temporal projection
// needs, per ViT block and optimizer step, W_e = W_fc W_p (a 768^3 product on 36 workgroups, 64 us) and, in backward, two more 768^3
// products for the product rule -- 12 blocks x 3 launches that each fill a seventh of the chip; batched they run side by side.
template <typename T, int ACT, int MAP>
__global__ __launch_bounds__(NT, 2) void gemm_nt_batch_kernel(const alpro_gemm_desc_t* __restrict__ descs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const alpro_gemm_desc_t g = descs[blockIdx.y];
  gemm_nt_tile<T, ACT, MAP>(g, blockIdx.x, smem);
}
}  // namespace
}  // namespace alpro
