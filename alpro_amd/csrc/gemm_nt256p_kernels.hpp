// ------------------------------------------------------------------------------------------------
// 256x256 tile, 8 waves (2 x 4, each 128x64 = 4x2 MFMA accumulators), K-tile 128 bytes, two LDS stages of
// 64 KiB filled by global_load_lds_dwordx4 (no VGPR round trip, no ds_write).  The LDS image written by
// the DMA is lane-linear (1 KiB = 8 rows per wave instruction), so the bank swizzle is applied to the
// per-lane SOURCE chunk and undone by the same XOR on the fragment read (linear dest + swizzled source).
#pragma once
#include "gemm_epilogue.hpp"
namespace alpro {
namespace {
constexpr int BM2 = 256, BN2 = 256, NT2 = 512;
constexpr int TILE2_BYTES = BM2 * ROWB;  // 32 KiB per operand per stage

// ------------------------------------------------------------------------------------------------
// Persistent form of the 256x256 kernel: one workgroup per CU walks its tiles (XCD-contiguous order).  On the
// K = 768 shapes of this model a tile is only 12 K-steps, so what the one-tile-per-workgroup kernel loses is the
// ~16 us per tile of workgroup turn-around + first-tile DMA latency + epilogue; here the first K-tile of the
// NEXT tile is DMA-prefetched before the epilogue runs, and the epilogue stages through its own 32 KiB of LDS
// (16 rows x 64 columns per wave at a time) so the two 64 KiB stage buffers are free to receive it.
// Fragment reads are register double-buffered (the reads of K-chunk s+1 are in flight under the MFMAs of s).
constexpr int EPI_BYTES = 8 * 16 * 64 * 4;  // 32 KiB: 8 waves x (16 rows x 64 cols) fp32

// TUNE: where the 8 DMA pieces of the next K-tile are issued among the 32 MFMAs of a K-step (experiment knob, ALPRO_GEMM_TUNE):
//   0  copy c after MFMA 4c+1 (waves 0-3) / 4c+3 (waves 4-7): spread over the whole step -- the last piece is issued ~100 cycles
//      before the step ends, so its full L2 / MALL latency is exposed at the next step's vmcnt(0)
//   1  copy c after MFMA 2c+1 / 2c+2: all pieces out in the first half of the step (default: +3-5 % on every shape,
//      round-2 A/B of the variants on the model shapes)
//   2  copy c after MFMA 3c+1 / 3c+2: first three quarters
__device__ __forceinline__ constexpr int copy_slot(int tune, int q, int pos) {
  if (tune == 0) return ((q & 1) && ((q >> 1) & 1) == pos) ? (q >> 2) : -1;
  if (tune == 1) { const int r = q - 1 - pos; return (r >= 0 && r < 16 && (r & 1) == 0) ? (r >> 1) : -1; }
  const int r = q - 1 - pos;
  return (r >= 0 && r < 24 && r % 3 == 0) ? r / 3 : -1;
}

// Tail split (round 3): with nblk = Q * grid + R tiles, the last round keeps only R workgroups busy (M = 50176 x N = 768 at B = 32: 591
// tiles on 256 CUs = 2.31 -> 3 rounds, 77 %).  When 2R <= grid, each tile of that round is cut in two along M and handed to TWO
// workgroups: a half tile is a 128 x 256 tile whose upper wave row (waves 4-7, one per SIMD) idles -- it still issues its share of the
// DMA and takes the barriers -- so the round costs about half of a full one (2.31 -> 2.5 round-equivalents instead of 3).
template <typename T, int ACT, int MAP, int TUNE = 1>
__global__ __launch_bounds__(NT2, 2) void gemm_nt256p_kernel(const alpro_gemm_desc_t g, const int tail_split) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int ntn = (g.N + BN2 - 1) / BN2, ntm = (g.M + BM2 - 1) / BM2;
  const int nblk = ntn * ntm;
  const int64_t lda_b = g.lda * (int64_t)sizeof(T), ldw_b = g.ldw * (int64_t)sizeof(T);
  const int nk = (g.K * (int)sizeof(T)) / ROWB;
  // XCD-contiguous walk: within one round of gridDim.x tiles, XCD x (= blockIdx % 8) owns a contiguous run
  const int per_xcd = (gridDim.x + 7) >> 3;
  const int slot = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* gbl_ptr;

  const char* a_src[4];
  const char* w_src[4];
  int m0 = 0, n0 = 0;
  const int G = gridDim.x;
  const int q_full = nblk / G, rem = nblk - q_full * G;
  const bool split = tail_split && rem > 0 && 2 * rem <= G;
  // it-th tile of this workgroup: (tile, half) with half = -1 for a full tile, 0 / 1 for the lower / upper 128 rows of a split tile
  auto locate = [&](int it, int& t, int& hf) -> bool {
    hf = -1;
    if (it < q_full) { t = slot + it * G; return true; }
    if (it > q_full) return false;
    if (split) {
      if (slot >= 2 * rem) return false;
      t = q_full * G + (slot >> 1);
      hf = slot & 1;
      return true;
    }
    t = q_full * G + slot;
    return slot < rem;
  };
  auto setup = [&](int tile, int hf) {
    const int tm = tile / ntn, tn = tile - tm * ntn;
    m0 = tm * BM2 + (hf > 0 ? BM2 / 2 : 0);
    n0 = tn * BN2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (wave + 8 * i) * 8 + (lane >> 3);
      const int ch = (lane & 7) ^ ((row >> 1) & 7);
      a_src[i] = (const char*)g.A + min(m0 + row, g.M - 1) * lda_b + ch * 16;
      w_src[i] = (const char*)g.W + min(n0 + row, g.N - 1) * ldw_b + ch * 16;
    }
  };
  const uint32_t lds_base = lds_addr_of(smem);
  // copy c = 0..7 of K-tile kt into stage buffer buf: (A, W) x 4 pieces of 1 KiB per wave.  Issued from inline asm
  // (common.hpp dma16) and tracked by the hand-placed vmcnt waits below.
  auto copy_piece = [&](int c, int kt, int buf, bool half_a = false) {
    const int i = c >> 1;
    if (half_a && !(c & 1) && i >= 2) return;  // rows 128..255 of a half tile's A image are never read
    const char* src = ((c & 1) ? w_src[i] : a_src[i]) + (int64_t)kt * ROWB;
    dma16(src, __builtin_amdgcn_readfirstlane(lds_base + buf * 2 * TILE2_BYTES + (c & 1) * TILE2_BYTES + (wave + 8 * i) * 1024));
  };
  auto stage_tile = [&](int kt, int buf, bool half_a = false) {
#pragma unroll
    for (int c = 0; c < 8; ++c) copy_piece(c, kt, buf, half_a);
  };
  int a_row[4], b_row[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_row[i] = wr * 128 + i * 32 + (lane & 31);
#pragma unroll
  for (int j = 0; j < 2; ++j) b_row[j] = wc * 64 + j * 32 + (lane & 31);
  const int khalf = lane >> 5;
  float* stage = (float*)(smem + 4 * TILE2_BYTES + wave * (16 * 64 * 4));

  int it = 0, tile, hf;
  if (!locate(0, tile, hf)) return;
  // Invariant at the top of every tile: K-tiles 0 and 1 are in buffers s0 and s0^1 and this wave has no DMA in flight,
  // so the first two K-steps need no vmcnt wait -- the previous tile's output stores drain underneath them.
  const int pos = wave >> 2;
  auto wait_vm0 = [] { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
  auto block_sync = [] {  // barrier that does NOT drain vmcnt (a __syncthreads() would wait for the output stores)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  setup(tile, hf);
  int s0 = 0;
  stage_tile(0, 0, hf >= 0);
  stage_tile(1, 1, hf >= 0);
  wait_vm0();
  while (true) {
    const int tm0 = m0, tn0 = n0;
    int next, next_hf;
    const bool more = locate(it + 1, next, next_hf);
    const bool active = hf < 0 || wr == 0;   // half tile: the upper wave row has nothing to compute
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = s0 ^ (kt & 1);
      if (kt >= 2) wait_vm0();  // own pieces of K-tile kt (issued one step ago); at kt == 2 also the previous tile's stores
      block_sync();             // K-tile kt visible to everyone; everyone is done with K-tile kt-1
      // The buffer of K-tile kt-1 is free from here on: its 8 copies (K-tile kt+1, or K-tile 0 of the NEXT tile on the
      // last step) are issued BETWEEN this step's 32 MFMAs, and the two waves that share a SIMD (w, w+4) use alternating
      // slots -- a copy stalls its wave ~60-150 cycles at issue, which the partner's MFMAs cover; issued back to back by
      // all 8 waves right after the barrier they idle the whole CU for several hundred cycles per K-step.
      int ckt = kt + 1;
      bool do_copy = kt >= 1 && kt + 1 < nk;
      bool copy_half = hf >= 0;
      if (kt >= 1 && kt + 1 == nk && more) {  // last step: start the NEXT tile's first K-tile
        setup(next, next_hf);
        ckt = 0;
        do_copy = true;
        copy_half = next_hf >= 0;
      }
      if (!active) {  // idle wave row of a half tile: its share of the DMA, nothing else (the barriers above / below are taken by everybody)
        if (do_copy) {
#pragma unroll
          for (int c = 0; c < 8; ++c) copy_piece(c, ckt, cur ^ 1, copy_half);
        }
        continue;
      }
      const char* cA = smem + cur * 2 * TILE2_BYTES;
      const char* cW = cA + TILE2_BYTES;
      u32x4 fa[2][4], fb[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[0][j] = *(const u32x4*)(cW + lds_off(b_row[j], khalf));
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[0][i] = *(const u32x4*)(cA + lds_off(a_row[i], khalf));
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < 3) {
#pragma unroll
          for (int j = 0; j < 2; ++j) fb[(s + 1) & 1][j] = *(const u32x4*)(cW + lds_off(b_row[j], 2 * (s + 1) + khalf));
#pragma unroll
          for (int i = 0; i < 4; ++i) fa[(s + 1) & 1][i] = *(const u32x4*)(cA + lds_off(a_row[i], 2 * (s + 1) + khalf));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            mma_chunk<T>(acc[i][j], fa[s & 1][i], fb[s & 1][j]);
            const int q = s * 8 + i * 2 + j;  // 0..31; see copy_slot
            if (do_copy) {
              if (copy_slot(TUNE, q, 0) >= 0 && pos == 0) copy_piece(copy_slot(TUNE, q, 0), ckt, cur ^ 1, copy_half);
              if (copy_slot(TUNE, q, 1) >= 0 && pos == 1) copy_piece(copy_slot(TUNE, q, 1), ckt, cur ^ 1, copy_half);
            }
          }
      }
    }
    block_sync();  // everyone is done with the last K-tile: its buffer takes the next tile's K-tile 1
    const int last = s0 ^ ((nk - 1) & 1);
    if (more) stage_tile(1, last, next_hf >= 0);
    s0 = last ^ 1;
    // epilogue; the two prefetched K-tiles must have landed before the first output store is issued (after that,
    // vmcnt also counts the stores and nobody waits on it until K-step 2 of the next tile)
    if (active) {
      const int mb = tm0 + wr * 128, nb = tn0 + wc * 64;
      float bias[4];
      load_bias4(g, nb + (lane & 15) * 4, bias);
      wait_vm0();
      // 8-row chunks through two alternating 2 KiB staging buffers per wave: the ds_writes of chunk c+1 are independent
      // of the ds_reads of chunk c, so LDS latency and the global stores of consecutive chunks overlap.  No hardware
      // wait is needed (DS operations of one wave execute in order); the compiler's order is pinned by wave_lds_order().
      auto stage_chunk = [&](float* st, const f32x16& a0, const f32x16& a1, int q) {
        wave_lds_order();
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int row = r4 + 4 * (lane >> 5);
          st[row * 64 + (lane & 31)] = a0[4 * q + r4];
          st[row * 64 + 32 + (lane & 31)] = a1[4 * q + r4];
        }
        wave_lds_order();
      };
      auto run_epilogue = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const bool pf = FAST && MAP != ALPRO_MAP_FRAME_TOKENS && g.residual != nullptr;  // (FRAME_TOKENS: its row map + the ring would spill)  // residual rows are fetched one chunk ahead (see epi_prefetch_res)
        // Residual ring: RD - 1 chunks (2 KiB per wave each) are in flight ahead of the one being finished.
        constexpr int RD = 2;  // deeper (4: no change, 6: spills) -- profiles/r2_gemm_epilogue_experiments.txt item 5
        float4 ring[RD][2];
        if (pf) {
#pragma unroll
          for (int c0 = 0; c0 < RD - 1; ++c0) epi_prefetch_res<MAP>(g, mb + c0 * 8, nb, lane, ring[c0]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = i * 4 + q;
            if (pf && c + RD - 1 < 16) epi_prefetch_res<MAP>(g, mb + (c + RD - 1) * 8, nb, lane, ring[(c + RD - 1) % RD]);
            float* st = stage + (c & 1) * 512;
            stage_chunk(st, acc[i][0], acc[i][1], q);
            epi_rows16<T, ACT, MAP, FAST, 2>(g, st, mb + c * 8, nb, lane, bias, pf ? ring[c % RD] : nullptr);
          }
        }
      };
      const bool fast = epi_fast_ok(g, mb, 128, nb);
      bool c16 = false;
      if constexpr (sizeof(T) == 2 && MAP == ALPRO_MAP_IDENTITY)
        c16 = fast && g.c_dtype != ALPRO_F32 && ((g.ldc & 7) == 0) && (!g.C2 || (g.ldc2 & 7) == 0) && (!g.row_scale || g.row_scale_group >= 8);
      if (c16) {
        if constexpr (sizeof(T) == 2 && MAP == ALPRO_MAP_IDENTITY) {
          float bias8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) bias8[e] = g.bias ? g.bias[nb + (lane & 7) * 8 + e] : 0.f;
          // GELU_BWD: the saved pre-activation rows are fetched two chunks ahead of their use (same reason as the residual)
          u32x4 pring[3];
          auto load_pre = [&](int c) {
            return __builtin_nontemporal_load((const u32x4*)((const T*)g.C2 + (int64_t)(mb + c * 8 + (lane >> 3)) * g.ldc2 + nb + (lane & 7) * 8));
          };
          constexpr bool READS_C2 = ACT == ALPRO_ACT_GELU_BWD || ACT == ALPRO_ACT_MUL_SAVED;
          if (READS_C2) {
            pring[0] = load_pre(0);
            pring[1] = load_pre(1);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int c = i * 4 + q;
              if (READS_C2 && c + 2 < 16) pring[(c + 2) % 3] = load_pre(c + 2);
              float* st = stage + (c & 1) * 512;
              stage_chunk(st, acc[i][0], acc[i][1], q);
              epi_rows16_c16<T, ACT, 1>(g, st, mb + c * 8, nb, lane, bias8, READS_C2 ? &pring[c % 3] : nullptr);
            }
          }
        }
      } else if (fast) {
        run_epilogue(std::true_type{});
      } else {
        run_epilogue(std::false_type{});
      }
    }
    if (!more) break;
    tile = next;
    hf = next_hf;
    ++it;
    setup(tile, hf);  // recomputed (not kept live): frees the 16 source-pointer registers across the epilogue
  }
}
}  // namespace
}  // namespace alpro
