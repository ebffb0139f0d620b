// NT GEMM with fused epilogue for gfx950:  C = epilogue(A[M,K] * W[N,K]^T) -- host dispatch and C ABI.  The kernels: gemm_nt128_kernels.hpp
// (128 x 128 tile, register-staged), gemm_nt256p_kernels.hpp (persistent 256 x 256), gemm_nt256q_kernels.hpp (8-phase 256 x 256).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "gemm_nt128_kernels.hpp"
#include "gemm_nt256p_kernels.hpp"
#include "gemm_nt256q_kernels.hpp"

namespace alpro {

namespace {
// Would launch_gemm send this descriptor to the 8-phase kernel (gemm_nt256q_kernel)?  Eligible: 16-bit operands, identity map, 16-bit output
// through the 16-byte-store epilogue or fp32 output through the fp32 one, whole 256-column tiles, 128-byte-aligned operand rows, an even number
// >= 4 of 64-deep K-tiles, 32-bit operand offsets, >= 160 whole tiles (below that the 128 x 128 kernel fills the chip better).
// Ragged M: when the remainder is a multiple of 16 rows the kernel takes the partial tile row itself (invalid copy pieces re-read valid rows,
// the epilogue skips rows beyond M) -- ONE launch; the round-4 first form ran the remainder as a second launch on the 128 x 128 kernel: 46
// launches of ~46 us per training step at B = 64 (M = 100416 = 392 * 256 + 64), serialised behind the main kernel.  Other remainders still
// take that split (the remainder launch carries m_off: row scale / dropout index by absolute row).
static bool q_kernel_takes(const alpro_gemm_desc_t& g, bool* ragged_in_kernel) {
  constexpr int BM2q = 256, BN2q = 256;
  if (g.dtype == ALPRO_F32 || g.map_mode != ALPRO_MAP_IDENTITY) return false;
  const int m_full = g.M / BM2q * BM2q, m_rem = g.M - m_full;
  const bool c16 = g.c_dtype != ALPRO_F32 && (g.ldc & 7) == 0 && (!g.C2 || g.c2_tiled || (g.ldc2 & 7) == 0) && (!g.residual || (g.ldr & 3) == 0) && ((uintptr_t)g.C % 16) == 0 &&
                   (!g.row_scale || g.row_scale_group >= 8);   // (a pass of 8 rows takes its scales from at most two groups: epi_rows16_c16)
  const bool c32 = g.c_dtype == ALPRO_F32 && g.act == ALPRO_ACT_NONE && !g.C2 && !g.drop_seed && (g.ldc & 3) == 0 && (!g.residual || ((g.ldr & 3) == 0 && ((uintptr_t)g.residual % 16) == 0)) &&
                   ((uintptr_t)g.C % 16) == 0 && (!g.row_scale || g.row_scale_group >= 16);   // (the fp32 epilogue takes a fragment row's scales from at most two groups)
  const bool shape = (g.N % BN2q) == 0 && ((g.lda * 2) % 128) == 0 && ((g.ldw * 2) % 128) == 0 && (g.K % 128) == 0 && g.K >= 256 &&
                     (int64_t)g.M * g.lda * 2 < (int64_t)0xFFFF0000 && (int64_t)g.N * g.ldw * 2 < (int64_t)0xFFFF0000;
  *ragged_in_kernel = m_rem > 0 && (m_rem % 16) == 0;
  const int full_tiles = (g.N / BN2q) * (m_full / BM2q);
  const int force = get_option(OPT_GEMM_TILE);
  return get_option(OPT_GEMM_KIND) == 1 && (c16 || c32) && shape && (force ? force == 256 : full_tiles >= 160);
}
// ... and may its C2 buffer be in the tile layout (alpro_hip.h: c2_tiled)?  Every tile of the output must go through the kernel's packed
// epilogue: the GELU_SAVE_GRAD / MUL_SAVED pair without anything that epilogue does not do, and no second launch for a remainder.
static bool c2_tiled_ok(const alpro_gemm_desc_t& g) {
  const int m_rem = g.M % 256;
  return (g.act == ALPRO_ACT_GELU_SAVE_GRAD || g.act == ALPRO_ACT_MUL_SAVED) && g.C2 && ((uintptr_t)g.C2 % 16) == 0 && g.c_dtype != ALPRO_F32 && !g.residual && !g.row_scale &&
         !g.drop_seed && (m_rem % 16) == 0;
}

template <typename T, int ACT, int MAP>
int launch_gemm_inst(const alpro_gemm_desc_t& g, hipStream_t st) {
  constexpr bool TUNABLE = std::is_same<T, bf16_t>::value && ACT == ALPRO_ACT_NONE && MAP == ALPRO_MAP_IDENTITY;   // (gemm_tune 0 / 2 exist for this form only)
  constexpr size_t LDS_P = 4 * TILE2_BYTES + EPI_BYTES;
  static DeviceOnce once_nt, once_p, once_p2;
  set_lds_once(once_nt, gemm_nt_kernel<T, ACT, MAP>, 4 * TILE_BYTES);
  set_lds_once(once_p, gemm_nt256p_kernel<T, ACT, MAP>, LDS_P);
  if constexpr (TUNABLE) set_lds_once(once_p2, gemm_nt256p_kernel<T, ACT, MAP, 2>, LDS_P);
  const int big_tiles = ((g.N + BN2 - 1) / BN2) * ((g.M + BM2 - 1) / BM2);
  const int force = get_option(OPT_GEMM_TILE);
  const int nk = (g.K * (int)sizeof(T)) / ROWB;
  // the persistent 256^2 kernel wins from ~160 tiles up (measured, tools/gemm_bert_bench.py: M=15168 N=768 = 180 tiles is 15-25 % faster than on the 128^2 kernel; M=2560 N=3072 = 120 tiles is not); its pipeline needs >= 2 K-tiles
  const bool use256 = nk >= 2 && (force ? force == 256 : big_tiles >= 160);
  if constexpr (sizeof(T) == 2 && MAP == ALPRO_MAP_IDENTITY) {
    // round 4: the 8-phase two-group schedule (gemm_nt256q_kernel) for the identity-map shapes; needs an even number >= 4 of 64-deep K-tiles
    // and 32-bit operand offsets.  gemm_kind 0 = the round-3 kernel (A/B), 1 = the 8-phase kernel
    static DeviceOnce once_q;
    set_lds_once(once_q, gemm_nt256q_kernel<T, ACT, MAP>, 2 * STAGE2_BYTES + EPI_BYTES);
    // eligible: 16-bit output through the 16-byte-store epilogue, whole 256-column tiles, 128-byte-aligned operand rows, an even number >= 4 of
    // K-tiles; a ragged M (the ViT's B * 1569 token rows: M % 256 = 64) is split -- whole tiles here, the remaining rows on the 128 x 128 kernel
    // in a second launch -- when the epilogue does not index by absolute row (row scale, dropout)
    const int m_full = g.M / BM2 * BM2, m_rem = g.M - m_full;
    bool ragged_in_kernel = false;
    const bool take_q = q_kernel_takes(g, &ragged_in_kernel);
    ALPRO_CHECK(!g.c2_tiled || (take_q && c2_tiled_ok(g)), "alpro_gemm: c2_tiled is not available for this descriptor (M=%d N=%d K=%d act=%d): ask alpro_gemm_c2_tiled_rows first", g.M, g.N, g.K, g.act);
    if (take_q) {
      alpro_gemm_desc_t gq = g;
      if (!ragged_in_kernel) gq.M = m_full;
      // one workgroup per CU the launch may count on, whatever the tile count: the per-XCD lists are chunks of 32 tiles, and a workgroup
      // whose list (and, dynamic walk, every other list) is empty returns at once
      int grid = cu_budget(st);
      if (const int cap = get_option(OPT_GEMM_GRID)) grid = cap < grid ? (cap + 7) / 8 * 8 : grid;
      // Tail hand-over (round 6, option gemm_tail; VERDICT r3-r5 "the last partial round of the N = 768 projections").  With tiles = Q * grid + R
      // and a small R the last round keeps R workgroups busy for a whole tile time while the others idle -- at B = 32: the N = 768 projections
      // 588 / 591 tiles = 2.3 rounds, fc1 2352 = 9.19, fc2 588 (K = 3072).  A two-group 8-phase tile cannot be cut (a half tile takes as long as
      // a whole one: DESIGN.md), and split-K pays 256 KiB of fp32 partials per tile at K = 768.  What does work: the row panels that make up
      // the partial round go to the 128 x 128 kernel as a SECOND launch -- 4 R small tiles, two workgroups per CU, one short round behind the
      // Q full ones -- when R <= 0.4 grid (beyond that the small kernel's lower rate eats the saving) AND K >= 2048.  Measured (MI355X, fp16, B = 32,
      // tools/gemm_tail_ab.py, profiles/r6_gemm_tail_handover.txt): fc2 (K = 3072, 591 tiles) 274 -> 261 us (-4.7 %); the K = 768 projections
      // 74.4 -> 75.3 / 70.2 -> 71.2 us and fc1 (2364 tiles) 242 -> 239: the small kernel runs 304 tiles of 128 x 128 x 768 at ~300 TF/s, i.e. as
      // long as the round it replaces -- at K = 768 a tile is mostly epilogue and fill, and there the hand-over is NOT taken.  Same arithmetic per
      // element, different summation order inside the MFMAs: not bitwise equal to the unsplit launch (tests pin both against fp64),
      // bit-reproducible run to run.
      const int ntn_q = g.N / BN2, ntm_q = (gq.M + BM2 - 1) / BM2;
      const int tiles = ntn_q * ntm_q;
      int tail_panels = 0;
      if (get_option(OPT_GEMM_TAIL) == 1 && !g.c2_tiled && tiles > grid && g.K >= 2048) {
        const int R = tiles % grid;
        if (R > 0 && 5 * R <= 2 * grid) tail_panels = (R + ntn_q - 1) / ntn_q;
      }
      int64_t m_tail0 = -1;   // first row of what the second launch computes (-1: nothing)
      if (tail_panels > 0 && tail_panels < ntm_q) {
        m_tail0 = (int64_t)(ntm_q - tail_panels) * BM2;
        gq.M = (int)m_tail0;
      } else if (m_rem && !ragged_in_kernel) {
        m_tail0 = m_full;
      }
      TileSched sc;
      sc.blk = sc.prev = nullptr;
      sc.magic_ntn = magic_u32((uint32_t)(g.N / BN2));
      sc.epi = (uint32_t)get_option(OPT_GEMM_EPI);
      {
        SchedLaunch blocks(get_option(OPT_GEMM_SCHED) == 1 ? st : nullptr, get_option(OPT_GEMM_SCHED) == 1);   // (holds the stream's block pair until the launch is enqueued)
        sc.blk = blocks.cur;
        sc.prev = blocks.prev;
        hipLaunchKernelGGL((gemm_nt256q_kernel<T, ACT, MAP>), dim3(grid), dim3(NT2), 2 * STAGE2_BYTES + EPI_BYTES, st, gq, sc);
        blocks.commit(hipPeekAtLastError() == hipSuccess);
      }
      if (m_tail0 >= 0) {
        alpro_gemm_desc_t gr = g;
        gr.M = (int)(g.M - m_tail0);
        gr.A = (const char*)g.A + m_tail0 * g.lda * 2;
        gr.C = (char*)g.C + m_tail0 * g.ldc * (g.c_dtype == ALPRO_F32 ? 4 : 2);
        gr.m_off = g.m_off + m_tail0;
        if (g.C2) gr.C2 = (char*)g.C2 + m_tail0 * g.ldc2 * 2;
        if (g.residual) gr.residual = g.residual + m_tail0 * g.ldr;
        const int ntn = (gr.N + BN - 1) / BN, ntm = (gr.M + BM - 1) / BM;
        hipLaunchKernelGGL((gemm_nt_kernel<T, ACT, MAP>), dim3(ntn * ntm), dim3(NT), 4 * TILE_BYTES, st, gr);
      }
      return check_launch("alpro_gemm");
    }
  }
  if (use256) {
    const int cus = cu_budget(st);
    int grid = big_tiles < cus ? (big_tiles + 7) / 8 * 8 : cus;  // multiple of 8: the XCD-contiguous slot map must be a bijection
    if (const int cap = get_option(OPT_GEMM_GRID)) grid = cap < grid ? (cap + 7) / 8 * 8 : grid;  // tuning aid: cap the persistent grid
    const int tune = get_option(OPT_GEMM_TUNE);
    const int tail = get_option(OPT_GEMM_TAIL);
    auto kern = gemm_nt256p_kernel<T, ACT, MAP>;
    if constexpr (TUNABLE) kern = tune == 0 ? gemm_nt256p_kernel<T, ACT, MAP, 0> : tune == 2 ? gemm_nt256p_kernel<T, ACT, MAP, 2> : kern;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT2), LDS_P, st, g, tail);
  } else {
    const int ntn = (g.N + BN - 1) / BN, ntm = (g.M + BM - 1) / BM;
    hipLaunchKernelGGL((gemm_nt_kernel<T, ACT, MAP>), dim3(ntn * ntm), dim3(NT), 4 * TILE_BYTES, st, g);
  }
  return check_launch("alpro_gemm");
}

// activation and row map are compile-time (keeps each kernel's epilogue small); activations only combine
// with the identity map on this path (fc1 / BERT intermediate / MLM transform / mpm_head)
template <typename T>
int launch_gemm(const alpro_gemm_desc_t& g, hipStream_t st) {
#ifdef ALPRO_ISA_QUICK   // tools/isa_quick.sh: two instantiations per dtype instead of nine (register-pressure iterations on the 8-phase kernel; never the product build)
  return g.act == ALPRO_ACT_MUL_SAVED ? launch_gemm_inst<T, ALPRO_ACT_MUL_SAVED, ALPRO_MAP_IDENTITY>(g, st) : launch_gemm_inst<T, ALPRO_ACT_NONE, ALPRO_MAP_IDENTITY>(g, st);
#else
  if (g.act != ALPRO_ACT_NONE) {
    if (g.map_mode != ALPRO_MAP_IDENTITY) {
      set_error("alpro_gemm: an activation cannot be combined with a row map");
      return ALPRO_ERR_INVALID;
    }
    if (g.act == ALPRO_ACT_GELU_BWD) return launch_gemm_inst<T, ALPRO_ACT_GELU_BWD, ALPRO_MAP_IDENTITY>(g, st);
    if (g.act == ALPRO_ACT_GELU_SAVE_GRAD) return launch_gemm_inst<T, ALPRO_ACT_GELU_SAVE_GRAD, ALPRO_MAP_IDENTITY>(g, st);
    if (g.act == ALPRO_ACT_MUL_SAVED) return launch_gemm_inst<T, ALPRO_ACT_MUL_SAVED, ALPRO_MAP_IDENTITY>(g, st);
    return g.act == ALPRO_ACT_GELU ? launch_gemm_inst<T, ALPRO_ACT_GELU, ALPRO_MAP_IDENTITY>(g, st)
                                   : launch_gemm_inst<T, ALPRO_ACT_RELU, ALPRO_MAP_IDENTITY>(g, st);
  }
  switch (g.map_mode) {
    case ALPRO_MAP_IDENTITY: return launch_gemm_inst<T, ALPRO_ACT_NONE, ALPRO_MAP_IDENTITY>(g, st);
    case ALPRO_MAP_SKIP_CLS: return launch_gemm_inst<T, ALPRO_ACT_NONE, ALPRO_MAP_SKIP_CLS>(g, st);
    case ALPRO_MAP_FRAME_TOKENS: return launch_gemm_inst<T, ALPRO_ACT_NONE, ALPRO_MAP_FRAME_TOKENS>(g, st);
    default: return launch_gemm_inst<T, ALPRO_ACT_NONE, ALPRO_MAP_PATCH_EMBED>(g, st);
  }
#endif
}

template <typename T>
int launch_gemm_batch(const alpro_gemm_desc_t* descs_dev, int njobs, int max_tiles, hipStream_t st) {
  static DeviceOnce once;
  set_lds_once(once, gemm_nt_batch_kernel<T, ALPRO_ACT_NONE, ALPRO_MAP_IDENTITY>, 4 * TILE_BYTES);
  hipLaunchKernelGGL((gemm_nt_batch_kernel<T, ALPRO_ACT_NONE, ALPRO_MAP_IDENTITY>), dim3(max_tiles, njobs), dim3(NT), 4 * TILE_BYTES, st, descs_dev);
  return check_launch("alpro_gemm_batch");
}
}  // namespace
}  // namespace alpro

static int check_gemm_desc(const alpro_gemm_desc_t* d);

extern "C" int alpro_gemm_batch(const alpro_gemm_desc_t* descs_host, const alpro_gemm_desc_t* descs_device, int njobs, void* stream) {
  using namespace alpro;
  ALPRO_CHECK(descs_host && descs_device && njobs > 0, "alpro_gemm_batch: bad args");
  int max_tiles = 0;
  for (int i = 0; i < njobs; ++i) {
    const alpro_gemm_desc_t* d = descs_host + i;
    if (const int rc = check_gemm_desc(d)) return rc;
    ALPRO_CHECK(d->dtype == descs_host[0].dtype, "alpro_gemm_batch: all jobs must share the operand dtype");
    ALPRO_CHECK(d->act == ALPRO_ACT_NONE && d->map_mode == ALPRO_MAP_IDENTITY && !d->drop_seed && !d->bias2 && !d->C2,
                "alpro_gemm_batch: plain epilogues only (bias, alpha, row scale, fp32 residual)");
    const int t = ((d->N + BN - 1) / BN) * ((d->M + BM - 1) / BM);
    max_tiles = t > max_tiles ? t : max_tiles;
  }
  ALPRO_DISPATCH_DTYPE(descs_host[0].dtype, T, return launch_gemm_batch<T>(descs_device, njobs, max_tiles, (hipStream_t)stream));
  return ALPRO_OK;
}

static int check_gemm_desc(const alpro_gemm_desc_t* d) {
  using namespace alpro;
  ALPRO_CHECK(d && d->A && d->W && d->C, "alpro_gemm: null operand");
  ALPRO_CHECK(d->M > 0 && d->N > 0 && d->K > 0, "alpro_gemm: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
  const int esz = d->dtype == ALPRO_F32 ? 4 : 2;
  ALPRO_CHECK((d->K * esz) % 128 == 0, "alpro_gemm: K=%d must be a multiple of %d for dtype %d", d->K, 128 / esz, d->dtype);
  ALPRO_CHECK((d->lda * esz) % 16 == 0 && (d->ldw * esz) % 16 == 0, "alpro_gemm: lda/ldw must keep rows 16-byte aligned");
  ALPRO_CHECK(((uintptr_t)d->A % 16) == 0 && ((uintptr_t)d->W % 16) == 0, "alpro_gemm: A/W must be 16-byte aligned");
  ALPRO_CHECK(d->c_dtype == d->dtype || d->c_dtype == ALPRO_F32, "alpro_gemm: c_dtype must be dtype or F32");
  ALPRO_CHECK(d->map_mode >= 0 && d->map_mode <= 3, "alpro_gemm: bad map_mode %d", d->map_mode);
  ALPRO_CHECK(d->act >= 0 && d->act <= ALPRO_ACT_MUL_SAVED, "alpro_gemm: bad act %d", d->act);
  ALPRO_CHECK(!d->bias2 || d->map_mode == ALPRO_MAP_SKIP_CLS, "alpro_gemm: bias2 is only defined under the SKIP_CLS map");
  ALPRO_CHECK((d->act != ALPRO_ACT_GELU_BWD && d->act != ALPRO_ACT_MUL_SAVED && d->act != ALPRO_ACT_GELU_SAVE_GRAD) || (d->C2 && d->N % 8 == 0 && (d->c2_tiled || d->ldc2 % 8 == 0)),
              "alpro_gemm: GELU_BWD / MUL_SAVED / GELU_SAVE_GRAD need the C2 buffer (N, ldc2 multiples of 8)");
  ALPRO_CHECK(!d->drop_seed || (d->map_mode == ALPRO_MAP_IDENTITY && d->drop_p > 0.f && d->drop_p < 1.f), "alpro_gemm: dropout needs the identity map and 0 < p < 1");
  ALPRO_CHECK(!d->C2 || (d->N % 4 == 0 && (d->c2_tiled || d->ldc2 % 4 == 0) && d->ldc % 4 == 0), "alpro_gemm: C2 needs N, ldc, ldc2 multiples of 4");
  ALPRO_CHECK(!d->c2_tiled || d->act == ALPRO_ACT_GELU_SAVE_GRAD || d->act == ALPRO_ACT_MUL_SAVED, "alpro_gemm: c2_tiled is for GELU_SAVE_GRAD / MUL_SAVED only");
  ALPRO_CHECK(d->map_mode != ALPRO_MAP_FRAME_TOKENS || d->side, "alpro_gemm: FRAME_TOKENS needs a side buffer");
  ALPRO_CHECK(!d->row_scale || d->row_scale_group > 0, "alpro_gemm: row_scale_group must be > 0");
  return ALPRO_OK;
}

extern "C" int64_t alpro_gemm_c2_tiled_rows(int64_t M, int64_t N, int64_t K, int dtype) {
  using namespace alpro;
  if (M <= 0 || N <= 0 || K <= 0 || M > 0x7fffffff || N > 0x7fffffff || K > 0x7fffffff || (dtype != ALPRO_F16 && dtype != ALPRO_BF16)) return 0;
  alpro_gemm_desc_t g = {};
  g.A = g.W = (const void*)(uintptr_t)256;   // (never dereferenced: alignment only)
  g.C = g.C2 = (void*)(uintptr_t)256;
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.lda = g.ldw = K; g.ldc = N;
  g.dtype = g.c_dtype = dtype;
  g.act = ALPRO_ACT_GELU_SAVE_GRAD;
  g.c2_tiled = 1;
  bool ragged = false;
  return (q_kernel_takes(g, &ragged) && c2_tiled_ok(g)) ? (M + 255) / 256 * 256 : 0;
}

extern "C" int alpro_gemm(const alpro_gemm_desc_t* d, void* stream) {
  using namespace alpro;
  if (const int rc = check_gemm_desc(d)) return rc;
#ifdef ALPRO_ISA_QUICK
  return launch_gemm<f16_t>(*d, (hipStream_t)stream);
#else
  ALPRO_DISPATCH_DTYPE(d->dtype, T, return launch_gemm<T>(*d, (hipStream_t)stream));
  return ALPRO_OK;
#endif
}
