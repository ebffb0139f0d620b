// Attention backward for gfx950 (head_dim 64): dQ, dK, dV from dO with the softmax recomputed from the saved
// row log-sum-exp.  Same MFMA formulation as the forward (attention.hip): every product keeps its contraction
// index in registers by choosing the orientation per product, so no accumulator ever crosses lanes.
//
//   phase 1 (K, V tiles resident in LDS; one 32-query tile per wave; lane = query)
//       S^T = K Q^T, dP^T = V dO^T                  A = rows of K / V (ds_read_b128), B = Q / dO rows (registers)
//       P^T = exp(S^T*scale + bias - lse[q]),  dS^T = P^T o (dP^T - delta[q]) * scale,  delta = rowsum(dO o O)
//       dQ^T = K^T dS^T                             A = K^T via ds_read_b64_tr_b16, B = dS^T straight from registers
//   phase 2 (Q, dO tiles re-staged into the same LDS; one 32-key tile per wave; lane = key)
//       S = Q K^T, dP = dO V^T                      A = rows of Q / dO, B = K / V rows of the key tile (registers)
//       dV^T += dO^T P,  dK^T += Q^T dS             A = dO^T / Q^T via transpose reads, B = P / dS from registers
// The LDS tiles are U tiles (attn_tile.hpp): one swizzle serves the row reads and the transpose reads.  The temporal variant
// treats 32 consecutive tokens as one tile with a block-diagonal group mask (one wave per workgroup).
#include "common.hpp"
#include "attn_tile.hpp"

namespace alpro {
namespace {

template <typename T>
__device__ __forceinline__ void stage_tile(char* tile, const T* src, int64_t ld, int rows_valid, int LP, int tid, int nthreads) {
  typedef TileCfg<T> C;
  for (int c = tid; c < LP * C::CPR; c += nthreads) {
    const int row = c / C::CPR, ch = c - row * C::CPR;
    u32x4 v = mk4(0, 0, 0, 0);
    if (row < rows_valid) v = *(const u32x4*)(src + (int64_t)row * ld + ch * C::CN);
    *(u32x4*)(tile + tile_off<T>(row, ch)) = v;
  }
}


// ================================================================================================
// 16-bit full-attention backward, throughput form (same two phases and MFMA orientations as attn_bwd_kernel):
//  * tiles go global -> LDS by DMA with the swizzle applied on the source side; padded rows read a zero page;
//  * exp2 with log2(e) folded into the score scale; LDS holds -lse*log2(e) (or -inf for padded queries, which makes
//    their P rows exactly 0) and delta*scale, so a score costs FMA + v_exp_f32 and a dS costs FMA + MUL;
//  * the next query tile's Q / dO / O fragments are prefetched under the current tile's work (phase 1);
//  * dQ, dK, dV tiles are transposed through 4 KiB of wave-private LDS and leave as 16-byte row stores;
//  * <= 256 registers and ~76 KiB of LDS: two workgroups per CU.
__device__ u32x4 g_bwd_zero[4];

// wave-private transpose: accumulator pair (column = token of this lane, rows = d) -> 32 row-major 128-byte rows.
// HALF: 2 KiB of staging instead of 4 -- the two 32-wide d halves go one after the other as 64-byte row pieces (used where
// the full staging would push the workgroup over half of the CU's LDS, i.e. 8 key tiles).
template <typename T, bool HALF = false>
__device__ __forceinline__ void store_rows_via_lds(char* Ow, const f32x16 (&o)[2], T* dst, int64_t ld, int row_base, int rows_valid, int lane) {
  const int g = lane >> 5, ql = lane & 31;
  if constexpr (!HALF) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const uint32_t lo = pack2(o[dt][4 * rq], o[dt][4 * rq + 1], (T*)0);
        const uint32_t hi = pack2(o[dt][4 * rq + 2], o[dt][4 * rq + 3], (T*)0);
        *(u32x2*)(Ow + ql * 128 + (((dt * 4 + rq) ^ ((ql >> 1) & 7)) << 4) + g * 8) = mk2(lo, hi);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = p * 8 + (lane >> 3), slot = lane & 7;
      const u32x4 v = *(const u32x4*)(Ow + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
      if (row_base + row < rows_valid) __builtin_nontemporal_store(v, (u32x4*)(dst + (int64_t)(row_base + row) * ld + slot * 8));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staging rows may be rewritten right away
  } else {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const uint32_t lo = pack2(o[dt][4 * rq], o[dt][4 * rq + 1], (T*)0);
        const uint32_t hi = pack2(o[dt][4 * rq + 2], o[dt][4 * rq + 3], (T*)0);
        *(u32x2*)(Ow + ql * 64 + ((rq ^ ((ql >> 2) & 3)) << 4) + g * 8) = mk2(lo, hi);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int row = p * 16 + (lane >> 2), slot = lane & 3;
        const u32x4 v = *(const u32x4*)(Ow + row * 64 + ((slot ^ ((row >> 2) & 3)) << 4));
        if (row_base + row < rows_valid) __builtin_nontemporal_store(v, (u32x4*)(dst + (int64_t)(row_base + row) * ld + dt * 32 + slot * 8));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

template <typename T, int NKT, bool HAS_BIAS, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_bwd16_kernel(const T* __restrict__ qkv, const T* __restrict__ out,
                                                                          const T* __restrict__ dout, const float* __restrict__ lse,
                                                                          T* __restrict__ dqkv, int L, int H, float scale,
                                                                          const float* __restrict__ key_bias, float drop_p, uint32_t drop_seed, int order) {
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int LP = NKT * 32, RB = 128;
  constexpr bool HALF = NKT == 8;             // 8 key tiles: 2 KiB staging per wave keeps two workgroups per CU (2 x 75 KiB)
  constexpr int OW = HALF ? 2048 : 4096;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* tA = smem;              // K, then Q
  char* tB = smem + LP * RB;    // V, then dO
  char* Os = smem + 2 * LP * RB;
  float* Bs = (float*)(Os + 4 * OW);  // key bias * log2(e); -inf on padded keys
  float* Ls = Bs + LP;                   // -lse * log2(e); -inf on padded queries
  float* Ds = Ls + LP;                   // delta * scale
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int b, h;
  attn_unit(blockIdx.x, gridDim.x, H, order, b, h);
  const int64_t row0 = (int64_t)b * L;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const T* qb = qkv + row0 * ldq + h * HD;
  const T* ob = out + row0 * ldo + h * HD;
  const T* dob = dout + row0 * ldo + h * HD;
  T* db = dqkv + row0 * ldq + h * HD;
  const float* lse_b = lse + ((int64_t)b * H + h) * L;
  const uint32_t dth = drop_thresh24(drop_p);
  const float dks = drop_seed ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t dbase = ((uint64_t)b * H + h) * (uint64_t)L;  // + q, then * L + key
  const float sl = scale * LOG2E;
  for (int c = tid; c < LP; c += 256) {
    Bs[c] = c < L ? (HAS_BIAS ? key_bias[(int64_t)b * L + c] * LOG2E : 0.f) : -INFINITY;
    Ls[c] = c < L ? -lse_b[c] * LOG2E : -INFINITY;
  }
  const uint32_t a_lds = lds_addr_of(tA), b_lds = lds_addr_of(tB);
  const char* zero = (const char*)g_bwd_zero;
  // two row-major (row, 64) tiles -> LDS images, chunk ^ (bit1(row) << 2 | (row >> 2) & 3)
  auto stage2 = [&](const T* srcA, int64_t lda_, const T* srcB, int64_t ldb_) {
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
      const int piece = wave + 4 * i;
      const int row = piece * 8 + (lane >> 3), slot = lane & 7;
      const int ch = slot ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
      const char* pa = row < L ? (const char*)(srcA + (int64_t)row * lda_ + ch * 8) : zero;
      const char* pb = row < L ? (const char*)(srcB + (int64_t)row * ldb_ + ch * 8) : zero;
      dma16(pa, __builtin_amdgcn_readfirstlane(a_lds + piece * 1024));
      dma16(pb, __builtin_amdgcn_readfirstlane(b_lds + piece * 1024));
    }
  };
  stage2(qb + H * HD, ldq, qb + 2 * H * HD, ldq);

  const int g = lane >> 5, ql = lane & 31;
  const int ntile = (L + 31) >> 5;
  char* Ow = Os + wave * OW;
  // ---------------------------------------------------------------- phase 1: dQ (lane = query)
  auto load_q3 = [&](int qt, u32x4(&qf)[4], u32x4(&dof)[4], u32x4(&of)[4]) {
    const int qc = min(qt * 32 + ql, L - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int off = (2 * ks + g) * 8;
      qf[ks] = *(const u32x4*)(qb + (int64_t)qc * ldq + off);
      dof[ks] = *(const u32x4*)(dob + (int64_t)qc * ldo + off);
      of[ks] = *(const u32x4*)(ob + (int64_t)qc * ldo + off);
    }
  };
  u32x4 qf[4], dof[4], of[4];
  load_q3(min(wave, ntile - 1), qf, dof, of);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int qt = wave; qt < ntile; qt += 4) {
    const int q = qt * 32 + ql;
    const int qc = min(q, L - 1);
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      float a[8], c2[8];
      unpack_chunk<T>(dof[ks], a);
      unpack_chunk<T>(of[ks], c2);
#pragma unroll
      for (int e = 0; e < 8; ++e) delta += a[e] * c2[e];
    }
    delta += __shfl_xor(delta, 32, 64);
    const float nds = -delta * scale;
    const float nlq = Ls[q];
    if (g == 0) Ds[q] = nds;
    u32x4 qn[4], don[4], on[4];
    f32x16 dq[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt < ntile) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
        const int krow = kt * 32 + ql;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const u32x4 ka = *(const u32x4*)(tA + tile_off<T>(krow, 2 * ks + g));
          const u32x4 va = *(const u32x4*)(tB + tile_off<T>(krow, 2 * ks + g));
          mma_chunk<T>(s, ka, qf[ks]);
          mma_chunk<T>(dp, va, dof[ks]);
        }
        if (kt == 0) load_q3(min(qt + 4, ntile - 1), qn, don, on);  // lands under this tile's work
        const bool plain = !HAS_BIAS && (kt + 1) * 32 <= L;          // all 32 keys valid, no bias
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          float bb[4] = {nlq, nlq, nlq, nlq};
          if (!plain) {
            const float4 bq = *(const float4*)(Bs + kt * 32 + 8 * rq + 4 * g);
            bb[0] += bq.x; bb[1] += bq.y; bb[2] += bq.z; bb[3] += bq.w;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rq + e;
            const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sl, bb[e]));
            float gd = dp[r];
            if constexpr (DROP) gd = drop_keep(drop_seed, (dbase + qc) * L + kt * 32 + 8 * rq + 4 * g + e, dth) ? gd * dks : 0.f;
            s[r] = p * fmaf(gd, scale, nds);  // dS^T = P o (dP - delta) * scale
          }
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = s[cc * 8 + e];
          const u32x4 bop = pack_chunk<T>(v);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(dq[dt], load_t_chunk<T>(tA, kt * 32, cc, lane, dt), bop);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    store_rows_via_lds<T, HALF>(Ow, dq, db, ldq, qt * 32, L, lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = qn[ks];
      dof[ks] = don[ks];
      of[ks] = on[ks];
    }
  }
  __syncthreads();
  // ---------------------------------------------------------------- phase 2: dK, dV (lane = key)
  stage2(qb, ldq, dob, ldo);
  u32x4 kf[4], vf[4];
  {
    const int kc = min(min(wave, ntile - 1) * 32 + ql, L - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int off = (2 * ks + g) * 8;
      kf[ks] = *(const u32x4*)(qb + (int64_t)kc * ldq + H * HD + off);
      vf[ks] = *(const u32x4*)(qb + (int64_t)kc * ldq + 2 * H * HD + off);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = wave; kt < ntile; kt += 4) {
    const int key = kt * 32 + ql;
    if (kt != wave) {
      const int kc = min(key, L - 1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int off = (2 * ks + g) * 8;
        kf[ks] = *(const u32x4*)(qb + (int64_t)kc * ldq + H * HD + off);
        vf[ks] = *(const u32x4*)(qb + (int64_t)kc * ldq + 2 * H * HD + off);
      }
    }
    const float kb = HAS_BIAS ? Bs[key] : 0.f;
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;
#pragma unroll 1
    for (int qt = 0; qt < ntile; ++qt) {
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
      const int qrow = qt * 32 + ql;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const u32x4 qa = *(const u32x4*)(tA + tile_off<T>(qrow, 2 * ks + g));
        const u32x4 da = *(const u32x4*)(tB + tile_off<T>(qrow, 2 * ks + g));
        mma_chunk<T>(s, qa, kf[ks]);
        mma_chunk<T>(dp, da, vf[ks]);
      }
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const float4 lq = *(const float4*)(Ls + qt * 32 + 8 * rq + 4 * g);
        const float4 dq4 = *(const float4*)(Ds + qt * 32 + 8 * rq + 4 * g);
        float ll[4] = {lq.x, lq.y, lq.z, lq.w};
        const float dd[4] = {dq4.x, dq4.y, dq4.z, dq4.w};
        if (HAS_BIAS) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ll[e] += kb;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * rq + e;
          const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sl, ll[e]));
          float gd = dp[r], pm = p;
          if constexpr (DROP) {
            const int qq = qt * 32 + 8 * rq + 4 * g + e;
            const bool keep = drop_keep(drop_seed, (dbase + (qq < L ? qq : L - 1)) * L + key, dth);
            pm = keep ? p * dks : 0.f;
            gd = keep ? gd * dks : 0.f;
          }
          s[r] = pm;                          // dropped P (feeds dV)
          dp[r] = p * fmaf(gd, scale, dd[e]);  // dS
        }
      }
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        float pv[8], sv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          pv[e] = s[cc * 8 + e];
          sv[e] = dp[cc * 8 + e];
        }
        const u32x4 pb = pack_chunk<T>(pv), sb = pack_chunk<T>(sv);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          mma_chunk<T>(dv[dt], load_t_chunk<T>(tB, qt * 32, cc, lane, dt), pb);
          mma_chunk<T>(dk[dt], load_t_chunk<T>(tA, qt * 32, cc, lane, dt), sb);
        }
      }
    }
    store_rows_via_lds<T, HALF>(Ow, dk, db + H * HD, ldq, kt * 32, L, lane);
    store_rows_via_lds<T, HALF>(Ow, dv, db + 2 * H * HD, ldq, kt * 32, L, lane);
  }
}

// ================================================================================================
// Key-owned 16-bit backward for 5..8 key tiles (ViT spatial L = 197, fusion L = 237): every (query tile, key tile)
// pair is computed ONCE.  The two-phase kernel above evaluates S, dP, P and dS of every pair twice (once per
// orientation, 28 MFMAs + 2 x 16 exp per pair); here wave w owns key tile w for the whole unit (K / V fragments and
// the dK^T / dV^T accumulators stay in its registers) and walks the query tiles in lockstep with the other waves:
//       S = Q K^T, dP = dO V^T, P, dS                       as phase 2 above (lane = key)
//       dV^T += dO^T P,  dK^T += Q^T dS                     as phase 2 above
//       dQ^T(partial over this key tile) = K^T dS^T         A = K^T via transpose reads (as phase 1), B = dS^T:
//           the dS tile is written 16-bit into 2 KiB of wave-private LDS as [key][query] rows (the same packed pairs
//           that feed the dK product) and read back with ds_read_b64_tr_b16 in the k order of the A chunk
// 20 MFMAs and 16 exp per pair, and the dQ contraction over ALL keys happens in one accumulator, so nothing is reduced across
// waves: the workgroup alternates between
//   main pass  (RQ query tiles): wave w computes the pairs (q tile, key tile w), accumulates dV^T / dK^T in registers and writes
//              each dS tile, 16-bit, as a [key][query] image of 2 KiB into shared LDS (the packed pairs that feed the dK product,
//              8-byte slots swizzled by (key >> 2) & 7: conflict-free for the ds_write_b64 rows and for the transpose reads);
//   dQ pass    wave j takes (query tile j >> 1, d half j & 1): dQ^T = sum over key tiles K^T dS^T with A = K^T via
//              ds_read_b64_tr_b16 (as phase 1 above) and B = dS^T read back from the images with ds_read_b64_tr_b16 in the k
//              order of the A chunk; two alternating accumulators, fixed order (deterministic, no atomics); rows leave as 8-byte
//              stores straight from the accumulator layout.
// Two workgroup barriers per round (RQ = 4 query tiles with <= 7 key tiles, 3 with 8).  V is never staged (only a register
// operand); K, Q, dO tiles + the dS images take 143..147 KiB: one 8-wave workgroup per CU.  Dropout is a template parameter here
// (and in the two-phase kernel): a runtime test per score splits the softmax into 16 basic blocks per pair and serialises the
// v_exp_f32 latencies.
template <typename T, int NKT, bool DROP>
__global__ __launch_bounds__(512) void attn_bwd16k_kernel(const T* __restrict__ qkv, const T* __restrict__ out,
                                                                        const T* __restrict__ dout, const float* __restrict__ lse,
                                                                        T* __restrict__ dqkv, int L, int H, float scale,
                                                                        const float* __restrict__ key_bias, float drop_p, uint32_t drop_seed, int order) {
  static_assert(sizeof(T) == 2 && NKT >= 5 && NKT <= 8, "16-bit storage, 5..8 key tiles");
  constexpr int LP = NKT * 32, RB = 128;
  constexpr int RQ = NKT <= 7 ? 4 : 3;   // query tiles per round
  constexpr int IMG = 2048;               // one dS tile: 32 key rows x 32 queries x 2 bytes
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* tK = smem;
  char* tQ = smem + LP * RB;
  char* tD = smem + 2 * LP * RB;       // dO
  char* DSb = smem + 3 * LP * RB;      // dS images [query tile of the round][key tile]; at the end the row staging of dK / dV
  float* Bs = (float*)(DSb + RQ * NKT * IMG);  // key bias * log2(e); -inf on padded keys
  float* Ls = Bs + LP;                 // -lse * log2(e); -inf on padded queries
  float* Ds = Ls + LP;                 // -delta * scale
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int b, h;
  attn_unit(blockIdx.x, gridDim.x, H, order, b, h);
  const int64_t row0 = (int64_t)b * L;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const T* qb = qkv + row0 * ldq + h * HD;
  const T* ob = out + row0 * ldo + h * HD;
  const T* dob = dout + row0 * ldo + h * HD;
  T* db = dqkv + row0 * ldq + h * HD;
  const float* lse_b = lse + ((int64_t)b * H + h) * L;
  const uint32_t dth = drop_thresh24(drop_p);
  const float dks = drop_seed ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t dbase = ((uint64_t)b * H + h) * (uint64_t)L;  // + q, then * L + key
  const float sl = scale * LOG2E;
  const int g = lane >> 5, ql = lane & 31;
  const int ntile = (L + 31) >> 5;           // >= 5 (dispatch)
  const bool active = wave < ntile;          // wave-uniform: this wave owns key tile `wave`
  for (int c = tid; c < LP; c += 512) {
    Bs[c] = c < L ? (key_bias ? key_bias[(int64_t)b * L + c] * LOG2E : 0.f) : -INFINITY;
    Ls[c] = c < L ? -lse_b[c] * LOG2E : -INFINITY;
  }
  {  // K, Q, dO rows -> LDS images (chunk ^ (bit1(row) << 2 | (row >> 2) & 3)), 1 KiB DMA pieces
    const uint32_t k_lds = lds_addr_of(tK), q_lds = lds_addr_of(tQ), d_lds = lds_addr_of(tD);
    const char* zero = (const char*)g_bwd_zero;
#pragma unroll
    for (int i = 0; i < (NKT * 4 + 7) / 8; ++i) {
      const int piece = wave + 8 * i;
      if (piece < ntile * 4) {
        const int row = piece * 8 + (lane >> 3), slot = lane & 7;
        const int ch = slot ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
        const char* pk = row < L ? (const char*)(qb + (int64_t)row * ldq + H * HD + ch * 8) : zero;
        const char* pq = row < L ? (const char*)(qb + (int64_t)row * ldq + ch * 8) : zero;
        const char* pd = row < L ? (const char*)(dob + (int64_t)row * ldo + ch * 8) : zero;
        dma16(pk, __builtin_amdgcn_readfirstlane(k_lds + piece * 1024));
        dma16(pq, __builtin_amdgcn_readfirstlane(q_lds + piece * 1024));
        dma16(pd, __builtin_amdgcn_readfirstlane(d_lds + piece * 1024));
      }
    }
  }
  // K / V fragments of key tile `wave` (B operands, lane = key) and delta of QUERY tile `wave`
  u32x4 kf[4], vf[4];
  {
    const int rc = min(min(wave, ntile - 1) * 32 + ql, L - 1);
    u32x4 dof[4], of[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int off = (2 * ks + g) * 8;
      dof[ks] = *(const u32x4*)(dob + (int64_t)rc * ldo + off);
      of[ks] = *(const u32x4*)(ob + (int64_t)rc * ldo + off);
      kf[ks] = *(const u32x4*)(qb + (int64_t)rc * ldq + H * HD + off);
      vf[ks] = *(const u32x4*)(qb + (int64_t)rc * ldq + 2 * H * HD + off);
    }
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      float a[8], c2[8];
      unpack_chunk<T>(dof[ks], a);
      unpack_chunk<T>(of[ks], c2);
#pragma unroll
      for (int e = 0; e < 8; ++e) delta += a[e] * c2[e];
    }
    delta += __shfl_xor(delta, 32, 64);
    if (active && g == 0) Ds[wave * 32 + ql] = -delta * scale;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int key = wave * 32 + ql;
  const bool need_kb = key_bias != nullptr || (wave + 1) * 32 > L;   // padded keys of the last tile: P = exp2(-inf) = 0, so they add nothing to dQ
  const float kb = (active && need_kb) ? Bs[key] : 0.f;
  const int swk = (ql >> 2) & 7;                           // 8-byte slot swizzle of the dS image (row = key)
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;
  // dS[query ql of the tile][keys k0 .. k0+3] from a [key][query] image (k0 multiple of 4)
  auto ds_quad = [&](const char* img, int k0) -> u32x2 {
    const int p = lane & 15, cb = (lane >> 4) & 1;
    const int row = k0 + (p >> 2);
    const char* a = img + row * 64 + ((((cb << 2) | (p & 3)) ^ ((row >> 2) & 7)) << 3);
    return ds_read_tr16(a);
  };
#pragma unroll 1
  for (int q0 = 0; q0 < ntile; q0 += RQ) {
    const int nq = min(RQ, ntile - q0);
    // ---------------------------------------------------------------- main pass: pairs (q0 + tl, key tile `wave`)
    if (active) {
#pragma unroll 1
      for (int tl = 0; tl < nq; ++tl) {
        const int qt = q0 + tl;
        char* img = DSb + (tl * NKT + wave) * IMG;
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
        const int qrow = qt * 32 + ql;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const u32x4 qa = *(const u32x4*)(tQ + tile_off<T>(qrow, 2 * ks + g));
          const u32x4 da = *(const u32x4*)(tD + tile_off<T>(qrow, 2 * ks + g));
          mma_chunk<T>(s, qa, kf[ks]);
          mma_chunk<T>(dp, da, vf[ks]);
        }
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float4 lq = *(const float4*)(Ls + qt * 32 + 8 * rq + 4 * g);
          const float4 dq4 = *(const float4*)(Ds + qt * 32 + 8 * rq + 4 * g);
          float ll[4] = {lq.x, lq.y, lq.z, lq.w};
          const float dd[4] = {dq4.x, dq4.y, dq4.z, dq4.w};
          if (need_kb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ll[e] += kb;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rq + e;
            const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sl, ll[e]));
            float gd = dp[r], pm = p;
            if constexpr (DROP) {
              const int qq = qt * 32 + 8 * rq + 4 * g + e;
              const bool keep = drop_keep(drop_seed, (dbase + (qq < L ? qq : L - 1)) * L + (key < L ? key : L - 1), dth);
              pm = keep ? p * dks : 0.f;
              gd = keep ? gd * dks : 0.f;
            }
            s[r] = pm;                           // dropped P (feeds dV)
            dp[r] = p * fmaf(gd, scale, dd[e]);  // dS
          }
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          float pv[8], sv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            pv[e] = s[cc * 8 + e];
            sv[e] = dp[cc * 8 + e];
          }
          const u32x4 pb = pack_chunk<T>(pv), sb = pack_chunk<T>(sv);
          // dS image: row = key (64 bytes = 32 queries), registers 4rq .. 4rq+3 are queries 8rq + 4g .. +3 -> 8-byte slot 2rq + g
          *(u32x2*)(img + ql * 64 + (((4 * cc + g) ^ swk) << 3)) = mk2(sb.x, sb.y);
          *(u32x2*)(img + ql * 64 + (((4 * cc + 2 + g) ^ swk) << 3)) = mk2(sb.z, sb.w);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            mma_chunk<T>(dv[dt], load_t_chunk<T>(tD, qt * 32, cc, lane, dt), pb);
            mma_chunk<T>(dk[dt], load_t_chunk<T>(tQ, qt * 32, cc, lane, dt), sb);
          }
        }
      }
    }
    __syncthreads();
    // ---------------------------------------------------------------- dQ pass: wave j = (query tile j >> 1, d half j & 1)
    if (wave < 2 * nq) {
      const int tl = wave >> 1, dt = wave & 1;
      f32x16 acc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
        if (kt < ntile) {
          const char* img = DSb + (tl * NKT + kt) * IMG;
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            const u32x2 lo = ds_quad(img, 16 * cc + 4 * g), hi = ds_quad(img, 16 * cc + 8 + 4 * g);
            const uint32_t lx = lo.x, ly = lo.y, hx = hi.x, hy = hi.y;
            mma_chunk<T>(acc[kt & 1], load_t_chunk<T>(tK, kt * 32, cc, lane, dt), mk4(lx, ly, hx, hy));
          }
        }
      const int q = (q0 + tl) * 32 + ql;
      if (q < L) {
        T* dst = db + (int64_t)q * ldq + dt * 32 + 4 * g;
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const uint32_t lo = pack2(acc[0][4 * rq] + acc[1][4 * rq], acc[0][4 * rq + 1] + acc[1][4 * rq + 1], (T*)0);
          const uint32_t hi = pack2(acc[0][4 * rq + 2] + acc[1][4 * rq + 2], acc[0][4 * rq + 3] + acc[1][4 * rq + 3], (T*)0);
          __builtin_nontemporal_store(mk2(lo, hi), (u32x2*)(dst + 8 * rq));
        }
      }
    }
    __syncthreads();   // the images are rewritten by the next round / become the row staging below
  }
  if (active) {
    store_rows_via_lds<T, false>(DSb + wave * 4096, dk, db + H * HD, ldq, wave * 32, L, lane);
    store_rows_via_lds<T, false>(DSb + wave * 4096, dv, db + 2 * H * HD, ldq, wave * 32, L, lane);
  }
}

#define ALPRO_TDROP 0
#define ALPRO_TKERNEL(name) name##_kernel
#define ALPRO_TDROP_PARAMS
#include "attention_bwd_temporal_kernels.hpp"
#undef ALPRO_TDROP
#undef ALPRO_TKERNEL
#undef ALPRO_TDROP_PARAMS
#define ALPRO_TDROP 1
#define ALPRO_TKERNEL(name) name##_drop_kernel
#define ALPRO_TDROP_PARAMS , float drop_p, uint32_t drop_seed
#include "attention_bwd_temporal_kernels.hpp"
#undef ALPRO_TDROP
#undef ALPRO_TKERNEL
#undef ALPRO_TDROP_PARAMS

template <typename T, int NKT, bool HAS_BIAS, bool DROP>
int launch_bwd16(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int batch, int L, int H, float scale,
                 const float* key_bias, float dp, uint32_t ds, hipStream_t st) {
  const size_t lds = 2 * (size_t)NKT * 32 * 128 + 4 * (NKT == 8 ? 2048 : 4096) + 3 * (size_t)NKT * 32 * sizeof(float);
  static DeviceOnce once;
  set_lds_once(once, attn_bwd16_kernel<T, NKT, HAS_BIAS, DROP>, lds);
  hipLaunchKernelGGL((attn_bwd16_kernel<T, NKT, HAS_BIAS, DROP>), dim3((unsigned)(batch * H)), dim3(256), lds, st, (const T*)qkv, (const T*)out, (const T*)dout,
                     lse, (T*)dqkv, L, H, scale, key_bias, dp, ds, get_option(OPT_ATTN_ORDER));
  return check_launch("alpro_attn_bwd");
}

template <typename T, int NKT, bool DROP>
int launch_bwd16k(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int batch, int L, int H, float scale,
                  const float* key_bias, float dp, uint32_t ds, hipStream_t st) {
  constexpr int LP = NKT * 32;
  const size_t lds = 3 * (size_t)LP * 128 + (size_t)(NKT <= 7 ? 4 : 3) * NKT * 2048 + 3 * (size_t)LP * sizeof(float);
  static DeviceOnce once;
  set_lds_once(once, attn_bwd16k_kernel<T, NKT, DROP>, lds);
  hipLaunchKernelGGL((attn_bwd16k_kernel<T, NKT, DROP>), dim3((unsigned)(batch * H)), dim3(512), lds, st, (const T*)qkv, (const T*)out, (const T*)dout,
                     lse, (T*)dqkv, L, H, scale, key_bias, dp, ds, get_option(OPT_ATTN_ORDER));
  return check_launch("alpro_attn_bwd");
}


template <typename T, int NKT, int NW, bool GROUPED>
int launch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int64_t nblocks_b, int L, int H, float scale,
               const float* key_bias, int Tn, int64_t total_rows, float dp, uint32_t ds, hipStream_t st) {
  const size_t lds = 2 * (size_t)NKT * 32 * TileCfg<T>::RB + 3 * (size_t)NKT * 32 * sizeof(float);
  static DeviceOnce once;
  set_lds_once(once, attn_bwd_kernel<T, NKT, NW, GROUPED>, lds);
  hipLaunchKernelGGL((attn_bwd_kernel<T, NKT, NW, GROUPED>), dim3((unsigned)(nblocks_b * H)), dim3(NW * 64), lds, st, (const T*)qkv, (const T*)out,
                     (const T*)dout, lse, (T*)dqkv, L, H, scale, key_bias, Tn, total_rows, dp, ds);
  return check_launch("alpro_attn_bwd");
}

template <typename T>
int dispatch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int batch, int L, int H, float scale,
                 const float* key_bias, float dp, uint32_t ds, hipStream_t st) {
  const int nkt = (L + 31) / 32;
  const int64_t rows = (int64_t)batch * L;
  if constexpr (sizeof(T) == 2) {
#define ALPRO_BWD16(N)                                                                                                          \
  do {                                                                                                                          \
    if (ds)                                                                                                                     \
      return key_bias ? launch_bwd16<T, N, true, true>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, dp, ds, st)     \
                      : launch_bwd16<T, N, false, true>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, dp, ds, st);   \
    return key_bias ? launch_bwd16<T, N, true, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, dp, ds, st)      \
                    : launch_bwd16<T, N, false, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, dp, ds, st);    \
  } while (0)
    if (nkt <= 2) ALPRO_BWD16(2);
    if (nkt <= 4) ALPRO_BWD16(4);
    // attn_bwd option: 0 two-phase everywhere; 1 (default) the measured best per shape: key-owned with 8 key tiles (fusion encoder,
    // L = 237: 0.48 vs 0.54 ms at 256 sequences), two-phase below (ViT spatial L = 197: 0.55 vs 0.63 ms at 512 sequences -- one 8-wave
    // workgroup per CU leaves its input latency uncovered); 2 key-owned wherever it applies (>= 5 key tiles).
    const int kind = get_option(OPT_ATTN_BWD);
    if ((nkt >= 5 && kind >= 2) || (nkt == 8 && kind == 1)) {   // every (query tile, key tile) pair once, one 8-wave workgroup per CU
#define ALPRO_BWD16K(N)                                                                                        \
  return ds ? launch_bwd16k<T, N, true>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, dp, ds, st)   \
            : launch_bwd16k<T, N, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, dp, ds, st)
      if (nkt <= 7) ALPRO_BWD16K(7);
      ALPRO_BWD16K(8);
#undef ALPRO_BWD16K
    }
    if (nkt <= 7) ALPRO_BWD16(7);
    ALPRO_BWD16(8);
#undef ALPRO_BWD16
  }
  if (nkt <= 2) return launch_bwd<T, 2, 4, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, 0, rows, dp, ds, st);
  if (nkt <= 4) return launch_bwd<T, 4, 4, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, 0, rows, dp, ds, st);
  if (nkt <= 7) return launch_bwd<T, 7, 4, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, 0, rows, dp, ds, st);
  return launch_bwd<T, 8, 4, false>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, 0, rows, dp, ds, st);
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int batch, int L,
                              int H, float scale, const float* key_bias, float drop_p, uint32_t drop_seed, void* stream) {
  ALPRO_CHECK(qkv && out && dout && lse && dqkv && batch > 0 && H > 0, "alpro_attn_bwd: bad args");
  ALPRO_CHECK(L > 0 && L <= ALPRO_ATTN_MAX_L, "alpro_attn_bwd: L=%d unsupported (1..%d = ALPRO_ATTN_MAX_L)", L, ALPRO_ATTN_MAX_L);
  if (L > 256) return attn_long_bwd(qkv, out, dout, lse, dqkv, dtype, batch, L, H, scale, key_bias, drop_p, drop_seed, (hipStream_t)stream);
  ALPRO_DISPATCH_DTYPE(dtype, T, return dispatch_bwd<T>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, drop_p, drop_seed, (hipStream_t)stream));
  return ALPRO_OK;
}

extern "C" int alpro_attn_temporal_bwd_drop(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype,
                                            int64_t rows, int T, int H, float scale, float drop_p, uint32_t drop_seed, void* stream) {
  ALPRO_CHECK(qkv && out && dout && lse && dqkv && rows > 0 && H > 0, "alpro_attn_temporal_bwd: bad args");
  ALPRO_CHECK(T > 0 && T <= ALPRO_ATTN_MAX_T, "alpro_attn_temporal_bwd: num_frm=%d unsupported (1..%d = ALPRO_ATTN_MAX_T)", T, ALPRO_ATTN_MAX_T);
  ALPRO_CHECK(rows % T == 0, "alpro_attn_temporal_bwd: rows=%lld not a multiple of T=%d", (long long)rows, T);
  ALPRO_CHECK(drop_p >= 0.f && drop_p < 1.f, "alpro_attn_temporal_bwd: drop_p=%g out of range (dropout needs 0 <= p < 1)", (double)drop_p);
  if (drop_p == 0.f) drop_seed = 0;   // either one 0: dropout off, the kernels of alpro_attn_temporal_bwd
  hipStream_t st = (hipStream_t)stream;
  if (32 % T != 0) return attn_temporal_any_bwd(qkv, out, dout, lse, dqkv, dtype, rows, T, H, scale, drop_p, drop_seed, st);
  const int64_t chunks = (rows + 31) / 32;
  if (dtype != ALPRO_F32) {
    const int64_t units = chunks * H;
    int64_t grid = (units + 3) / 4;
    if (grid > 512) grid = 512;
    const size_t lds = 4 * (4 * 4096 + 256);
    static DeviceOnce once_bf16, once_f16, once_bf16_drop, once_f16_drop;
    set_lds_once(once_bf16, attn_temporal_bwd16_kernel<bf16_t>, lds);
    set_lds_once(once_f16, attn_temporal_bwd16_kernel<f16_t>, lds);
    set_lds_once(once_bf16_drop, attn_temporal_bwd16_drop_kernel<bf16_t>, lds);
    set_lds_once(once_f16_drop, attn_temporal_bwd16_drop_kernel<f16_t>, lds);
    if (drop_seed) {
      if (dtype == ALPRO_BF16)
        hipLaunchKernelGGL(attn_temporal_bwd16_drop_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), lds, st, (const bf16_t*)qkv, (const bf16_t*)dout, lse, (bf16_t*)dqkv,
                           rows, T, H, scale, units, drop_p, drop_seed);
      else
        hipLaunchKernelGGL(attn_temporal_bwd16_drop_kernel<f16_t>, dim3((unsigned)grid), dim3(256), lds, st, (const f16_t*)qkv, (const f16_t*)dout, lse, (f16_t*)dqkv,
                           rows, T, H, scale, units, drop_p, drop_seed);
    } else if (dtype == ALPRO_BF16) {
      hipLaunchKernelGGL(attn_temporal_bwd16_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), lds, st, (const bf16_t*)qkv, (const bf16_t*)dout, lse,
                         (bf16_t*)dqkv, rows, T, H, scale, units);
    } else {
      hipLaunchKernelGGL(attn_temporal_bwd16_kernel<f16_t>, dim3((unsigned)grid), dim3(256), lds, st, (const f16_t*)qkv, (const f16_t*)dout, lse,
                         (f16_t*)dqkv, rows, T, H, scale, units);
    }
    return check_launch("alpro_attn_temporal_bwd");
  }
  if (drop_seed) {   // fp32 is the one dtype that gets here
    const size_t lds = 2 * 32 * (size_t)TileCfg<float>::RB + 3 * 32 * sizeof(float);
    hipLaunchKernelGGL((attn_bwd_drop_kernel<float, 1, 1, true>), dim3((unsigned)(chunks * H)), dim3(64), lds, st, (const float*)qkv, (const float*)out, (const float*)dout, lse,
                       (float*)dqkv, 32, H, scale, (const float*)nullptr, T, rows, drop_p, drop_seed);
    return check_launch("alpro_attn_temporal_bwd");
  }
  ALPRO_DISPATCH_DTYPE(dtype, T_, return (launch_bwd<T_, 1, 1, true>(qkv, out, dout, lse, dqkv, chunks, 32, H, scale, nullptr, T, rows, 0.f, 0u, st)));
  return ALPRO_OK;
}

extern "C" int alpro_attn_temporal_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype,
                                       int64_t rows, int T, int H, float scale, void* stream) {
  return alpro_attn_temporal_bwd_drop(qkv, out, dout, lse, dqkv, dtype, rows, T, H, scale, 0.f, 0u, stream);
}
