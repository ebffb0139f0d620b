// Epilogue pieces of the NT GEMM kernels: LDS swizzle, row maps, the wave-private staging hand-offs and the 16-row epilogues (fp32-staged and
// 16-bit identity-map forms) that gemm_nt_kernel, gemm_nt256p_kernel and the staged paths of gemm_nt256q_kernel share.
#pragma once
#include "gemm_pipe.hpp"
namespace alpro {
namespace {
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }

struct RowDst {
  int64_t out, res;
  bool side;
};
template <int mode>
__device__ __forceinline__ RowDst map_row(int p0, int p1, int m) {
  RowDst d;
  d.side = false;
  if (mode == ALPRO_MAP_IDENTITY) {
    d.out = d.res = m;
  } else if (mode == ALPRO_MAP_SKIP_CLS) {
    d.out = d.res = (int64_t)m + m / p0 + 1;
  } else if (mode == ALPRO_MAP_FRAME_TOKENS) {
    const int T = p0, N = p1;
    const int bt = m / (N + 1), j = m - bt * (N + 1);
    const int b = bt / T, t = bt - b * T;
    if (j == 0) {
      d.side = true;
      d.out = bt;
      d.res = -1;
    } else {
      d.out = d.res = (int64_t)b * (1 + N * T) + 1 + (int64_t)(j - 1) * T + t;
    }
  } else {  // PATCH_EMBED
    const int T = p0, N = p1;
    const int bt = m / N, n = m - bt * N;
    const int b = bt / T, t = bt - b * T;
    d.out = (int64_t)b * (1 + N * T) + 1 + (int64_t)n * T + t;
    d.res = (int64_t)n * T + t;
  }
  return d;
}

template <typename T>
__device__ __forceinline__ void store_c(void* C, int c_dtype, int64_t idx, float v) {
  if (c_dtype == ALPRO_F32) ((float*)C)[idx] = v;
  else ((T*)C)[idx] = from_f32<T>(v);
}

// Wave-private LDS hand-off: DS operations of one wave execute in issue order, so a ds_read after a ds_write of the
// same wave needs no hardware wait -- only the compiler must not reorder them.
// (named apart from attention_temporal_any.hip's wave_lds_sync(), which waits WITHOUT the wave barrier)
__device__ __forceinline__ void wave_lds_handoff() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The same hand-off without the wait: pins the COMPILER's issue order only (no instruction).  The compiler reasons per lane -- when it can
// prove that a lane's own staging writes and its own reads never overlap, it may move the read above a write that ANOTHER lane's read depends
// on.  Round 4 hit exactly that: the fp32-output epilogue of the 8-phase kernel read its first staged row before the last ds_write2 of the
// fragment row had been issued (256 stale elements per tile, tests/test_hip_ops.py::test_gemm_8phase_kernel[f32res]); the other staging
// epilogues had been in source order by luck.  Every stage write block is now bracketed by this.
__device__ __forceinline__ void wave_lds_order() { asm volatile("" ::: "memory"); }

template <typename T, int ACT> __device__ __forceinline__ float apply_act(float x) {
  if (ACT == ALPRO_ACT_GELU) return gelu_fast<T>(x);   // (GELU_SAVE_GRAD computes gelu together with gelu' before this point)
  if (ACT == ALPRO_ACT_RELU) return x < 0.f ? 0.f : x;   // NaN passes, as torch.relu and alpro_gemm_rows_f32 (fmaxf turned it into 0)
  return x;
}

// Output / residual accesses are non-temporal: they are streamed once (150-600 MB per launch against 32 MB of L2), and
// keeping them out of the L2 allocation path is worth 7-8 % on the bf16-output GEMMs (round-2 measurement).
// Epilogue of 16 staged rows x 64 columns of one wave: lane l handles columns 4*(l&15)..+3 of rows p*4 + (l>>4),
// p = 0..3, so every global access is a 16-byte (fp32) / 8-byte (16-bit) piece of a 256-/128-byte row segment.
// FAST (wave-uniform): the whole 16x64 block is in range and every stride is vector-aligned -> no per-element
// predication at all (the predicated variant is ~4x the instructions and was costing ~11 us per 256x256 tile).
template <typename T, int ACT, int MAP, bool FAST, int PASSES = 4>
__device__ __forceinline__ void epi_rows16(const alpro_gemm_desc_t& g, const float* stage, int m_base, int n_base, int lane, const float (&bias)[4],
                                           const float4* pre_res = nullptr) {
  const int c4 = (lane & 15) * 4;
  const int n = n_base + c4;
  float4 rr[PASSES];
  int64_t orow[PASSES];
  bool live[PASSES], side[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int m = m_base + p * 4 + (lane >> 4);
    live[p] = FAST || (m < g.M && n < g.N);
    const RowDst d = map_row<MAP>(g.map_p0, g.map_p1, live[p] ? m : 0);
    orow[p] = d.out;
    side[p] = d.side;
    rr[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pre_res) {
      rr[p] = pre_res[p];  // already in flight / landed: issued two chunks ago by the caller
    } else if (g.residual && live[p] && !d.side) {
      const float* rp = g.residual + d.res * g.ldr + n;
      if (FAST) {
        const f32x4 t = __builtin_nontemporal_load((const f32x4*)rp);  // streamed once
        rr[p] = make_float4(t.x, t.y, t.z, t.w);
      }
      else {
        rr[p].x = rp[0];
        if (n + 1 < g.N) rr[p].y = rp[1];
        if (n + 2 < g.N) rr[p].z = rp[2];
        if (n + 3 < g.N) rr[p].w = rp[3];
      }
    }
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int row = p * 4 + (lane >> 4);
    if (!live[p]) continue;
    const float4 a = *(const float4*)(stage + row * 64 + c4);
    float v[4] = {a.x, a.y, a.z, a.w};
    const float res[4] = {rr[p].x, rr[p].y, rr[p].z, rr[p].w};
    const float rs = g.row_scale ? g.row_scale[(g.m_off + m_base + row) / g.row_scale_group] : 1.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = g.alpha * v[e] + bias[e];
    if ((ACT == ALPRO_ACT_GELU || ACT == ALPRO_ACT_RELU) && g.C2) {  // pre-activation copy (host guarantees vector alignment for C2)
      if constexpr (sizeof(T) == 2) {
        __builtin_nontemporal_store(mk2(pack2(v[0], v[1], (T*)0), pack2(v[2], v[3], (T*)0)), (u32x2*)((T*)g.C2 + orow[p] * g.ldc2 + n));
      } else {
        *(float4*)((float*)g.C2 + orow[p] * g.ldc2 + n) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    if (ACT == ALPRO_ACT_GELU_SAVE_GRAD) {  // v = gelu(v), C2 = gelu'(v)
      float dv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) gelu_and_grad<T>(v[e], v[e], dv[e]);
      if (FAST) {
        if constexpr (sizeof(T) == 2) {
          __builtin_nontemporal_store(mk2(pack2(dv[0], dv[1], (T*)0), pack2(dv[2], dv[3], (T*)0)), (u32x2*)((T*)g.C2 + orow[p] * g.ldc2 + n));
        } else {
          *(float4*)((float*)g.C2 + orow[p] * g.ldc2 + n) = make_float4(dv[0], dv[1], dv[2], dv[3]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < g.N) ((T*)g.C2)[orow[p] * g.ldc2 + n + e] = from_f32<T>(dv[e]);
      }
    }
    if (ACT == ALPRO_ACT_GELU_BWD || ACT == ALPRO_ACT_MUL_SAVED) {  // v *= gelu'(saved pre-activation) / v *= saved factor
      const T* pp = (const T*)g.C2 + orow[p] * g.ldc2 + n;
      float pre[4];
      if (FAST) {
        if constexpr (sizeof(T) == 2) {
          const u32x2 u = *(const u32x2*)pp;
          const uint32_t ux = u.x, uy = u.y;
          pre[0] = to_f32(T{(uint16_t)(ux & 0xFFFFu)});
          pre[1] = to_f32(T{(uint16_t)(ux >> 16)});
          pre[2] = to_f32(T{(uint16_t)(uy & 0xFFFFu)});
          pre[3] = to_f32(T{(uint16_t)(uy >> 16)});
        } else {
          const float4 f = *(const float4*)pp;
          pre[0] = f.x; pre[1] = f.y; pre[2] = f.z; pre[3] = f.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pre[e] = (n + e < g.N) ? to_f32(pp[e]) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= (ACT == ALPRO_ACT_MUL_SAVED) ? pre[e] : gelu_grad<T>(pre[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = apply_act<T, ACT>(v[e]) * rs;
    if (MAP == ALPRO_MAP_IDENTITY && g.drop_seed) {
      const uint32_t th = drop_thresh24(g.drop_p);
      const float ks = 1.0f / (1.0f - g.drop_p);
      const uint64_t i0 = (uint64_t)(g.m_off + m_base + row) * (uint64_t)g.N + (uint64_t)n;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = drop_keep(g.drop_seed, i0 + e, th) ? v[e] * ks : 0.f;
    }
    if constexpr (MAP == ALPRO_MAP_SKIP_CLS) {
      if (g.bias2) {  // unscaled second bias (merged temporal projection)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (FAST || n + e < g.N) ? g.bias2[n + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += res[e];
    if (MAP == ALPRO_MAP_FRAME_TOKENS && side[p]) {
      float* dst = g.side + orow[p] * g.ld_side + n;
      if (FAST) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < g.N) dst[e] = v[e];
      }
    } else if (FAST) {
      if (g.c_dtype == ALPRO_F32) {
        __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, (f32x4*)((float*)g.C + orow[p] * g.ldc + n));
      } else if constexpr (sizeof(T) == 2) {
        __builtin_nontemporal_store(mk2(pack2(v[0], v[1], (T*)0), pack2(v[2], v[3], (T*)0)), (u32x2*)((T*)g.C + orow[p] * g.ldc + n));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < g.N) store_c<T>(g.C, g.c_dtype, orow[p] * g.ldc + n + e, v[e]);
    }
  }
}

// Residual rows of one 8-row chunk (the two passes of epi_rows16<.., PASSES = 2>) for a FAST tile.  The persistent kernel
// issues these one chunk ahead of their use (two would spill): loaded at the point of use, every chunk exposed a full HBM round trip
// (16 chunks x ~1.5 us = the whole 25 us epilogue of the N=768 fp32-residual GEMMs; 16 KiB in flight per CU = ~11 B/clk).
template <int MAP>
__device__ __forceinline__ void epi_prefetch_res(const alpro_gemm_desc_t& g, int m_base, int n_base, int lane, float4 (&rr)[2]) {
  const int n = n_base + (lane & 15) * 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const RowDst d = map_row<MAP>(g.map_p0, g.map_p1, m_base + p * 4 + (lane >> 4));
    rr[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!d.side) {
      const f32x4 t = __builtin_nontemporal_load((const f32x4*)(g.residual + d.res * g.ldr + n));
      rr[p] = make_float4(t.x, t.y, t.z, t.w);
    }
  }
}

// 16-bit outputs under the identity map (qkv / proj / fc1 / every dgrad): 8 columns per lane -> one 16-byte store per
// lane, 8 rows per wave instruction.  The store path is ISSUE-bound per CU (~one wave-store per ~100 cycles measured),
// so halving the number of store instructions halves the epilogue tail.  Whole block in range (FAST) only.
// Round 5: no vector-memory load sits behind a run-time test inside a pass.  Rounds 3-4 tested g.row_scale / g.residual per pass; the row scale was
// a conditional per-lane load, and the join behind a conditional load is closed with s_waitcnt vmcnt(0): every one of a tile's 16 passes
// waited for the previous pass's output store to be acknowledged -- and, in the MUL_SAVED form, for the saved-factor rows fetched AHEAD, which
// defeated the run-ahead.  Now (i) the fp32 residual is a template parameter (RES: the caller tests the pointer once per tile), and (ii) the
// row scale of a pass comes from SCALAR loads: a pass covers 8 consecutive rows, which lie in at most two groups when row_scale_group >= 8
// (launcher: drop-path scales per 8-frame token group, per 197-token frame, per clip) -- one wave-uniform division, two s_load_dword, a
// compare per lane.  The plain GEMMs (qkv, fc1, dgrads) have no load at all in their passes: the stores stream.
template <typename T, int ACT, int PASSES = 2, bool RES = true>
__device__ __forceinline__ void epi_rows16_c16(const alpro_gemm_desc_t& g, const float* stage, int m_base, int n_base, int lane, const float (&bias)[8],
                                               const u32x4* pre_c2 = nullptr) {
  const int c8 = (lane & 7) * 8;
  const int n = n_base + c8;
  float rsv[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) rsv[p] = 1.0f;
  if (g.row_scale) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const uint32_t m0 = (uint32_t)g.m_off + (uint32_t)__builtin_amdgcn_readfirstlane(m_base) + p * 8;   // first row of the pass (wave-uniform; rows < 2^31)
      const uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(m0 / (uint32_t)g.row_scale_group));
      const uint32_t edge = (gi + 1) * (uint32_t)g.row_scale_group;
      const float lo = sload_f32(g.row_scale, gi), hi = sload_f32(g.row_scale, edge < (uint32_t)g.m_off + (uint32_t)g.M ? gi + 1 : gi);
      rsv[p] = (m0 + (uint32_t)(lane >> 3)) >= edge ? hi : lo;
    }
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int row = p * 8 + (lane >> 3);
    const int64_t m = m_base + row;
    const float4 a0 = *(const float4*)(stage + row * 64 + c8), a1 = *(const float4*)(stage + row * 64 + c8 + 4);
    float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float rs = rsv[p];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = g.alpha * v[e] + bias[e];
    if ((ACT == ALPRO_ACT_GELU || ACT == ALPRO_ACT_RELU) && g.C2) __builtin_nontemporal_store(pack_chunk<T>(v), (u32x4*)((T*)g.C2 + m * g.ldc2 + n));
    if (ACT == ALPRO_ACT_GELU_SAVE_GRAD) {
      float dv[8];
      if constexpr (sizeof(T) == 2) {   // 16-bit storage: the one-exponential form on pairs (common.hpp gelu_and_grad2)
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          f32x2v yy, dd;
          gelu_and_grad2((f32x2v){v[e], v[e + 1]}, yy, dd);
          v[e] = yy.x; v[e + 1] = yy.y;
          dv[e] = dd.x; dv[e + 1] = dd.y;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) gelu_and_grad<T>(v[e], v[e], dv[e]);
      }
      __builtin_nontemporal_store(pack_chunk<T>(dv), (u32x4*)((T*)g.C2 + m * g.ldc2 + n));
    }
    if (ACT == ALPRO_ACT_GELU_BWD || ACT == ALPRO_ACT_MUL_SAVED) {
      float pre[8];
      unpack_chunk<T>(pre_c2 ? pre_c2[p] : *(const u32x4*)((const T*)g.C2 + m * g.ldc2 + n), pre);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= (ACT == ALPRO_ACT_MUL_SAVED) ? pre[e] : gelu_grad<T>(pre[e]);
    }
    if constexpr (ACT == ALPRO_ACT_GELU && sizeof(T) == 2) {   // the same arithmetic as gelu_fast, polynomial on pairs (v_pk_fma_f32)
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const f32x2v yy = gelu_fast2((f32x2v){v[e], v[e + 1]});
        v[e] = yy.x * rs;
        v[e + 1] = yy.y * rs;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = apply_act<T, ACT>(v[e]) * rs;
    }
    if (g.drop_seed) {
      float dp = g.drop_p;
      asm volatile("" : "+s"(dp));   // keeps 1 / (1 - p) (and its packed-multiply splat) from being hoisted over the K loop as a kernel invariant, where it is spilled and reloaded per pass
      const uint32_t th = drop_thresh24(dp);
      const float ks = 1.0f / (1.0f - dp);
      const uint64_t i0 = (uint64_t)(g.m_off + m) * (uint64_t)g.N + (uint64_t)n;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = drop_keep(g.drop_seed, i0 + e, th) ? v[e] * ks : 0.f;
    }
    if constexpr (RES) {
      if (g.residual) {
        const f32x4 r0 = __builtin_nontemporal_load((const f32x4*)(g.residual + m * g.ldr + n)), r1 = __builtin_nontemporal_load((const f32x4*)(g.residual + m * g.ldr + n + 4));
        v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
      }
    }
    __builtin_nontemporal_store(pack_chunk<T>(v), (u32x4*)((T*)g.C + m * g.ldc + n));
  }
}

// wave-uniform test for the FAST epilogue of a (rows x 64) wave sub-tile
__device__ __forceinline__ bool epi_fast_ok(const alpro_gemm_desc_t& g, int m_base, int rows, int n_base) {
  return (m_base + rows <= g.M) && (n_base + 64 <= g.N) && ((g.ldc & 3) == 0) && (!g.residual || (g.ldr & 3) == 0) &&
         ((g.ld_side & 3) == 0);
}

__device__ __forceinline__ void load_bias4(const alpro_gemm_desc_t& g, int n, float (&bias)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) bias[e] = (g.bias && n + e < g.N) ? g.bias[n + e] : 0.f;
}
}  // namespace
}  // namespace alpro
