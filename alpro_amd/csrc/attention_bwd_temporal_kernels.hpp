// Included TWICE by attention_bwd.hip, inside its namespaces: ALPRO_TDROP 0 stamps out the kernels NAME_kernel as they have always been, ALPRO_TDROP 1
// the kernels NAME_drop_kernel with dropout on the attention probabilities.  The two are separate texts for the compiler, not one template with a
// flag behind a forwarding kernel: with the body in an inlined function template the p = 0 kernels came out as different machine code
// (other register counts), and they have to stay the code they are.  No include guard.
// GDROP: probability dropout of the GROUPED (temporal) form, compiled in (the un-grouped form tests drop_seed at run time, as before).
template <typename T, int NKT, int NW, bool GROUPED>
__global__ __launch_bounds__(NW * 64) void ALPRO_TKERNEL(attn_bwd)(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                           const float* __restrict__ lse, T* __restrict__ dqkv, int L, int H, float scale,
                                                           const float* __restrict__ key_bias, int Tn, int64_t total_rows, float drop_p,
                                                           uint32_t drop_seed) {
  constexpr bool GDROP = ALPRO_TDROP != 0;
  static_assert(!GDROP || (GROUPED && NKT == 1), "GDROP is the temporal form's dropout");
  typedef TileCfg<T> C;
  constexpr int LP = NKT * 32;
  constexpr int NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* tA = smem;                 // K, then Q
  char* tB = smem + LP * C::RB;    // V, then dO
  float* Bs = (float*)(smem + 2 * LP * C::RB);
  float* Ls = Bs + LP;
  float* Ds = Ls + LP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int64_t row0 = (int64_t)b * L;
  const int Le = GROUPED ? (int)((total_rows - row0) < 32 ? (total_rows - row0) : 32) : L;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const T* qb = qkv + row0 * ldq + h * HD;
  const T* ob = out + row0 * ldo + h * HD;
  const T* dob = dout + row0 * ldo + h * HD;
  T* db = dqkv + row0 * ldq + h * HD;
  const float* lse_b = lse + ((int64_t)b * H + h) * L;
  const uint32_t dth = drop_thresh24(drop_p);
  const float dks = drop_seed ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t dbase = ((uint64_t)b * H + h) * (uint64_t)L;  // + q, then * L + key
  for (int c = tid; c < LP; c += NT) {
    Bs[c] = c < Le ? ((!GROUPED && key_bias) ? key_bias[(int64_t)b * L + c] : 0.f) : -INFINITY;
    Ls[c] = c < Le ? lse_b[c] : INFINITY;
  }
  stage_tile<T>(tA, qb + H * HD, ldq, Le, LP, tid, NT);
  stage_tile<T>(tB, qb + 2 * H * HD, ldq, Le, LP, tid, NT);
  __syncthreads();

  const int g = lane >> 5, ql = lane & 31;
  const int ntile = (Le + 31) >> 5;
  // ---------------------------------------------------------------- phase 1: dQ (lane = query)
  for (int qt = wave; qt < ntile; qt += NW) {
    const int q = qt * 32 + ql;
    const int qc = q < Le ? q : Le - 1;
    u32x4 qf[C::KS], dof[C::KS];
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      const int off = (2 * ks + g) * C::CN;
      qf[ks] = *(const u32x4*)(qb + (int64_t)qc * ldq + off);
      dof[ks] = *(const u32x4*)(dob + (int64_t)qc * ldo + off);
      const u32x4 of = *(const u32x4*)(ob + (int64_t)qc * ldo + off);
      float a[C::CN], c2[C::CN];
      unpack_chunk<T>(dof[ks], a);
      unpack_chunk<T>(of, c2);
#pragma unroll
      for (int e = 0; e < C::CN; ++e) delta += a[e] * c2[e];
    }
    delta += __shfl_xor(delta, 32, 64);
    const float lse_q = Ls[q];
    if (g == 0) Ds[q] = delta;
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
        for (int ks = 0; ks < C::KS; ++ks) {
          const u32x4 ka = *(const u32x4*)(tA + tile_off<T>(krow, 2 * ks + g));
          const u32x4 va = *(const u32x4*)(tB + tile_off<T>(krow, 2 * ks + g));
          mma_chunk<T>(s, ka, qf[ks]);
          mma_chunk<T>(dp, va, dof[ks]);
        }
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float4 bq = *(const float4*)(Bs + kt * 32 + 8 * rq + 4 * g);
          const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rq + e;
            float p = expf(s[r] * scale + bb[e] - lse_q);
            if (GROUPED && ((8 * rq + 4 * g + e) / Tn != ql / Tn)) p = 0.f;
            float gd = dp[r];
            if (!GROUPED && drop_seed) gd = drop_keep(drop_seed, (dbase + qc) * L + kt * 32 + 8 * rq + 4 * g + e, dth) ? gd * dks : 0.f;
            if constexpr (GDROP) gd = drop_keep(drop_seed, temporal_drop_base(row0, ql, Tn, H, h) + (uint64_t)(8 * rq + 4 * g + e), dth) ? gd * dks : 0.f;
            s[r] = p * (gd - delta) * scale;  // dS^T
          }
        }
#pragma unroll
        for (int cc = 0; cc < C::CPT; ++cc) {
          float v[C::CN];
#pragma unroll
          for (int e = 0; e < C::CN; ++e) v[e] = s[cc * C::CN + e];
          const u32x4 bop = pack_chunk<T>(v);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(dq[dt], load_t_chunk<T>(tA, kt * 32, cc, lane, dt), bop);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (q < Le) store_row64<T>(db + (int64_t)q * ldq, dq, lane);
  }
  __syncthreads();
  // ---------------------------------------------------------------- phase 2: dK, dV (lane = key)
  stage_tile<T>(tA, qb, ldq, Le, LP, tid, NT);
  stage_tile<T>(tB, dob, ldo, Le, LP, tid, NT);
  __syncthreads();
  for (int kt = wave; kt < ntile; kt += NW) {
    const int key = kt * 32 + ql;
    const int kc = key < Le ? key : Le - 1;
    u32x4 kf[C::KS], vf[C::KS];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      const int off = (2 * ks + g) * C::CN;
      kf[ks] = *(const u32x4*)(qb + (int64_t)kc * ldq + H * HD + off);
      vf[ks] = *(const u32x4*)(qb + (int64_t)kc * ldq + 2 * H * HD + off);
    }
    const float kb = Bs[key];
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
      for (int ks = 0; ks < C::KS; ++ks) {
        const u32x4 qa = *(const u32x4*)(tA + tile_off<T>(qrow, 2 * ks + g));
        const u32x4 da = *(const u32x4*)(tB + tile_off<T>(qrow, 2 * ks + g));
        mma_chunk<T>(s, qa, kf[ks]);
        mma_chunk<T>(dp, da, vf[ks]);
      }
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const float4 lq = *(const float4*)(Ls + qt * 32 + 8 * rq + 4 * g);
        const float4 dq4 = *(const float4*)(Ds + qt * 32 + 8 * rq + 4 * g);
        const float ll[4] = {lq.x, lq.y, lq.z, lq.w}, dd[4] = {dq4.x, dq4.y, dq4.z, dq4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * rq + e;
          float p = expf(s[r] * scale + kb - ll[e]);
          if (GROUPED && ((8 * rq + 4 * g + e) / Tn != ql / Tn)) p = 0.f;
          float dm = 1.0f;
          if (!GROUPED && drop_seed) {
            const int qq = qt * 32 + 8 * rq + 4 * g + e;
            dm = drop_keep(drop_seed, (dbase + (qq < Le ? qq : Le - 1)) * L + key, dth) ? dks : 0.f;
          }
          if constexpr (GDROP) dm = drop_keep(drop_seed, temporal_drop_base_key(row0, ql, Tn, H, h) + (uint64_t)(8 * rq + 4 * g + e) * (uint64_t)Tn, dth) ? dks : 0.f;
          s[r] = p * dm;                                // dropped P (feeds dV)
          dp[r] = p * (dm * dp[r] - dd[e]) * scale;     // dS
        }
      }
#pragma unroll
      for (int cc = 0; cc < C::CPT; ++cc) {
        float pv[C::CN], sv[C::CN];
#pragma unroll
        for (int e = 0; e < C::CN; ++e) {
          pv[e] = s[cc * C::CN + e];
          sv[e] = dp[cc * C::CN + e];
        }
        const u32x4 pb = pack_chunk<T>(pv), sb = pack_chunk<T>(sv);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          mma_chunk<T>(dv[dt], load_t_chunk<T>(tB, qt * 32, cc, lane, dt), pb);
          mma_chunk<T>(dk[dt], load_t_chunk<T>(tA, qt * 32, cc, lane, dt), sb);
        }
      }
    }
    if (key < Le) {
      store_row64<T>(db + (int64_t)key * ldq + H * HD, dk, lane);
      store_row64<T>(db + (int64_t)key * ldq + 2 * H * HD, dv, lane);
    }
  }
}

// ================================================================================================
// 16-bit temporal-attention backward: one WAVE per (32 consecutive tokens, head) unit, everything wave-private.
// The four 4 KiB tiles K, V, Q, dO of the unit go global -> LDS by DMA (16 copies per unit, swizzled on the source side) and
// every operand is then read from LDS; delta = rowsum(P o dP) (== rowsum(dO o O) for the recomputed P), so the saved
// output is not read at all; dQ / dK / dV leave through the dead K / V tiles as 16-byte row stores.  No workgroup
// barrier anywhere: 4 independent waves per workgroup, 2 workgroups per CU, units handed out grid-stride.
// DROP: the mask is regenerated from the seed, dP = keep / (1 - p) * (dO V^T), and
// delta = rowsum(P o dP) with that dP (== rowsum(dO o O) for the dropped O).
template <typename T>
__global__ __launch_bounds__(256, 2) void ALPRO_TKERNEL(attn_temporal_bwd16)(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                                    const float* __restrict__ lse, T* __restrict__ dqkv, int64_t rows, int Tn,
                                                                    int H, float scale, int64_t units ALPRO_TDROP_PARAMS) {
  constexpr bool DROP = ALPRO_TDROP != 0;
#if !ALPRO_TDROP
  constexpr float drop_p = 0.f;
  constexpr uint32_t drop_seed = 0u;
#endif
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int WB = 4 * 4096 + 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* base = smem + wave * WB;
  char* tK = base;
  char* tV = base + 4096;
  char* tQ = base + 8192;
  char* tD = base + 12288;
  float* Ls = (float*)(base + 16384);  // -lse * log2(e); -inf on padded queries
  float* Ds = Ls + 32;                  // -delta * scale
  const uint32_t lds0 = lds_addr_of(base);
  const char* zero = (const char*)g_bwd_zero;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const int g = lane >> 5, ql = lane & 31;
  const float sl = scale * LOG2E;
  const int qgrp = ql / Tn;
  const uint32_t dth = drop_thresh24(drop_p);
  const float dks = DROP ? 1.0f / (1.0f - drop_p) : 1.0f;
  for (int64_t unit = (int64_t)blockIdx.x * 4 + wave; unit < units; unit += (int64_t)gridDim.x * 4) {
    const int64_t chunk = unit / H;
    const int h = (int)(unit - chunk * H);
    const int64_t r0 = chunk * 32;
    const int Le = (int)((rows - r0) < 32 ? (rows - r0) : 32);
    const T* qb = qkv + r0 * ldq + h * HD;
    const T* dob = dout + r0 * ldo + h * HD;
    T* db = dqkv + r0 * ldq + h * HD;
#pragma unroll
    for (int piece = 0; piece < 4; ++piece) {
      const int row = piece * 8 + (lane >> 3), slot = lane & 7;
      const int ch = slot ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
      const bool ok = row < Le;
      const T* src = qb + (int64_t)row * ldq + ch * 8;
      dma16(ok ? (const char*)(src + H * HD) : zero, __builtin_amdgcn_readfirstlane(lds0 + piece * 1024));
      dma16(ok ? (const char*)(src + 2 * H * HD) : zero, __builtin_amdgcn_readfirstlane(lds0 + 4096 + piece * 1024));
      dma16(ok ? (const char*)src : zero, __builtin_amdgcn_readfirstlane(lds0 + 8192 + piece * 1024));
      dma16(ok ? (const char*)(dob + (int64_t)row * ldo + ch * 8) : zero, __builtin_amdgcn_readfirstlane(lds0 + 12288 + piece * 1024));
    }
    if (lane < 32) Ls[lane] = lane < Le ? -lse[unit * 32 + lane] * LOG2E : -INFINITY;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ------------------------------------------------------------ phase 1: dQ (lane = query)
    u32x4 qf[4], dof[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = *(const u32x4*)(tQ + tile_off<T>(ql, 2 * ks + g));
      dof[ks] = *(const u32x4*)(tD + tile_off<T>(ql, 2 * ks + g));
    }
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      mma_chunk<T>(s, *(const u32x4*)(tK + tile_off<T>(ql, 2 * ks + g)), qf[ks]);
      mma_chunk<T>(dp, *(const u32x4*)(tV + tile_off<T>(ql, 2 * ks + g)), dof[ks]);
    }
    const float nlq = Ls[ql];
    float delta = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = (r & 3) + 8 * (r >> 2) + 4 * g;
      const float p = (key / Tn == qgrp) ? __builtin_amdgcn_exp2f(fmaf(s[r], sl, nlq)) : 0.f;
      s[r] = p;
      if constexpr (DROP) dp[r] = drop_keep(drop_seed, temporal_drop_base(r0, ql, Tn, H, h) + (uint64_t)key, dth) ? dp[r] * dks : 0.f;
      delta = fmaf(p, dp[r], delta);
    }
    delta += __shfl_xor(delta, 32, 64);
    const float nds = -delta * scale;
    if (g == 0) Ds[ql] = nds;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] *= fmaf(dp[r], scale, nds);  // dS^T
    f32x16 acc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = s[cc * 8 + e];
      const u32x4 bop = pack_chunk<T>(v);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(acc[dt], load_t_chunk<T>(tK, 0, cc, lane, dt), bop);
    }
    // K / V rows of this lane's key as phase-2 B operands, then the K tile is dead: dQ leaves through it
    u32x4 kf[4], vf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks] = *(const u32x4*)(tK + tile_off<T>(ql, 2 * ks + g));
      vf[ks] = *(const u32x4*)(tV + tile_off<T>(ql, 2 * ks + g));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    store_rows_via_lds<T>(tK, acc, db, ldq, 0, Le, lane);
    // ------------------------------------------------------------ phase 2: dK, dV (lane = key)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      mma_chunk<T>(s, *(const u32x4*)(tQ + tile_off<T>(ql, 2 * ks + g)), kf[ks]);
      mma_chunk<T>(dp, *(const u32x4*)(tD + tile_off<T>(ql, 2 * ks + g)), vf[ks]);
    }
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const float4 lq = *(const float4*)(Ls + 8 * rq + 4 * g);
      const float4 dq4 = *(const float4*)(Ds + 8 * rq + 4 * g);
      const float ll[4] = {lq.x, lq.y, lq.z, lq.w}, dd[4] = {dq4.x, dq4.y, dq4.z, dq4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * rq + e;
        const float p = ((8 * rq + 4 * g + e) / Tn == qgrp) ? __builtin_amdgcn_exp2f(fmaf(s[r], sl, ll[e])) : 0.f;
        if constexpr (DROP) {
          const float dm = drop_keep(drop_seed, temporal_drop_base_key(r0, ql, Tn, H, h) + (uint64_t)(8 * rq + 4 * g + e) * (uint64_t)Tn, dth) ? dks : 0.f;
          s[r] = p * dm;   // dropped P (feeds dV)
          dp[r] = p * fmaf(dp[r] * dm, scale, dd[e]);
        } else {
          s[r] = p;
          dp[r] = p * fmaf(dp[r], scale, dd[e]);
        }
      }
    }
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;
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
        mma_chunk<T>(dv[dt], load_t_chunk<T>(tD, 0, cc, lane, dt), pb);
        mma_chunk<T>(dk[dt], load_t_chunk<T>(tQ, 0, cc, lane, dt), sb);
      }
    }
    store_rows_via_lds<T>(tK, dk, db + H * HD, ldq, 0, Le, lane);
    store_rows_via_lds<T>(tV, dv, db + 2 * H * HD, ldq, 0, Le, lane);
  }
}
