// Included TWICE by attention_temporal_any.hip, inside its namespaces: ALPRO_TDROP 0 stamps out the kernels NAME_kernel as they have always been, ALPRO_TDROP 1
// the kernels NAME_drop_kernel with dropout on the attention probabilities.  The two are separate texts for the compiler, not one template with a
// flag behind a forwarding kernel: with the body in an inlined function template the p = 0 kernels came out as different machine code
// (other register counts), and they have to stay the code they are.  No include guard.
// ================================================================================================
// forward: grid-stride over units = ceil(rows / 32) * H, 4 waves per workgroup
// DROP: probability dropout with the contract of alpro_attn_fwd for batch = rows / T, L = T: keep iff drop_keep(seed, ((grp H + h) T + q) T + k).
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 3 : 2) void ALPRO_TKERNEL(tattn_any_fwd)(const T* __restrict__ qkv, T* __restrict__ out, int64_t rows, int Tn, int H, float scale,
                                                            int64_t units, float* __restrict__ lse ALPRO_TDROP_PARAMS) {
  constexpr bool DROP = ALPRO_TDROP != 0;
#if !ALPRO_TDROP
  constexpr float drop_p = 0.f;
  constexpr uint32_t drop_seed = 0u;
#endif
  typedef TCfg<T> C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* Vs = smem + wave * C::IMG;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const int g = lane >> 5, ql = lane & 31;
  const float sl = scale * LOG2E;
  for (int64_t unit = (int64_t)blockIdx.x * 4 + wave; unit < units; unit += (int64_t)gridDim.x * 4) {
    const int64_t chunk = unit / H;
    const int h = (int)(unit - chunk * H);
    const int64_t r0 = chunk * 32;
    int64_t rend, w0, w1;
    tattn_window(r0, rows, Tn, rend, w0, w1);
    const int nt = (int)((w1 - w0 + 31) >> 5);
    const int64_t qc = min(r0 + ql, rows - 1);
    const int gs = (int)((qc - w0) / Tn) * Tn;   // this query's keys: window rows [gs, gs + Tn)
    const T* base = qkv + h * HD;
    DropBase dbase = {};   // mask index of window row kk for this query: base + kk (64 bits: rows * H * T passes 2^32 at large batches)
    if constexpr (DROP) dbase = drop_base((((uint64_t)((w0 + gs) / Tn) * H + h) * Tn + (uint64_t)(qc - w0 - gs)) * Tn - (uint64_t)gs);
    u32x4 qf[C::KS];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) qf[ks] = *(const u32x4*)(base + qc * ldq + (2 * ks + g) * C::CN);
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int t = 0; t < nt; ++t) {
      const int64_t k0 = w0 + 32 * t;
      wave_lds_sync();   // the previous tile's V reads are done
      stage_tile<T>(Vs, base + 2 * H * HD, ldq, k0, w1, lane);
      const int64_t kr = min(k0 + ql, w1 - 1);
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) mma_chunk<T>(s, *(const u32x4*)(base + kr * ldq + H * HD + (2 * ks + g) * C::CN), qf[ks]);
      float mb = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = 32 * t + acc_row(r, lane);
        const float v = kk >= gs && kk < gs + Tn ? s[r] * sl : -INFINITY;
        s[r] = v;
        mb = fmaxf(mb, v);
      }
      mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
      const float mn = fmaxf(m, mb);
      const float mr = mn == -INFINITY ? 0.f : mn;          // no key of this query's group seen yet: p = 0, nothing to rescale
      const float alpha = __builtin_amdgcn_exp2f(m - mr);   // exp2(-inf) == 0 before the first key
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[r] - mr);   // exp2(-inf) == 0 for keys of other groups
        s[r] = p;
        ps += p;
      }
      ps += __shfl_xor(ps, 32, 64);
      l = fmaf(l, alpha, ps);   // the row sum (and lse) are those of the un-dropped probabilities
      m = mn;
      if constexpr (DROP) {
        const uint32_t th = drop_thresh24(drop_p);
        const float dks = 1.0f / (1.0f - drop_p);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = drop_keep(drop_seed, dbase, (uint32_t)(32 * t + acc_row(r, lane)), th) ? s[r] * dks : 0.f;
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
      wave_lds_sync();   // V tile visible
#pragma unroll
      for (int cc = 0; cc < C::CPT; ++cc) {
        float pv[C::CN];
#pragma unroll
        for (int e = 0; e < C::CN; ++e) pv[e] = s[cc * C::CN + e];
        const u32x4 bop = pack_chunk<T>(pv);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(o[dt], load_t_chunk<T>(Vs, 0, cc, lane, dt), bop);
      }
    }
    if (r0 + ql < rows) {
      const float inv = 1.0f / l;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= inv;
      store_row64<T>(out + (r0 + ql) * ldo + h * HD, o, lane);
      if (lse && g == 0) lse[unit * 32 + ql] = (m + __log2f(l)) * LN2;   // (chunk * H + h) * 32 + row
    }
  }
}

// ================================================================================================
// backward: grid-stride over the same units; per wave two staged tiles, 32 lse and 32 delta values
// DROP: the mask is regenerated from the seed; dP = keep / (1 - p) * (dO V^T), delta = rowsum(dO o O) with the dropped O, P recomputed from lse.
template <typename T>
// (the 16-bit dropout form does not fit the 256 registers of two workgroups per CU without spilling: one per CU there, as in fp32; p = 0 keeps two)
__global__ __launch_bounds__(256, sizeof(T) == 2 && !ALPRO_TDROP ? 2 : 1) void ALPRO_TKERNEL(tattn_any_bwd)(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                            const float* __restrict__ lse, T* __restrict__ dqkv, int64_t rows, int Tn, int H,
                                                            float scale, int64_t units ALPRO_TDROP_PARAMS) {
  constexpr bool DROP = ALPRO_TDROP != 0;
#if !ALPRO_TDROP
  constexpr float drop_p = 0.f;
  constexpr uint32_t drop_seed = 0u;
#endif
  typedef TCfg<T> C;
  constexpr int WB = 2 * C::IMG + 64 * sizeof(float);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* tA = smem + wave * WB;   // K (dQ phase) / Q (dK-dV phase)
  char* tB = tA + C::IMG;        // dO (dK-dV phase)
  float* Ls = (float*)(tB + C::IMG);   // lse * log2(e) of the staged query rows
  float* Ds = Ls + 32;                 // delta of the staged query rows
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const int g = lane >> 5, ql = lane & 31;
  const float sl = scale * LOG2E;
  for (int64_t unit = (int64_t)blockIdx.x * 4 + wave; unit < units; unit += (int64_t)gridDim.x * 4) {
    const int64_t chunk = unit / H;
    const int h = (int)(unit - chunk * H);
    const int64_t r0 = chunk * 32;
    int64_t rend, w0, w1;
    tattn_window(r0, rows, Tn, rend, w0, w1);
    const int nt = (int)((w1 - w0 + 31) >> 5);
    const int64_t rc = min(r0 + ql, rows - 1);   // this lane's row of the unit: a query in the dQ phase, a key in the dK / dV phase
    const int gs = (int)((rc - w0) / Tn) * Tn;   // its group: window rows [gs, gs + Tn)
    const bool live = r0 + ql < rows;
    const uint32_t dth = drop_thresh24(drop_p);
    const float dks = DROP ? 1.0f / (1.0f - drop_p) : 1.0f;
    // mask index (64 bits) of this lane's row against window row w: as a query, base (gh + pos) Tn - gs, + w (w a key); as a key, base
    // (gh - gs) Tn + pos, + w Tn (w a query); gh = (group H + h) Tn from the window's first group (wave-uniform) and the lane's group inside it
    const uint64_t gh = DROP ? ((uint64_t)(w0 / Tn) * H + h) * Tn + (uint64_t)(gs / Tn) * (uint64_t)(H * Tn) : 0, pos = (uint64_t)((int)(rc - w0) - gs);
    const T* base = qkv + h * HD;
    const T* ob = out + h * HD;
    const T* dob = dout + h * HD;

    // ---- dQ: the unit's queries against the window's keys
    {
      DropBase dq_i = {};
      if constexpr (DROP) dq_i = drop_base((gh + pos) * Tn - (uint64_t)gs);
      u32x4 qf[C::KS], dof[C::KS];
      float delta = 0.f;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        const int off = (2 * ks + g) * C::CN;
        qf[ks] = *(const u32x4*)(base + rc * ldq + off);
        dof[ks] = *(const u32x4*)(dob + rc * ldo + off);
        float a[C::CN], c2[C::CN];
        unpack_chunk<T>(dof[ks], a);
        unpack_chunk<T>(*(const u32x4*)(ob + rc * ldo + off), c2);
#pragma unroll
        for (int e = 0; e < C::CN; ++e) delta = fmaf(a[e], c2[e], delta);
      }
      delta += __shfl_xor(delta, 32, 64);
      const float lq = lse[((rc >> 5) * H + h) * 32 + (rc & 31)] * LOG2E;
      f32x16 dq[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
      for (int t = 0; t < nt; ++t) {
        const int64_t k0 = w0 + 32 * t;
        wave_lds_sync();
        stage_tile<T>(tA, base + H * HD, ldq, k0, w1, lane);
        const int64_t kr = min(k0 + ql, w1 - 1);
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
          const int off = (2 * ks + g) * C::CN;
          mma_chunk<T>(s, *(const u32x4*)(base + kr * ldq + H * HD + off), qf[ks]);
          mma_chunk<T>(dp, *(const u32x4*)(base + kr * ldq + 2 * H * HD + off), dof[ks]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = 32 * t + acc_row(r, lane);
          const float p = kk >= gs && kk < gs + Tn ? __builtin_amdgcn_exp2f(fmaf(s[r], sl, -lq)) : 0.f;
          if constexpr (DROP) dp[r] = drop_keep(drop_seed, dq_i, (uint32_t)kk, dth) ? dp[r] * dks : 0.f;
          s[r] = p * (dp[r] - delta) * scale;   // dS^T
        }
        wave_lds_sync();   // K tile visible
#pragma unroll
        for (int cc = 0; cc < C::CPT; ++cc) {
          float v[C::CN];
#pragma unroll
          for (int e = 0; e < C::CN; ++e) v[e] = s[cc * C::CN + e];
          const u32x4 bop = pack_chunk<T>(v);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(dq[dt], load_t_chunk<T>(tA, 0, cc, lane, dt), bop);
        }
      }
      if (live) store_row64<T>(dqkv + (r0 + ql) * ldq + h * HD, dq, lane);
    }

    // ---- dK / dV: the unit's keys against the window's queries
    {
      DropBase dk_i = {};
      if constexpr (DROP) dk_i = drop_base((gh - (uint64_t)gs) * Tn + pos);
      u32x4 kf[C::KS], vf[C::KS];
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        const int off = (2 * ks + g) * C::CN;
        kf[ks] = *(const u32x4*)(base + rc * ldq + H * HD + off);
        vf[ks] = *(const u32x4*)(base + rc * ldq + 2 * H * HD + off);
      }
      f32x16 dk[2], dv[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;
      for (int t = 0; t < nt; ++t) {
        const int64_t q0 = w0 + 32 * t;
        wave_lds_sync();
        stage_tile<T>(tA, base, ldq, q0, w1, lane);
        {   // dO rows -> tB, delta of each row -> Ds (its CPR chunks sit in CPR consecutive lanes), lse -> Ls
          u32x4 dv4[C::NLD], ov4[C::NLD];
#pragma unroll
          for (int i = 0; i < C::NLD; ++i) {
            const int c = lane + 64 * i, row = c / C::CPR, ch = c - row * C::CPR;
            const bool ok = q0 + row < w1;
            dv4[i] = ok ? *(const u32x4*)(dob + (q0 + row) * ldo + ch * C::CN) : mk4(0u, 0u, 0u, 0u);
            ov4[i] = ok ? *(const u32x4*)(ob + (q0 + row) * ldo + ch * C::CN) : mk4(0u, 0u, 0u, 0u);
          }
          const int64_t qr = q0 + ql;
          const float lv = qr < w1 ? lse[((qr >> 5) * H + h) * 32 + (qr & 31)] * LOG2E : 0.f;
#pragma unroll
          for (int i = 0; i < C::NLD; ++i) {
            const int c = lane + 64 * i, row = c / C::CPR, ch = c - row * C::CPR;
            *(u32x4*)(tB + tile_off<T>(row, ch)) = dv4[i];
            float a[C::CN], c2[C::CN];
            unpack_chunk<T>(dv4[i], a);
            unpack_chunk<T>(ov4[i], c2);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < C::CN; ++e) d = fmaf(a[e], c2[e], d);
#pragma unroll
            for (int o = C::CPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
            if (ch == 0) Ds[row] = d;
          }
          if (g == 0) Ls[ql] = lv;
        }
        wave_lds_sync();   // Q, dO, lse, delta visible
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
          mma_chunk<T>(s, *(const u32x4*)(tA + tile_off<T>(ql, 2 * ks + g)), kf[ks]);
          mma_chunk<T>(dp, *(const u32x4*)(tB + tile_off<T>(ql, 2 * ks + g)), vf[ks]);
        }
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float4 lq4 = *(const float4*)(Ls + 8 * rq + 4 * g);
          const float4 dd4 = *(const float4*)(Ds + 8 * rq + 4 * g);
          const float ll[4] = {lq4.x, lq4.y, lq4.z, lq4.w}, dd[4] = {dd4.x, dd4.y, dd4.z, dd4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rq + e, qq = 32 * t + 8 * rq + 4 * g + e;
            const float p = qq >= gs && qq < gs + Tn ? __builtin_amdgcn_exp2f(fmaf(s[r], sl, -ll[e])) : 0.f;
            float dm = 1.0f;
            if constexpr (DROP) dm = drop_keep(drop_seed, dk_i, (uint32_t)(qq * Tn), dth) ? dks : 0.f;
            s[r] = p * dm;                                // (dropped) P (feeds dV)
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
            mma_chunk<T>(dv[dt], load_t_chunk<T>(tB, 0, cc, lane, dt), pb);
            mma_chunk<T>(dk[dt], load_t_chunk<T>(tA, 0, cc, lane, dt), sb);
          }
        }
      }
      if (live) {
        store_row64<T>(dqkv + (r0 + ql) * ldq + H * HD + h * HD, dk, lane);
        store_row64<T>(dqkv + (r0 + ql) * ldq + 2 * H * HD + h * HD, dv, lane);
      }
    }
  }
}
