// Included TWICE by attention.hip, inside its namespaces: ALPRO_TDROP 0 stamps out the kernels NAME_kernel as they have always been, ALPRO_TDROP 1
// the kernels NAME_drop_kernel with dropout on the attention probabilities.  The two are separate texts for the compiler, not one template with a
// flag behind a forwarding kernel: with the body in an inlined function template the p = 0 kernels came out as different machine code
// (other register counts), and they have to stay the code they are.  No include guard.
// ================================================================================================
// temporal attention: one wave per (32 consecutive tokens, head); groups of Tn tokens
// Probability dropout (DROP) follows alpro_attn_fwd's contract with batch = rows / Tn, L = Tn: keep iff drop_keep(seed, ((grp H + h) Tn + q) Tn + k),
// kept probabilities scaled by 1 / (1 - p), lse from the un-dropped row.
template <typename T>
__global__ __launch_bounds__(256) void ALPRO_TKERNEL(attn_temporal_fwd)(const T* __restrict__ qkv, T* __restrict__ out, int64_t rows, int Tn,
                                                                int H, float scale, int64_t units, float* __restrict__ lse ALPRO_TDROP_PARAMS) {
  constexpr bool DROP = ALPRO_TDROP != 0;
#if !ALPRO_TDROP
  constexpr float drop_p = 0.f;
  constexpr uint32_t drop_seed = 0u;
#endif
  typedef TileCfg<T> C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* Vs = smem + wave * 32 * C::RB;
  const int64_t ldq = 3 * (int64_t)H * HD;
  const int g = lane >> 5, ql = lane & 31;
  const int64_t iters = (units + (int64_t)gridDim.x * 4 - 1) / ((int64_t)gridDim.x * 4);
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t unit = (it * gridDim.x + blockIdx.x) * 4 + wave;
    const bool active = unit < units;
    const int64_t chunk = active ? unit / H : 0;
    const int h = active ? (int)(unit - chunk * H) : 0;
    const int64_t r0 = chunk * 32;
    const T* base = qkv + h * HD;
    // V tile -> wave-private LDS (coalesced: CPR lanes cover one 64-wide row)
    __syncthreads();  // previous iteration's column reads are done
#pragma unroll
    for (int i = 0; i < C::CPR / 2; ++i) {
      const int c = lane + i * 64, row = c / C::CPR, ch = c - row * C::CPR;
      u32x4 vv = mk4(0, 0, 0, 0);
      if (active && r0 + row < rows) vv = *(const u32x4*)(base + (r0 + row) * ldq + 2 * H * HD + ch * C::CN);
      *(u32x4*)(Vs + row * C::RB + (v_swz<T>(row, ch) << 4)) = vv;
    }
    const int64_t qrow = min(r0 + ql, rows - 1);
    u32x4 qf[C::KS], kf[C::KS];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      const T* src = base + qrow * ldq + (2 * ks + g) * C::CN;
      qf[ks] = *(const u32x4*)src;
      kf[ks] = *(const u32x4*)(src + H * HD);
    }
    f32x16 s[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) s[0][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) mma_chunk<T>(s[0], kf[ks], qf[ks]);
    const int qgrp = ql / Tn;
    const float l_se = softmax_tiles<1>(s, scale, [&](int, int rq) {
      const int k0 = 8 * rq + 4 * g;  // block-diagonal mask: a query attends to the T frames of its own patch
      return make_float4((k0 + 0) / Tn == qgrp ? 0.f : -INFINITY, (k0 + 1) / Tn == qgrp ? 0.f : -INFINITY,
                         (k0 + 2) / Tn == qgrp ? 0.f : -INFINITY, (k0 + 3) / Tn == qgrp ? 0.f : -INFINITY);
    });
    if (lse && active && g == 0) lse[unit * 32 + ql] = l_se;  // (chunk*H + h)*32 + token
    if constexpr (DROP) {
      const uint32_t th = drop_thresh24(drop_p);
      const float dks = 1.0f / (1.0f - drop_p);
      const uint64_t base_i = temporal_drop_base(r0, ql, Tn, H, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) s[0][r] = drop_keep(drop_seed, base_i + (uint64_t)acc_row(r, lane), th) ? s[0][r] * dks : 0.f;
    }
    __syncthreads();  // V tile visible
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    pv_tiles<T, 1>(o, s, Vs, lane);
    if (active && r0 + ql < rows) store_row64<T>(out + (r0 + ql) * H * HD + h * HD, o, lane);
  }
}

// ================================================================================================
// 16-bit temporal attention, throughput form (round 2): one WAVE per (32 consecutive tokens, head) unit, everything wave-private
// like attn_temporal_bwd16.  The three 4 KiB tiles K, V, Q of the unit go global -> LDS by DMA in 128-byte row pieces (12 copies per
// unit, bank swizzle on the source side) instead of fragment-shaped 16-byte-per-row register loads (32 cache lines per instruction),
// log2-domain softmax with the 1/sum applied to the 32x64 output tile, and the output leaves through the dead K tile as 16-byte row
// stores.  No workgroup barrier: 4 independent waves per workgroup, units handed out grid-stride.
template <typename T>
__global__ __launch_bounds__(256, 2) void ALPRO_TKERNEL(attn_temporal_fwd16)(const T* __restrict__ qkv, T* __restrict__ out, int64_t rows, int Tn, int H,
                                                                    float scale, int64_t units, float* __restrict__ lse ALPRO_TDROP_PARAMS) {
  constexpr bool DROP = ALPRO_TDROP != 0;
#if !ALPRO_TDROP
  constexpr float drop_p = 0.f;
  constexpr uint32_t drop_seed = 0u;
#endif
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int WB = 3 * 4096;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* tK = smem + wave * WB;
  char* tV = tK + 4096;
  char* tQ = tK + 8192;
  const uint32_t lds0 = lds_addr_of(tK);
  const char* zero = (const char*)g_attn_zero;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const int g = lane >> 5, ql = lane & 31;
  const float sl = scale * LOG2E;
  const int qgrp = ql / Tn;
  for (int64_t unit = (int64_t)blockIdx.x * 4 + wave; unit < units; unit += (int64_t)gridDim.x * 4) {
    const int64_t chunk = unit / H;
    const int h = (int)(unit - chunk * H);
    const int64_t r0 = chunk * 32;
    const int Le = (int)((rows - r0) < 32 ? (rows - r0) : 32);
    const T* qb = qkv + r0 * ldq + h * HD;
    // (the previous unit's LDS reads fed MFMAs / global stores that were issued before this point, so they have completed)
#pragma unroll
    for (int piece = 0; piece < 4; ++piece) {
      const int row = piece * 8 + (lane >> 3), slot = lane & 7;
      const bool ok = row < Le;
      const T* src = qb + (int64_t)row * ldq;
      const int ck = (slot ^ ((row >> 1) & 7)) << 3, cv = (slot ^ (((row >> 1) & 1) << 2)) << 3;
      dma16(ok ? (const char*)(src + H * HD + ck) : zero, __builtin_amdgcn_readfirstlane(lds0 + piece * 1024));
      dma16(ok ? (const char*)(src + 2 * H * HD + cv) : zero, __builtin_amdgcn_readfirstlane(lds0 + 4096 + piece * 1024));
      dma16(ok ? (const char*)(src + ck) : zero, __builtin_amdgcn_readfirstlane(lds0 + 8192 + piece * 1024));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    f32x16 s[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) s[0][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int off = ql * 128 + (((2 * ks + g) ^ ((ql >> 1) & 7)) << 4);
      mma_chunk<T>(s[0], *(const u32x4*)(tK + off), *(const u32x4*)(tQ + off));
    }
    // block-diagonal mask: a query attends to the Tn frames of its own patch (vit.py:146-157)
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool mine = ((r & 3) + 8 * (r >> 2) + 4 * g) / Tn == qgrp;
      s[0][r] = mine ? s[0][r] * sl : -INFINITY;
      m = fmaxf(m, s[0][r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = __builtin_amdgcn_exp2f(s[0][r] - m);  // exp2(-inf) == 0 off the diagonal block
      s[0][r] = pr;
      sum += pr;
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if (lse && g == 0 && ql < Le) lse[unit * 32 + ql] = (m + __builtin_amdgcn_logf(sum)) * LN2;  // (chunk*H + h)*32 + token
    if constexpr (DROP) {   // after the row sum: sum and lse are those of the un-dropped probabilities
      const uint32_t th = drop_thresh24(drop_p);
      const float dks = 1.0f / (1.0f - drop_p);
      const uint64_t base_i = temporal_drop_base(r0, ql, Tn, H, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) s[0][r] = drop_keep(drop_seed, base_i + (uint64_t)acc_row(r, lane), th) ? s[0][r] * dks : 0.f;
    }
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    pv_tiles<T, 1>(o, s, tV, lane);
    // O^T (lane = query, 4 consecutive d per register quad) -> row-major rows through the dead K tile
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const uint32_t lo = pack2(o[dt][4 * rq] * inv, o[dt][4 * rq + 1] * inv, (T*)0);
        const uint32_t hi = pack2(o[dt][4 * rq + 2] * inv, o[dt][4 * rq + 3] * inv, (T*)0);
        *(u32x2*)(tK + ql * 128 + (((dt * 4 + rq) ^ ((ql >> 1) & 7)) << 4) + g * 8) = mk2(lo, hi);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // DS ops of one wave complete in order; nothing else touches this tile
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = p * 8 + (lane >> 3), slot = lane & 7;
      const u32x4 v = *(const u32x4*)(tK + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
      if (row < Le) store16_sc1(out + (r0 + row) * ldo + h * HD + slot * 8, v);
    }
  }
}
