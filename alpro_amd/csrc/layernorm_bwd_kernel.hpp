// layernorm_bwd_kernel, the text of both of its forms.  backward.hip includes this file twice:
//   ALPRO_LN_DATA 0  layernorm_bwd_kernel       dx (+ emitted rows) and the parameter gradients: dgamma / dbeta / the emit's colsum_pre
//   ALPRO_LN_DATA 1  layernorm_bwd_data_kernel  dx (+ emitted rows) only -- gamma and beta are frozen (requires_grad == False) and nobody asked
//                                               for colsum_pre: no column sums in registers, no LDS, no partials, no atomics, no reduce launch
// One text for the row arithmetic, so the two forms cannot drift apart; two texts for the compiler, so the first form's machine code is what it
// was before the second existed (a bool template parameter on a shared body is what moved the attention kernels).  The argument
// list is the same (dgamma, dbeta, part go unused in the data form).
#if ALPRO_LN_DATA
#define ALPRO_LNB_KERNEL layernorm_bwd_data_kernel
#define ALPRO_LNB_EMIT emit_row<TE, false>   // the SKIP_CLS emit keeps no column sums either
#else
#define ALPRO_LNB_KERNEL layernorm_bwd_kernel
#define ALPRO_LNB_EMIT emit_row<TE>
#endif
// dx[src(m)] += rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat));  dgamma += dy*xhat;  dbeta += dy
// T = storage type of dy, TE = storage type of the emitted operand rows (the compute dtype; dy itself may be the fp32 stream)
template <typename T, typename TE>
__global__ __launch_bounds__(256) void ALPRO_LNB_KERNEL(const T* __restrict__ dy, int64_t ld_dy, const float* __restrict__ dy2,
                                                            const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma, float eps,
                                                            float* __restrict__ dx, int64_t ld_dx, int accumulate, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int64_t rows, int mode, int p0, int p1, float drop_p,
                                                            uint32_t drop_seed, const EmitArgs em, float* __restrict__ part, float* __restrict__ cls_ws) {
#if !ALPRO_LN_DATA
  __shared__ float red[2][4][LN_D];
#endif
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * 4 + w;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
#if !ALPRO_LN_DATA
  float g[12], ag[12], ab[12], cp[12];
  ln_load(gamma, lane, g);
#pragma unroll
  for (int i = 0; i < 12; ++i) ag[i] = ab[i] = cp[i] = 0.f;
#else
  float g[12], cp[12];   // cp: emit_row's argument, never written in this form
  ln_load(gamma, lane, g);
#endif
  // one row: loads, statistics, dgamma / dbeta terms; fin = its input-gradient row (not stored here)
  auto row_grad = [&](int64_t m, int64_t srow, float (&fin)[12]) {
    float xv[12], d[12];
    ln_load_nt(x + srow * ldx, lane, xv);
    ln_load_t<T>(dy + m * ld_dy, lane, d);
    if (dy2) {  // second gradient stream on the same LN output (fp32 copy consumed as a residual)
      float d2[12];
      ln_load_nt(dy2 + m * LN_D, lane, d2);
#pragma unroll
      for (int i = 0; i < 12; ++i) d[i] += d2[i];
    }
    if (drop_seed) {  // gradient through the dropout applied to this LayerNorm's output
      const uint32_t th = drop_thresh24(drop_p);
      const float ks = 1.0f / (1.0f - drop_p);
#pragma unroll
      for (int i = 0; i < 12; ++i) d[i] = row_drop_keep(drop_seed, m, lane, i, th) ? d[i] * ks : 0.f;
    }
    float mean, rstd;
    ln_stats(xv, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      xv[i] = (xv[i] - mean) * rstd;  // xhat
#if !ALPRO_LN_DATA
      ab[i] += d[i];
      ag[i] += d[i] * xv[i];
#endif
      d[i] *= g[i];             // dy * gamma
      s1 += d[i];
      s2 += d[i] * xv[i];
    }
    s1 = wave_sum(s1) * (1.0f / LN_D);
    s2 = wave_sum(s2) * (1.0f / LN_D);
#pragma unroll
    for (int i = 0; i < 12; ++i) fin[i] = rstd * (d[i] - s1 - xv[i] * s2);
  };
  for (int64_t m = wave; m < rows + em.extra_cls; m += nwaves) {
    if (m >= rows) {  // cast-only rows: the CLS rows a SKIP_CLS-mapped LayerNorm does not touch (their gradient is already final)
      const int64_t r = (m - rows) * (1 + (int64_t)em.p1 * em.p0);
      float v[12];
      ln_load_nt(dx + r * ld_dx, lane, v);
      ALPRO_LNB_EMIT(em, r, lane, v, cp);
      continue;
    }
    const SrcRow src = ln_src_row(mode, p0, p1, m);
    // round 6: the row of dx that the result is added to is fetched WITH the row's x / dy (it used to be read behind the four dependent wave
    // reductions: a second exposed memory latency per row)
    f32x4 cin[3];
    const bool acc_here = accumulate && !src.shared;
    if (acc_here) {
      const float* o = dx + src.row * ld_dx;
#pragma unroll
      for (int i = 0; i < 3; ++i) cin[i] = __builtin_nontemporal_load((const f32x4*)(o + i * 256 + lane * 4));
    }
    float fin[12];  // the finished gradient row
    row_grad(m, src.row, fin);
    if (src.shared) {
      // FRAME_TOKENS: the clip's CLS row receives one term per frame.  With a workspace the term of frame copy m / (N + 1) = b * T + t is
      // parked in cls_ws[b * T + t] and cls_rows_reduce_kernel adds the T terms of a clip in frame order (one writer per row, fixed order);
      // without one, fp32 atomics straight into the row (rounds 1-3: run-to-run differences in the last bit)
      if (cls_ws) {
        float* o = cls_ws + (m / (p1 + 1)) * LN_D;
#pragma unroll
        for (int i = 0; i < 3; ++i) *(float4*)(o + i * 256 + lane * 4) = make_float4(fin[4 * i], fin[4 * i + 1], fin[4 * i + 2], fin[4 * i + 3]);
      } else {
        float* o = dx + src.row * ld_dx;
#pragma unroll
        for (int i = 0; i < 12; ++i) atomicAdd(o + row_col(lane, i), fin[i]);
      }
      continue;
    }
    float* o = dx + src.row * ld_dx;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float* p = o + i * 256 + lane * 4;
      if (acc_here) {
        fin[4 * i] += cin[i].x; fin[4 * i + 1] += cin[i].y; fin[4 * i + 2] += cin[i].z; fin[4 * i + 3] += cin[i].w;
      }
      __builtin_nontemporal_store(f32x4{fin[4 * i], fin[4 * i + 1], fin[4 * i + 2], fin[4 * i + 3]}, (f32x4*)p);
    }
    if (em.mode != ALPRO_EMIT_NONE) ALPRO_LNB_EMIT(em, src.row, lane, fin, cp);
  }
#if !ALPRO_LN_DATA
  // block reduction of dgamma / dbeta (and the emit's column sums).  part != nullptr: this workgroup's sums go to its slot of the caller's
  // workspace -- part[block][3][768] -- and colsum_reduce_kernel adds the slots in a fixed order (bit-reproducible, the default since
  // round 4); part == nullptr: one fp32 atomic per column per workgroup straight into the gradients (no workspace, order varies)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[0][w][i * 256 + lane * 4 + e] = ag[4 * i + e];
      red[1][w][i * 256 + lane * 4 + e] = ab[4 * i + e];
    }
  __syncthreads();
  float* slot = part ? part + (int64_t)blockIdx.x * (3 * LN_D) : nullptr;
  for (int c = threadIdx.x; c < LN_D; c += 256) {
    const float sg = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
    const float sb = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    if (slot) { slot[c] = sg; slot[LN_D + c] = sb; }
    else { atomicAdd(dgamma + c, sg); atomicAdd(dbeta + c, sb); }
  }
  if (em.colsum_pre) {  // bias gradient of the Linear whose output gradient the emitted rows are (before the row scale)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[0][w][i * 256 + lane * 4 + e] = cp[4 * i + e];
    __syncthreads();
    for (int c = threadIdx.x; c < LN_D; c += 256) {
      const float sc = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
      if (slot) slot[2 * LN_D + c] = sc;
      else atomicAdd(em.colsum_pre + c, sc);
    }
  }
#endif
}
#undef ALPRO_LNB_KERNEL
#undef ALPRO_LNB_EMIT
