// Memory-bound backward kernels: transposes feeding the NT GEMM for dgrad / wgrad, LayerNorm backward
// (with the row maps of the forward gather turned into scatters), CLS-mean / final-pool (all three pooling modes) / BERT-embedding
// backward, and the GELU-gradient multiply.  All HBM-bound; 16-byte accesses wherever rows are contiguous.
#include "common.hpp"
#include "row768.hpp"
#include <algorithm>

namespace alpro {
namespace {

// ---- out[c, r] = (Tout) in[r, c] for r < R, zero for R <= r < Rpad; optional fp32 column sums (bias gradient) --
// 64x64 tile through LDS (fp32, +1 padding).  wgrad needs both operands with the token dimension contiguous.
template <typename Tin, typename Tout>
__device__ __forceinline__ void transpose_tile(float (&tile)[64][65], const Tin* __restrict__ in, int64_t ld_in, Tout* __restrict__ out,
                                               int64_t ld_out, int R, int C, int Rpad, float* __restrict__ colsum, int bx, int by) {
  const int r0 = by * 64, c0 = bx * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 4 row-groups of 64 lanes
#pragma unroll 4
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < C) ? to_f32(in[(int64_t)r * ld_in + c]) : 0.f;
  }
  __syncthreads();
  if (colsum && ty == 0 && c0 + tx < C) {
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) s += tile[i][tx];
    atomicAdd(colsum + c0 + tx, s);
  }
#pragma unroll 4
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < Rpad) out[(int64_t)c * ld_out + r] = from_f32<Tout>(tile[tx][i]);
  }
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void transpose_kernel(const Tin* __restrict__ in, int64_t ld_in, Tout* __restrict__ out, int64_t ld_out,
                                                        int R, int C, int Rpad, float* __restrict__ colsum) {
  __shared__ float tile[64][65];
  transpose_tile<Tin, Tout>(tile, in, ld_in, out, ld_out, R, C, Rpad, colsum, blockIdx.x, blockIdx.y);
}

// Many independent transposes in ONE launch: the dgrad operands W^T of every Linear are refreshed after each optimizer step, ~130
// matrices of 0.6-2.4 M elements -- each far too small to cover its own launch (10 us apiece, 2 ms per step as separate launches).
// Workgroup -> job by binary search over the jobs' first-tile prefix (uniform, a handful of scalar loads).
template <typename Tout>
__global__ __launch_bounds__(256) void transpose_batch_kernel(const alpro_transpose_job_t* __restrict__ jobs, int njobs) {
  __shared__ float tile[64][65];
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile0 <= (int)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const alpro_transpose_job_t jb = jobs[lo];
  const int t = blockIdx.x - jb.tile0, tcx = (jb.C + 63) / 64;
  transpose_tile<float, Tout>(tile, jb.in, jb.ld_in, (Tout*)jb.out, jb.ld_out, jb.R, jb.C, jb.Rpad, nullptr, t % tcx, t / tcx);
}

// ---- LayerNorm backward, D = 768, one wave per row ------------------------------------------------------
constexpr int LN_PART_BYTES = 3 * LN_D * (int)sizeof(float);  // one workgroup's column sums in the reduction workspace: dgamma | dbeta | colsum_pre

// What the backward does NEXT with the gradient row this kernel has just finished (round 3): every LayerNorm backward of the path is
// followed by an alpro_gather_cast that re-reads the fp32 row it wrote, scales it and casts it into the operand rows of the next
// wgrad / dgrad GEMMs (3.6 ms per training step, 308 MB re-read per call at B = 64).  With an emit mode the row leaves this kernel in
// both forms -- fp32 into the gradient stream and `dtype` into the GEMM operand -- and that pass disappears.  `r` = token row of dx:
//   ALPRO_EMIT_ROWS      out[r] = drop(v) * scale[r / group]                      (BERT: the dense-output dropout of xbert.py:358,436;
//                        ViT temporal LayerNorm -> the previous block's MLP gradient, scale = its drop-path row scale, group = 1 + N*T)
//   ALPRO_EMIT_FRAME     r = b*S + k.  k > 0 (patch n, frame t): out[(b*T+t)*(N+1) + 1 + n] = v * scale[b*T+t];
//                        k = 0: out[(b*T+t)*(N+1)] = v * scale[b*T+t] / T for every t   (inverse of vit.py:184-196; after norm2's backward)
//   ALPRO_EMIT_SKIP_CLS  k > 0: out[r - b - 1] = v * scale[(r - b - 1) / group]; colsum_pre[c] += v (unscaled: the bias gradient of
//                        temporal_fc); CLS rows emit nothing                      (after norm1's backward)
struct EmitArgs {
  void* out;
  int mode, p0, p1;          // p0 = T, p1 = N for the divided space-time modes
  const float* scale;
  int group;
  float drop_p;
  uint32_t drop_seed;
  float* colsum_pre;
  int extra_cls;             // ROWS mode after a SKIP_CLS-mapped LayerNorm: also emit the B CLS rows (final since the previous kernel)
};

// emit the finished gradient row `v` of token row r (see EmitArgs); cp accumulates the unscaled column sums (SKIP_CLS mode; CP = false:
// nobody wants them -- the data-only LayerNorm backward -- and cp is left alone)
template <typename T, bool CP = true>
__device__ __forceinline__ void emit_row(const EmitArgs& e, int64_t r, int lane, float (&v)[12], float (&cp)[12]) {
  T* out = (T*)e.out;
  if (e.mode == ALPRO_EMIT_ROWS) {
    if (e.drop_seed) {
      const uint32_t th = drop_thresh24(e.drop_p);
      const float ks = 1.0f / (1.0f - e.drop_p);
#pragma unroll
      for (int i = 0; i < 12; ++i) v[i] = row_drop_keep(e.drop_seed, r, lane, i, th) ? v[i] * ks : 0.f;
    }
    ln_store_scaled<T>(out + r * LN_D, lane, v, e.scale ? e.scale[r / e.group] : 1.0f);
    return;
  }
  const int Tn = e.p0, N = e.p1;
  const int64_t S = 1 + (int64_t)N * Tn;
  const int64_t b = r / S, k = r - b * S;
  if (e.mode == ALPRO_EMIT_FRAME) {
    if (k == 0) {
      const float inv = 1.0f / (float)Tn;
      for (int t = 0; t < Tn; ++t) ln_store_scaled<T>(out + ((b * Tn + t) * (N + 1)) * LN_D, lane, v, (e.scale ? e.scale[b * Tn + t] : 1.0f) * inv);
    } else {
      const int64_t n = (k - 1) / Tn;
      const int t = (int)((k - 1) - n * Tn);
      ln_store_scaled<T>(out + ((b * Tn + t) * (N + 1) + 1 + n) * LN_D, lane, v, e.scale ? e.scale[b * Tn + t] : 1.0f);
    }
  } else {  // SKIP_CLS
    if (k == 0) return;
    const int64_t o = r - b - 1;
    if constexpr (CP) {
#pragma unroll
      for (int i = 0; i < 12; ++i) cp[i] += v[i];
    }
    ln_store_scaled<T>(out + o * LN_D, lane, v, e.scale ? e.scale[o / e.group] : 1.0f);
  }
}

#define ALPRO_LN_DATA 0
#include "layernorm_bwd_kernel.hpp"
#undef ALPRO_LN_DATA
#define ALPRO_LN_DATA 1
#include "layernorm_bwd_kernel.hpp"
#undef ALPRO_LN_DATA

// dst_k[c] += sum over workgroup slots p of part[p][nslots][768] for the column sums k = 0 .. gridDim.y-1: ONE workgroup per (32 columns, k)
// -- 8 float4 column lanes x 128 slices of slots.  Slice s adds slots s, s + 128, ... in ascending order; then 8 x 8 lanes add 16 slice sums
// each (ascending) and one lane per column group adds those 8: a single writer per output and an order that depends on nothing but the slot
// count -- bit-reproducible.  (72 workgroups; the first form -- 36 workgroups of 64 columns, one lane walking all 64 slice sums -- took 13 us
// for 2048 slots.)
__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const float* __restrict__ part, int nparts, int nslots, float* __restrict__ d0,
                                                             float* __restrict__ d1, float* __restrict__ d2) {
  __shared__ float4 red[128][8];
  __shared__ float4 red2[8][8];
  const int k = blockIdx.y, c4 = threadIdx.x & 7, sl = threadIdx.x >> 3;
  float* dst = k == 0 ? d0 : (k == 1 ? d1 : d2);
  if (!dst) return;
  const int col = blockIdx.x * 32 + c4 * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int p = sl; p < nparts; p += 128) {
    const float4 v = *(const float4*)(part + ((int64_t)p * nslots + k) * LN_D + col);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  red[sl][c4] = s;
  __syncthreads();
  if (sl < 8) {
    float4 t = red[sl * 16][c4];
#pragma unroll
    for (int i = 1; i < 16; ++i) { const float4 v = red[sl * 16 + i][c4]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    red2[sl][c4] = t;
  }
  __syncthreads();
  if (sl == 0) {
    float4 t = red2[0][c4];
#pragma unroll
    for (int i = 1; i < 8; ++i) { const float4 v = red2[i][c4]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    float4* o = (float4*)(dst + col);
    const float4 c = *o;
    *o = make_float4(c.x + t.x, c.y + t.y, c.z + t.z, c.w + t.w);
  }
}

// dx[clip b's CLS row] += sum over the T frame terms parked in cls_ws[b * T + t] by layernorm_bwd_kernel, t ascending: one workgroup of 192
// lanes (float4 each) per clip.
__global__ __launch_bounds__(192) void cls_rows_reduce_kernel(const float* __restrict__ cls_ws, float* __restrict__ dx, int64_t ld_dx, int T, int N) {
  const int b = blockIdx.x, c = threadIdx.x * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = 0; t < T; ++t) {
    const float4 v = *(const float4*)(cls_ws + ((int64_t)b * T + t) * LN_D + c);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  float4* o = (float4*)(dx + (int64_t)b * (1 + (int64_t)N * T) * ld_dx + c);
  const float4 cur = *o;
  *o = make_float4(cur.x + s.x, cur.y + s.y, cur.z + s.z, cur.w + s.w);
}

// ---- final norm + pooling backward (ALPRO_POOL_*): the un-pooling folded into the LayerNorm backward -------------------------------------
// One wave per TOKEN row r = b*S + k of x, so dx has one writer per row and needs neither a map nor accumulation; the row's dy is read out of
// the pooled gradient where it lies (patch n, frame t):
//   TEMPORAL  dout (B, 1+N):    k = 0: dout[b, 0];  else dout[b, 1+n] / T
//   SPATIAL   dout (B, 1+T):    k = 0: dout[b, 0];  else dout[b, 1+t] / N
//   NONE      dout (B, T, 1+N): k = 0: sum_t dout[b, t, 0] (t ascending);  else dout[b, t, 1+n]
// The arithmetic of a row, the dgamma / dbeta partials (part[workgroup][2][768] for colsum_reduce_kernel, or atomics) and the ROWS emit are
// those of layernorm_bwd_kernel; that kernel's own code stays as it is (it is shared with every other LayerNorm of the path).
template <typename TE, int MODE>
__global__ __launch_bounds__(256) void vit_final_pool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 float eps, float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                 int64_t rows, int Tn, int N, const EmitArgs em, float* __restrict__ part) {
  __shared__ float red[2][4][LN_D];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int64_t S = 1 + (int64_t)N * Tn;
  float g[12], ag[12], ab[12], cp[12];
  ln_load(gamma, lane, g);
#pragma unroll
  for (int i = 0; i < 12; ++i) ag[i] = ab[i] = cp[i] = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < rows; r += nwaves) {
    const int64_t b = r / S, k = r - b * S;
    const int64_t n = k ? (k - 1) / Tn : 0;
    const int t = k ? (int)((k - 1) - n * Tn) : 0;
    int64_t src;     // row of dout
    float sc = 1.0f;
    if constexpr (MODE == ALPRO_POOL_TEMPORAL) {
      src = b * (N + 1) + (k ? 1 + n : 0);
      if (k) sc = 1.0f / (float)Tn;
    } else if constexpr (MODE == ALPRO_POOL_SPATIAL) {
      src = b * (Tn + 1) + (k ? 1 + t : 0);
      if (k) sc = 1.0f / (float)N;
    } else {
      src = (b * Tn + t) * (N + 1) + (k ? 1 + n : 0);
    }
    float xv[12], d[12];
    ln_load_nt(x + r * LN_D, lane, xv);
    ln_load(dout + src * LN_D, lane, d);   // plain: a pooled row is read by the T (N) token rows it was averaged over
    if (MODE == ALPRO_POOL_NONE && k == 0) {
      for (int f = 1; f < Tn; ++f) {
        float d2[12];
        ln_load(dout + (src + (int64_t)f * (N + 1)) * LN_D, lane, d2);
#pragma unroll
        for (int i = 0; i < 12; ++i) d[i] += d2[i];
      }
    }
    float mean, rstd;
    ln_stats(xv, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      d[i] *= sc;
      xv[i] = (xv[i] - mean) * rstd;  // xhat
      ab[i] += d[i];
      ag[i] += d[i] * xv[i];
      d[i] *= g[i];
      s1 += d[i];
      s2 += d[i] * xv[i];
    }
    s1 = wave_sum(s1) * (1.0f / LN_D);
    s2 = wave_sum(s2) * (1.0f / LN_D);
    float fin[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) fin[i] = rstd * (d[i] - s1 - xv[i] * s2);
    ln_store<float>(dx + r * LN_D, lane, fin);
    if (em.mode != ALPRO_EMIT_NONE) emit_row<TE>(em, r, lane, fin, cp);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    red[0][w][row_col(lane, i)] = ag[i];
    red[1][w][row_col(lane, i)] = ab[i];
  }
  __syncthreads();
  float* slot = part ? part + (int64_t)blockIdx.x * (2 * LN_D) : nullptr;
  for (int c = threadIdx.x; c < LN_D; c += 256) {
    const float sg = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
    const float sb = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    if (slot) { slot[c] = sg; slot[LN_D + c] = sb; }
    else { atomicAdd(dgamma + c, sg); atomicAdd(dbeta + c, sb); }
  }
}

// ---- out[m, :] = (T)(scale(m) * src[row(m), :]): gathers fp32 token-gradient rows into a GEMM operand ---------------
// row(m) follows the forward maps; under FRAME_TOKENS the j == 0 rows read the clip's CLS row times cls_scale (1/T).
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void gather_cast_kernel(const float* __restrict__ src, int64_t ld, T* __restrict__ out, int64_t rows, int mode,
                                                          int p0, int p1, const float* __restrict__ row_scale, int group, float cls_scale,
                                                          float drop_p, uint32_t drop_seed, float* __restrict__ colsum,
                                                          float* __restrict__ colsum_pre, float* __restrict__ part) {
  __shared__ float red[NW][LN_D];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * NW + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * NW;
  float cs[12], cp[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) cs[i] = cp[i] = 0.f;
  auto src_row = [&](int64_t m, float& sc) -> int64_t {
    sc = row_scale ? row_scale[m / group] : 1.0f;
    if (mode == ALPRO_MAP_PATCH_EMBED) {
      const int T_ = p0, N = p1;
      const int64_t bt = m / N;
      const int n = (int)(m - bt * N);
      const int64_t b = bt / T_;
      const int t = (int)(bt - b * T_);
      return b * (1 + (int64_t)N * T_) + 1 + (int64_t)n * T_ + t;
    }
    const SrcRow s = ln_src_row(mode, p0, p1, m);
    if (s.shared) sc *= cls_scale;
    return s.row;
  };
  auto emit = [&](int64_t m, float (&v)[12], float sc) {
    if (drop_seed) {
      const uint32_t th = drop_thresh24(drop_p);
      const float ks = 1.0f / (1.0f - drop_p);
#pragma unroll
      for (int i = 0; i < 12; ++i) v[i] = row_drop_keep(drop_seed, m, lane, i, th) ? v[i] * ks : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      cp[i] += v[i];
      v[i] *= sc;
      cs[i] += v[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      T* p = out + m * LN_D + i * 256 + lane * 4;
      if constexpr (sizeof(T) == 4) {
        __builtin_nontemporal_store(f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]}, (f32x4*)p);
      } else {
        u32x2 u;
        u.x = pack2(v[4 * i], v[4 * i + 1], (T*)0);
        u.y = pack2(v[4 * i + 2], v[4 * i + 3], (T*)0);
        *(u32x2*)p = u;  // ln_store<T> (row768.hpp) written out: the call changes this kernel's register numbers (profiles/r12_rowwise_isa.txt)
      }
    }
  };
  // two rows per wave iteration: both rows' loads are in flight before either is converted (the colsum launch uses a
  // small grid, so each wave walks ~25 rows and would otherwise expose one HBM round trip per row)
  for (int64_t m = wave; m < rows; m += 2 * nwaves) {
    const int64_t m2 = m + nwaves;
    const bool has2 = m2 < rows;
    float sc, sc2 = 0.f;
    const int64_t r = src_row(m, sc);
    const int64_t r2 = has2 ? src_row(m2, sc2) : r;
    float v[12], v2[12];
    ln_load_nt(src + r * ld, lane, v);
    ln_load_nt(src + r2 * ld, lane, v2);
    emit(m, v, sc);
    if (has2) emit(m2, v2, sc2);
  }
  // bias gradients of the Linears these rows are the dY of (after / before the row scale): LDS fold over the waves, then this workgroup's
  // sums go to its workspace slot part[block][2][768] for colsum_reduce_kernel (fixed order), or -- part == nullptr -- one atomic per column
  auto flush = [&](const float (&acc)[12], float* dst, int k) {
    const int w = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 12; ++i) red[w][row_col(lane, i)] = acc[i];
    __syncthreads();
    for (int c = threadIdx.x; c < LN_D; c += NW * 64) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < NW; ++j) t += red[j][c];
      if (part) part[((int64_t)blockIdx.x * 2 + k) * LN_D + c] = t;
      else unsafeAtomicAdd(dst + c, t);
    }
  };
  if (colsum) flush(cs, colsum, 0);
  if (colsum_pre) flush(cp, colsum_pre, 1);
}

// ---- du = dh * gelu'(u) (erf GELU), elementwise over 16-byte chunks ---------------------------------------
template <typename T>
__global__ void gelu_bwd_kernel(const T* __restrict__ dh, const T* __restrict__ u, T* __restrict__ du, int64_t n) {
  constexpr int E = Chunk<T>::N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * E;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * E; i + E <= n; i += stride) {
    float a[E], b[E], o[E];
    unpack_chunk<T>(*(const u32x4*)(dh + i), a);
    unpack_chunk<T>(*(const u32x4*)(u + i), b);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float x = b[e];
      const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
      const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
      o[e] = a[e] * (cdf + x * pdf);
    }
    *(u32x4*)(du + i) = pack_chunk<T>(o);
  }
}

// ---- CLS mean backward: dside[b*T+t] = dx_out[b,0] / T  (rows of the spatial proj output), dx_in[b,0] += dx_out[b,0]
__global__ void cls_mean_bwd_kernel(const float* __restrict__ dx_out, int64_t ldb, float* __restrict__ dside, int B, int T, int D) {
  const int b = blockIdx.x;
  const float inv = 1.0f / (float)T;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float g = dx_out[b * ldb + d] * inv;
    for (int t = 0; t < T; ++t) dside[((int64_t)b * T + t) * D + d] = g;
  }
}

// ---- dst[idx[i], :] += src[i, :] (word / position embedding gradients), D = 768 ---------------------------
// Rows whose index equals skip_idx contribute nothing: nn.Embedding(padding_idx=...) keeps the pad row's gradient at zero (xbert.py:171).
// fp32 atomics: the order of the duplicates' additions varies run to run (the bit-reproducible caller sorts instead, see hip.py).
__global__ __launch_bounds__(256) void scatter_add_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx, float* __restrict__ dst,
                                                               int rows, int idx_mod, int64_t skip_idx) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= rows) return;
  const int64_t r = idx ? idx[m] : (m % idx_mod);
  if (r == skip_idx) return;
  const float* s = src + (int64_t)m * LN_D;
  float* d = dst + r * LN_D;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float4 f = *(const float4*)(s + i * 256 + lane * 4);   // (ln_load + row_col of row768.hpp here: other register counts)
    float* p = d + i * 256 + lane * 4;
    atomicAdd(p, f.x); atomicAdd(p + 1, f.y); atomicAdd(p + 2, f.z); atomicAdd(p + 3, f.w);
  }
}

// idx == nullptr (destination row = m % idx_mod, the position table): one wave per DESTINATION row adds its rows m = r, r + idx_mod, ...
// in ascending order -- single writer, fixed order, no atomics.
__global__ __launch_bounds__(256) void scatter_add_mod_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int idx_mod) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= idx_mod || r >= rows) return;
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (int m = r; m < rows; m += idx_mod) {
    float v[12];
    ln_load_nt(src + (int64_t)m * LN_D, lane, v);
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] += v[i];
  }
  ln_accum_row(dst + (int64_t)r * LN_D, lane, acc);
}

// ---- indexed scatter in a fixed order (round 5): the word-embedding table's gradient (xbert.py:203-210 backward) ---------------------------
// dst[idx[i]] += src[i] with duplicates ([CLS], [SEP], [MASK] appear hundreds of times) added in ascending i, one writer per destination row.
// Rounds 1-4 went through torch's sort-based index_put_ for that (0.36 ms per step of generic sort / gather / scatter kernels).  Two launches
// here: (1) ONE workgroup sorts the composite keys (idx << 13 | i) of up to 8192 rows in LDS (bitonic network, 32 KiB); (2) one wave per
// sorted position: the head of a run of equal destinations sums the run's rows in key order (= ascending i) and adds the total to the table.
constexpr int SCATTER_SORT_MAX = 8192;
__global__ __launch_bounds__(1024) void scatter_sort_keys_kernel(const int64_t* __restrict__ idx, int rows, int64_t dst_rows, uint32_t* __restrict__ keys_out) {
  __shared__ uint32_t k[SCATTER_SORT_MAX];
  // An index outside [0, dst_rows) gets the padding key: its row is DROPPED (sorted behind every valid key, skipped by the run kernel).  Truncated
  // into the 19-bit field it would have landed in somebody else's row -- or beyond the table (torch's index_put_ device-asserts there).
  for (int i = threadIdx.x; i < SCATTER_SORT_MAX; i += 1024) {
    const int64_t d = i < rows ? idx[i] : -1;
    k[i] = (d >= 0 && d < dst_rows) ? (((uint32_t)d << 13) | (uint32_t)i) : 0xFFFFFFFFu;
  }
  __syncthreads();
  for (int size = 2; size <= SCATTER_SORT_MAX; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < SCATTER_SORT_MAX / 2; t += 1024) {
        const int lo = 2 * t - (t & (stride - 1));   // the lower element of the t-th compare-exchange pair at this stride
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint32_t a = k[lo], b = k[hi];
        if ((a > b) == up) {
          k[lo] = b;
          k[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < SCATTER_SORT_MAX; i += 1024) keys_out[i] = k[i];
}

__global__ __launch_bounds__(256) void scatter_add_runs_kernel(const float* __restrict__ src, const uint32_t* __restrict__ keys, float* __restrict__ dst, int rows,
                                                               int64_t skip_idx) {
  const int lane = threadIdx.x & 63;
  const int pos = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pos >= rows) return;
  const uint32_t key = keys[pos];
  if (key == 0xFFFFFFFFu) return;   // padding / an out-of-range index (dst_rows < 2^19: no valid key has this value)
  const uint32_t dest = key >> 13;
  if ((pos > 0 && (keys[pos - 1] >> 13) == dest) || (int64_t)dest == skip_idx) return;   // not the head of its run / the padding row (nn.Embedding(padding_idx))
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (int q = pos; q < rows; ++q) {
    const uint32_t kq = keys[q];
    if ((kq >> 13) != dest) break;
    float v[12];
    ln_load_nt(src + (int64_t)(kq & 8191u) * LN_D, lane, v);
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] += v[i];
  }
  ln_accum_row(dst + (int64_t)dest * LN_D, lane, acc);
}

// ---- small per-block terms of the merged temporal projection W_e = W_fc W_p (vit.py:157-162), all ViT blocks in one launch -------------
//   mode 0 (after an optimizer step):  b1[n] = sum_m W_fc[n, m] b_p[m]                      (the merged bias under the drop-path scale)
//   mode 1 (backward, product rule):   g_fc[n, m] += db1[n] b_p[m];   g_bp[m] += sum_n W_fc[n, m] db1[n]
// One workgroup per (job, 64-column block m0..m0+63) in mode 1 -- a single writer per output element and a fixed summation order, so the
// gradients stay bit-reproducible --, one wave per row n in mode 0.  D = 768.
template <int MODE>
__global__ __launch_bounds__(256) void tproj_small_kernel(const alpro_tproj_job_t* __restrict__ jobs, int D) {
  const alpro_tproj_job_t jb = jobs[blockIdx.y];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (MODE == 0) {
    const int n = blockIdx.x * 4 + w;
    if (n >= D) return;
    const float* row = jb.wfc + (int64_t)n * D;
    float acc = 0.f;
    for (int m = lane * 4; m < D; m += 256) {
      const float4 a = *(const float4*)(row + m), b = *(const float4*)(jb.bp + m);
      acc += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
    }
    acc = wave_sum(acc);
    if (lane == 0) jb.b1[n] = acc;
  } else {
    __shared__ float red[4][64];
    const int m = blockIdx.x * 64 + lane;
    const float bpm = jb.bp[m];
    // eight rows per trip, all 24 loads issued before the first store (round 6: one row per trip was 192 dependent memory round trips per wave,
    // 150 us for a launch that moves 20 MB); the sum over n keeps a fixed order (rows w, w + 4, ... in ascending order)
    float acc = 0.f;
    for (int n0 = w; n0 < D; n0 += 32) {   // D = 768: 24 trips of 8 rows (n0 + 4 k < D for every k)
      float d[8], gf[8], wf[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int n = n0 + 4 * k;
        const int64_t i = (int64_t)n * D + m;
        d[k] = jb.db1[n];
        gf[k] = jb.g_fc[i];
        wf[k] = jb.wfc[i];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        jb.g_fc[(int64_t)(n0 + 4 * k) * D + m] = gf[k] + d[k] * bpm;
        acc = fmaf(wf[k], d[k], acc);
      }
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0) jb.g_bp[m] += (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  }
}

// ---- colsum[n] += sum_m A[m, n] in the order of alpro_gemm_tn_acc_ws's bias gradient: the column sums of a Linear whose WEIGHT is frozen ------
// (requires_grad == False) while its bias is trained, so the dW GEMM that used to produce them does not run.  The sums must keep the bits that
// GEMM gives them (the all-trainable step is the oracle of the frozen-parameter tests), so this kernel restates its additions, not its speed:
//   * the weight-gradient GEMM cuts the tokens into R ranges of `per` 32-token stages; the ceil(K / 256) k-tiles that share a dY column panel take
//     turns, k-tile tk summing the stages with stage % tk_cnt == tk: one partial per (range, k-tile) = "set", set = range * tk_cnt + tk;
//   * inside a stage a lane owns one column and one token half g: tokens ks*16 + 4g + {0..3} and ks*16 + 8 + 4g + {0..3} for ks = 0, 1 (frag8 of
//     gemm_tn.hip), added as ((f0+f1)+(f2+f3))+((f4+f5)+(f6+f7)) onto the running sum, ks = 0 first; the two halves meet at the end (g = 0 + g = 1);
//     rows past M count as zeros;
//   * colsum_tn_reduce_kernel adds the sets as tn_reduce_kernel does: eight interleaved chains (set p, p + 8, ...) and a fixed tree over the eight.
// One wave per (set, 32 columns); every load is a 2-byte element of a 64-byte row segment -- a fraction of HBM speed, on a tensor the skipped GEMM
// would have read anyway.
template <typename T>
__global__ __launch_bounds__(256) void colsum_tn_kernel(const T* __restrict__ A, int64_t lda, int M, int N, int per, int tk_cnt, int total_steps,
                                                        float* __restrict__ part, int npad) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cg = blockIdx.x * 4 + w;
  if (cg * 32 >= npad) return;
  const int col = cg * 32 + (lane & 31), g = lane >> 5;
  const int set = blockIdx.y, range = set / tk_cnt, tk = set - range * tk_cnt;
  const int s0 = range * per, s1 = min(s0 + per, total_steps);
  const bool cv = col < N;
  float cs = 0.f;
  for (int st = s0 + (tk - s0 % tk_cnt + tk_cnt) % tk_cnt; st < s1; st += tk_cnt) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int base = st * 32 + ks * 16 + 4 * g;
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = base + (j & 3) + (j >> 2) * 8;
        f[j] = (cv && m < M) ? to_f32(A[(int64_t)m * lda + col]) : 0.f;
      }
      cs += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
    }
  }
  const float t = cs + __shfl_xor(cs, 32, 64);
  if (lane < 32) part[(int64_t)set * npad + col] = t;
}

__global__ __launch_bounds__(256) void colsum_tn_reduce_kernel(const float* __restrict__ part, int sets, int npad, float* __restrict__ colsum, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float r[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    float t = 0.f;
    for (int s = p; s < sets; s += 8) t += part[(int64_t)s * npad + n];
    r[p] = t;
  }
  colsum[n] += ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

inline int grid_for(int64_t work_items, int per_block, int cap) {
  int64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

template <typename Tin, typename Tout>
int launch_transpose(const void* in, int64_t ld_in, void* out, int64_t ld_out, int R, int C, int Rpad, float* colsum, hipStream_t st) {
  dim3 grid((C + 63) / 64, (Rpad + 63) / 64);
  hipLaunchKernelGGL((transpose_kernel<Tin, Tout>), grid, dim3(256), 0, st, (const Tin*)in, ld_in, (Tout*)out, ld_out, R, C, Rpad, colsum);
  return check_launch("alpro_transpose");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_transpose(const void* in, int in_dtype, int64_t ld_in, void* out, int out_dtype, int64_t ld_out, int R, int C,
                               int Rpad, float* colsum, void* stream) {
  ALPRO_CHECK(in && out && R > 0 && C > 0 && Rpad >= R, "alpro_transpose: bad args");
  ALPRO_CHECK(ld_out >= Rpad && ld_in >= C, "alpro_transpose: leading dimensions too small");
  ALPRO_CHECK(in_dtype == out_dtype || in_dtype == ALPRO_F32, "alpro_transpose: input must be fp32 or the output dtype");
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == ALPRO_F32) {
    ALPRO_DISPATCH_DTYPE(out_dtype, T, return (launch_transpose<float, T>(in, ld_in, out, ld_out, R, C, Rpad, colsum, st)));
  } else {
    ALPRO_DISPATCH_DTYPE(out_dtype, T, return (launch_transpose<T, T>(in, ld_in, out, ld_out, R, C, Rpad, colsum, st)));
  }
  return ALPRO_OK;
}

extern "C" int alpro_transpose_batch(const alpro_transpose_job_t* jobs, int njobs, int total_tiles, int out_dtype, void* stream) {
  ALPRO_CHECK(jobs && njobs > 0 && total_tiles > 0, "alpro_transpose_batch: bad args");
  ALPRO_DISPATCH_DTYPE(out_dtype, T, hipLaunchKernelGGL(transpose_batch_kernel<T>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, jobs, njobs));
  return check_launch("alpro_transpose_batch");
}

extern "C" int alpro_layernorm_bwd_emit(const void* dy, int dy_dtype, int64_t ld_dy, const float* dy2, const float* x, int64_t ldx,
                                        const float* gamma, float eps, float* dx, int64_t ld_dx, int accumulate, float* dgamma, float* dbeta,
                                        int rows, int D, int map_mode, int map_p0, int map_p1, float drop_p, uint32_t drop_seed, void* emit_out,
                                        int emit_dtype, int emit_mode, int emit_p0, int emit_p1, const float* emit_scale, int emit_scale_group, float emit_drop_p,
                                        uint32_t emit_drop_seed, float* emit_colsum_pre, int emit_extra_cls, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  ALPRO_CHECK(dy && x && gamma && dx && rows > 0, "alpro_layernorm_bwd: bad args");
  // dgamma == dbeta == NULL: gamma and beta are frozen -- the data-only form (layernorm_bwd_data_kernel: the same dx and emitted rows, no column sums,
  // no reduce launch).  The two come and go together, and a column sum somebody still wants (colsum_pre: the temporal_fc bias) takes the full kernel:
  // the caller then hands over a throw-away dgamma / dbeta pair.
  ALPRO_CHECK((dgamma != nullptr) == (dbeta != nullptr), "alpro_layernorm_bwd: dgamma and dbeta must both be given or both be NULL (got %s only); "
              "pass a throw-away buffer for the one that is not wanted", dgamma ? "dgamma" : "dbeta");
  const bool data_only = dgamma == nullptr;
  ALPRO_CHECK(!data_only || !emit_colsum_pre, "alpro_layernorm_bwd_emit: colsum_pre needs the column-sum form of the kernel -- pass a throw-away dgamma / dbeta pair with it");
  ALPRO_CHECK(!workspace || (((uintptr_t)workspace % 16) == 0 && workspace_bytes >= LN_PART_BYTES), "alpro_layernorm_bwd: the workspace must be 16-byte aligned and hold at least one workgroup's sums (%d bytes)", LN_PART_BYTES);
  ALPRO_CHECK(D == LN_D, "alpro_layernorm_bwd: D=%d unsupported", D);
  ALPRO_CHECK(map_mode >= 0 && map_mode <= ALPRO_MAP_FRAME_TOKENS, "alpro_layernorm_bwd: bad map_mode %d", map_mode);
  ALPRO_CHECK(map_mode != ALPRO_MAP_FRAME_TOKENS || accumulate, "alpro_layernorm_bwd: the FRAME_TOKENS scatter needs accumulate=1 (CLS rows are shared)");
  ALPRO_CHECK(emit_mode >= ALPRO_EMIT_NONE && emit_mode <= ALPRO_EMIT_SKIP_CLS, "alpro_layernorm_bwd_emit: bad emit_mode %d", emit_mode);
  ALPRO_CHECK(emit_mode == ALPRO_EMIT_NONE || emit_out, "alpro_layernorm_bwd_emit: an emit mode needs the output rows");
  ALPRO_CHECK(emit_mode == ALPRO_EMIT_NONE || ld_dx == LN_D, "alpro_layernorm_bwd_emit: the emit needs a dense gradient stream (ld_dx == 768)");
  ALPRO_CHECK(emit_mode == ALPRO_EMIT_NONE || emit_mode == ALPRO_EMIT_ROWS || (emit_p0 > 0 && emit_p1 > 0), "alpro_layernorm_bwd_emit: FRAME / SKIP_CLS emits need p0 = T, p1 = N");
  ALPRO_CHECK(!emit_scale || emit_scale_group > 0, "alpro_layernorm_bwd_emit: emit_scale_group must be > 0");
  ALPRO_CHECK(!emit_drop_seed || (emit_mode == ALPRO_EMIT_ROWS && emit_drop_p > 0.f && emit_drop_p < 1.f), "alpro_layernorm_bwd_emit: dropout only in ROWS mode, 0 < p < 1");
  ALPRO_CHECK(!emit_colsum_pre || emit_mode == ALPRO_EMIT_SKIP_CLS, "alpro_layernorm_bwd_emit: colsum_pre belongs to the SKIP_CLS emit");
  ALPRO_CHECK(emit_extra_cls == 0 || (emit_mode == ALPRO_EMIT_ROWS && map_mode == ALPRO_MAP_SKIP_CLS && emit_p0 > 0 && emit_p1 > 0),
              "alpro_layernorm_bwd_emit: extra CLS rows go with ROWS emit after a SKIP_CLS-mapped LayerNorm (p0 = T, p1 = N)");
  EmitArgs em;
  em.out = emit_out; em.mode = emit_mode; em.p0 = emit_p0; em.p1 = emit_p1; em.scale = emit_scale; em.group = emit_scale_group;
  em.drop_p = emit_drop_p; em.drop_seed = emit_drop_seed; em.colsum_pre = emit_colsum_pre; em.extra_cls = emit_extra_cls;
  ALPRO_CHECK(emit_mode == ALPRO_EMIT_NONE || emit_dtype == dy_dtype || dy_dtype == ALPRO_F32, "alpro_layernorm_bwd_emit: emit_dtype must be dy's dtype, or any dtype when dy is the fp32 stream");
  // workspace given: the column sums (dgamma, dbeta, colsum_pre) leave as per-workgroup partials and are added in a fixed order by a second
  // small kernel, and the T frame terms of every clip's CLS row (FRAME_TOKENS) are parked behind them for cls_rows_reduce_kernel --
  // bit-reproducible.  Layout: [workgroups][3][768] floats, then [B * T][768] floats; the grid is capped to what fits.  NULL: fp32 atomics.
  const bool frame = map_mode == ALPRO_MAP_FRAME_TOKENS;
  const size_t cls_bytes = frame ? (size_t)(rows / (map_p1 + 1)) * LN_D * sizeof(float) : 0;
  ALPRO_CHECK(!workspace || workspace_bytes >= cls_bytes + LN_PART_BYTES, "alpro_layernorm_bwd: the workspace must hold the CLS frame terms (%zu bytes) and at least one workgroup's sums", cls_bytes);
  // workgroup count: 8 rows per wave at least, 2048 workgroups at most -- two 4-wave workgroups per CU are resident at a time (157 VGPRs, 24 KB LDS), so
  // that is 4 rounds; fewer, fatter workgroups measured slower (tools/ln_bwd_bench.py: 1024: +14 %, 512: +5 %; `ln_grid` overrides the cap)
  const int cap = get_option(OPT_LN_GRID);
  int nblk = grid_for(rows, 4 * 8, cap > 0 ? cap : 256 * 8);
  if (workspace && !data_only) nblk = (int)std::min<size_t>((size_t)nblk, (workspace_bytes - cls_bytes) / LN_PART_BYTES);
  const dim3 grid(nblk), blk(256);
  float* part = data_only ? nullptr : (float*)workspace;   // data-only: no partials; the CLS frame terms lie at the head of the workspace
  float* cls_ws = (workspace && frame) ? (float*)workspace + (data_only ? 0 : (size_t)nblk * 3 * LN_D) : nullptr;
  hipStream_t st = (hipStream_t)stream;
#define ALPRO_LNB(T, TE) \
  do { if (data_only) ALPRO_LNB_K(layernorm_bwd_data_kernel, T, TE); else ALPRO_LNB_K(layernorm_bwd_kernel, T, TE); } while (0)
#define ALPRO_LNB_K(KERNEL, T, TE) hipLaunchKernelGGL((KERNEL<T, TE>), grid, blk, 0, st, (const T*)dy, ld_dy, dy2, x, ldx, gamma, eps, dx, ld_dx, accumulate, dgamma, dbeta, (int64_t)rows, map_mode, map_p0, map_p1, drop_p, drop_seed, em, part, cls_ws)
  if (dy_dtype == ALPRO_F32 && emit_mode != ALPRO_EMIT_NONE && emit_dtype == ALPRO_BF16) ALPRO_LNB(float, bf16_t);
  else if (dy_dtype == ALPRO_F32 && emit_mode != ALPRO_EMIT_NONE && emit_dtype == ALPRO_F16) ALPRO_LNB(float, f16_t);
  else if (dy_dtype == ALPRO_F32) ALPRO_LNB(float, float);
  else if (dy_dtype == ALPRO_BF16) ALPRO_LNB(bf16_t, bf16_t);
  else if (dy_dtype == ALPRO_F16) ALPRO_LNB(f16_t, f16_t);
  else { set_error("alpro_layernorm_bwd: bad dtype %d", dy_dtype); return ALPRO_ERR_INVALID; }
#undef ALPRO_LNB
#undef ALPRO_LNB_K
  if (part) hipLaunchKernelGGL(colsum_reduce_kernel, dim3(LN_D / 32, emit_colsum_pre ? 3 : 2), dim3(1024), 0, st, part, nblk, 3, dgamma, dbeta, emit_colsum_pre);
  if (cls_ws) hipLaunchKernelGGL(cls_rows_reduce_kernel, dim3(rows / (map_p1 + 1) / map_p0), dim3(192), 0, st, cls_ws, dx, ld_dx, map_p0, map_p1);
  return check_launch("alpro_layernorm_bwd");
}

extern "C" int alpro_layernorm_bwd(const void* dy, int dy_dtype, int64_t ld_dy, const float* dy2, const float* x, int64_t ldx,
                                   const float* gamma, float eps, float* dx, int64_t ld_dx, int accumulate, float* dgamma, float* dbeta,
                                   int rows, int D, int map_mode, int map_p0, int map_p1, float drop_p, uint32_t drop_seed, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return alpro_layernorm_bwd_emit(dy, dy_dtype, ld_dy, dy2, x, ldx, gamma, eps, dx, ld_dx, accumulate, dgamma, dbeta, rows, D, map_mode, map_p0, map_p1,
                                  drop_p, drop_seed, nullptr, dy_dtype, ALPRO_EMIT_NONE, 0, 0, nullptr, 1, 0.f, 0u, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int alpro_vit_final_pool_mode_bwd(const float* dout, const float* x, const float* gamma, float eps, float* dx, float* dgamma, float* dbeta,
                                             int mode, int64_t rows, int B, int T, int N, int D, void* emit_out, int emit_dtype, const float* emit_scale,
                                             int emit_scale_group, void* workspace, size_t workspace_bytes, void* stream) {
  constexpr size_t part_bytes = 2 * LN_D * sizeof(float);  // one workgroup's column sums: dgamma | dbeta
  ALPRO_CHECK(dout && x && gamma && dx && dgamma && dbeta && B > 0 && T > 0 && N > 0, "alpro_vit_final_pool_mode_bwd: bad args");
  ALPRO_CHECK(mode >= ALPRO_POOL_TEMPORAL && mode <= ALPRO_POOL_NONE, "alpro_vit_final_pool_mode_bwd: bad mode %d (ALPRO_POOL_TEMPORAL / _SPATIAL / _NONE)", mode);
  ALPRO_CHECK(D == LN_D, "alpro_vit_final_pool_mode_bwd: D=%d unsupported (hidden size is 768 on this path)", D);
  ALPRO_CHECK(rows == (int64_t)B * (1 + (int64_t)N * T), "alpro_vit_final_pool_mode_bwd: rows=%lld is not B * (1 + N * T) = %d * (1 + %d * %d)", (long long)rows, B, N, T);
  ALPRO_CHECK(!workspace || (((uintptr_t)workspace % 16) == 0 && workspace_bytes >= part_bytes), "alpro_vit_final_pool_mode_bwd: the workspace must be 16-byte aligned and hold at least one workgroup's sums (%zu bytes)", part_bytes);
  ALPRO_CHECK(!emit_out || emit_dtype == ALPRO_F32 || emit_dtype == ALPRO_BF16 || emit_dtype == ALPRO_F16, "alpro_vit_final_pool_mode_bwd: bad emit_dtype %d", emit_dtype);
  ALPRO_CHECK(!emit_scale || emit_scale_group > 0, "alpro_vit_final_pool_mode_bwd: emit_scale_group must be > 0");
  EmitArgs em;
  em.out = emit_out; em.mode = emit_out ? ALPRO_EMIT_ROWS : ALPRO_EMIT_NONE; em.p0 = T; em.p1 = N; em.scale = emit_scale; em.group = emit_scale_group;
  em.drop_p = 0.f; em.drop_seed = 0u; em.colsum_pre = nullptr; em.extra_cls = 0;
  const int cap = get_option(OPT_LN_GRID);   // the grid plan of alpro_layernorm_bwd: 8 rows per wave at least, 2048 workgroups at most
  int nblk = grid_for(rows, 4 * 8, cap > 0 ? cap : 256 * 8);
  if (workspace) nblk = (int)std::min<size_t>((size_t)nblk, workspace_bytes / part_bytes);
  const dim3 grid(nblk), blk(256);
  float* part = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
#define ALPRO_FPB(TE, M) hipLaunchKernelGGL((vit_final_pool_bwd_kernel<TE, M>), grid, blk, 0, st, dout, x, gamma, eps, dx, dgamma, dbeta, rows, T, N, em, part)
#define ALPRO_FPB_MODES(TE) \
  do { if (mode == ALPRO_POOL_TEMPORAL) ALPRO_FPB(TE, ALPRO_POOL_TEMPORAL); else if (mode == ALPRO_POOL_SPATIAL) ALPRO_FPB(TE, ALPRO_POOL_SPATIAL); else ALPRO_FPB(TE, ALPRO_POOL_NONE); } while (0)
  if (emit_out && emit_dtype == ALPRO_BF16) ALPRO_FPB_MODES(bf16_t);
  else if (emit_out && emit_dtype == ALPRO_F16) ALPRO_FPB_MODES(f16_t);
  else ALPRO_FPB_MODES(float);
#undef ALPRO_FPB_MODES
#undef ALPRO_FPB
  if (part) hipLaunchKernelGGL(colsum_reduce_kernel, dim3(LN_D / 32, 2), dim3(1024), 0, st, part, nblk, 2, dgamma, dbeta, (float*)nullptr);
  return check_launch("alpro_vit_final_pool_mode_bwd");
}

extern "C" int alpro_gather_cast(const float* src, int64_t ld, void* out, int dtype, int rows, int D, int map_mode, int map_p0, int map_p1,
                                 const float* row_scale, int row_scale_group, float cls_scale, float drop_p, uint32_t drop_seed, float* colsum,
                                 float* colsum_pre, void* workspace, size_t workspace_bytes, void* stream) {
  ALPRO_CHECK(src && out && rows > 0, "alpro_gather_cast: bad args");
  ALPRO_CHECK(!workspace || (((uintptr_t)workspace % 16) == 0 && workspace_bytes >= 2 * LN_D * sizeof(float)), "alpro_gather_cast: the workspace must be 16-byte aligned and hold at least one workgroup's sums");
  ALPRO_CHECK(D == LN_D, "alpro_gather_cast: D=%d unsupported", D);
  ALPRO_CHECK(map_mode >= 0 && map_mode <= ALPRO_MAP_PATCH_EMBED, "alpro_gather_cast: bad map_mode %d", map_mode);
  ALPRO_CHECK(!row_scale || row_scale_group > 0, "alpro_gather_cast: row_scale_group must be > 0");
  // with a colsum target: few, fat workgroups (16 waves) -- every workgroup ends with 768 same-address atomics, and those
  // serialise at the memory side (3072 workgroups cost 2x the whole cast); plain casts use many small workgroups
  if (colsum || colsum_pre) {
    // workspace given: per-workgroup partial sums + the fixed-order colsum_reduce_kernel (bit-reproducible); NULL: fp32 atomics
    float* part = (float*)workspace;
    int nblk = grid_for(rows, 32, 512);
    if (part) nblk = (int)std::min<size_t>((size_t)nblk, workspace_bytes / (2 * LN_D * sizeof(float)));
    ALPRO_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((gather_cast_kernel<T, 16>), dim3(nblk), dim3(1024), 0, (hipStream_t)stream, src, ld, (T*)out, (int64_t)rows, map_mode, map_p0, map_p1, row_scale, row_scale_group, cls_scale, drop_p, drop_seed, colsum, colsum_pre, part));
    if (part) hipLaunchKernelGGL(colsum_reduce_kernel, dim3(LN_D / 32, 2), dim3(1024), 0, (hipStream_t)stream, part, nblk, 2, colsum, colsum_pre, (float*)nullptr);
  } else {
    ALPRO_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((gather_cast_kernel<T, 4>), dim3(grid_for(rows, 8, 256 * 32)), dim3(256), 0, (hipStream_t)stream, src, ld, (T*)out, (int64_t)rows, map_mode, map_p0, map_p1, row_scale, row_scale_group, cls_scale, drop_p, drop_seed, colsum, colsum_pre, (float*)nullptr));
  }
  return check_launch("alpro_gather_cast");
}

extern "C" int alpro_colsum_tn(const void* A, int64_t lda, int dtype, int M, int N, int K, float* colsum, void* workspace, size_t workspace_bytes,
                               void* stream) {
  ALPRO_CHECK(A && colsum && M > 0 && N > 0 && K > 0, "alpro_colsum_tn: bad args");
  ALPRO_CHECK(dtype == ALPRO_BF16 || dtype == ALPRO_F16, "alpro_colsum_tn: 16-bit rows only (it restates the 16-bit weight-gradient GEMM's bias gradient)");
  ALPRO_CHECK(lda >= N, "alpro_colsum_tn: lda must cover N");
  // the token-range plan of the weight-gradient GEMM this launch stands in for (workspace plan, this stream's CU budget)
  const int ranges = alpro_gemm_tn_ranges(M, N, K, cu_budget((hipStream_t)stream));
  const int total_steps = (M + 31) / 32, per = (total_steps + ranges - 1) / ranges, tk_cnt = (K + 255) / 256;
  const int sets = ranges * tk_cnt, npad = (N + 31) / 32 * 32;
  ALPRO_CHECK(workspace && ((uintptr_t)workspace % 16) == 0 && workspace_bytes >= (size_t)sets * npad * sizeof(float),
              "alpro_colsum_tn: the workspace must be 16-byte aligned and hold %d partial sets of %d floats (%zu bytes)", sets, npad, (size_t)sets * npad * sizeof(float));
  float* part = (float*)workspace;
  const dim3 grid((npad / 32 + 3) / 4, sets);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == ALPRO_BF16) hipLaunchKernelGGL(colsum_tn_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)A, lda, M, N, per, tk_cnt, total_steps, part, npad);
  else hipLaunchKernelGGL(colsum_tn_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t*)A, lda, M, N, per, tk_cnt, total_steps, part, npad);
  hipLaunchKernelGGL(colsum_tn_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, st, part, sets, npad, colsum, N);
  return check_launch("alpro_colsum_tn");
}

extern "C" int alpro_tproj_small(const alpro_tproj_job_t* jobs_device, int njobs, int D, int mode, void* stream) {
  ALPRO_CHECK(jobs_device && njobs > 0 && (mode == 0 || mode == 1), "alpro_tproj_small: bad args");
  ALPRO_CHECK(D == LN_D, "alpro_tproj_small: D=%d unsupported", D);
  if (mode == 0) hipLaunchKernelGGL(tproj_small_kernel<0>, dim3(D / 4, njobs), dim3(256), 0, (hipStream_t)stream, jobs_device, D);
  else hipLaunchKernelGGL(tproj_small_kernel<1>, dim3(D / 64, njobs), dim3(256), 0, (hipStream_t)stream, jobs_device, D);
  return check_launch("alpro_tproj_small");
}

extern "C" int alpro_gelu_bwd(const void* dh, const void* u, void* du, int dtype, int64_t n, void* stream) {
  ALPRO_CHECK(dh && u && du && n > 0, "alpro_gelu_bwd: bad args");
  ALPRO_CHECK(n % 8 == 0, "alpro_gelu_bwd: n must be a multiple of 8");
  ALPRO_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(gelu_bwd_kernel<T>, dim3(grid_for(n / Chunk<T>::N, 256, 256 * 16)), dim3(256), 0, (hipStream_t)stream, (const T*)dh, (const T*)u, (T*)du, n));
  return check_launch("alpro_gelu_bwd");
}

extern "C" int alpro_cls_mean_bwd(const float* dx_out, int64_t ld_batch, float* dside, int B, int T, int D, void* stream) {
  ALPRO_CHECK(dx_out && dside && B > 0 && T > 0 && D > 0, "alpro_cls_mean_bwd: bad args");
  hipLaunchKernelGGL(cls_mean_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, dx_out, ld_batch, dside, B, T, D);
  return check_launch("alpro_cls_mean_bwd");
}

extern "C" int alpro_scatter_add_rows_ordered(const float* src, const int64_t* idx, float* dst, int rows, int D, int64_t dst_rows, int64_t skip_idx, uint32_t* keys_ws,
                                              void* stream) {
  ALPRO_CHECK(src && idx && dst && keys_ws && rows > 0, "alpro_scatter_add_rows_ordered: bad args");
  ALPRO_CHECK(D == LN_D, "alpro_scatter_add_rows_ordered: D=%d unsupported", D);
  ALPRO_CHECK(rows <= SCATTER_SORT_MAX && dst_rows > 0 && dst_rows < (1 << 19), "alpro_scatter_add_rows_ordered: at most %d source rows and fewer than 2^19 table rows (got %d, %lld)",
              SCATTER_SORT_MAX, rows, (long long)dst_rows);
  hipLaunchKernelGGL(scatter_sort_keys_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, idx, rows, dst_rows, keys_ws);
  hipLaunchKernelGGL(scatter_add_runs_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, keys_ws, dst, rows, skip_idx);
  return check_launch("alpro_scatter_add_rows_ordered");
}

extern "C" int alpro_scatter_add_rows(const float* src, const int64_t* idx, float* dst, int rows, int idx_mod, int D, int64_t skip_idx, void* stream) {
  ALPRO_CHECK(src && dst && rows > 0 && (idx || idx_mod > 0), "alpro_scatter_add_rows: bad args");
  ALPRO_CHECK(D == LN_D, "alpro_scatter_add_rows: D=%d unsupported", D);
  if (!idx && skip_idx < 0) {  // destination = row % idx_mod: one wave per destination row, ascending order (bit-reproducible)
    hipLaunchKernelGGL(scatter_add_mod_kernel, dim3((idx_mod + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, dst, rows, idx_mod);
    return check_launch("alpro_scatter_add_rows");
  }
  hipLaunchKernelGGL(scatter_add_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, idx, dst, rows, idx_mod, skip_idx);
  return check_launch("alpro_scatter_add_rows");
}
