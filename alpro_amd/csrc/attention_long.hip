// Full attention over L > 256 tokens (head_dim 64): the path alpro_attn_fwd / alpro_attn_bwd take above the whole-row kernels' 8 key tiles
// (attention.hip keeps every key of a (sequence, head) resident; these kernels stream them).  The MFMA formulation is the one of the
// whole-row kernels -- S^T = K Q^T with the query on the lane, P consumed from the accumulator registers as the B operand of O^T = V^T P^T --
// around a key-blocked loop:
//
//   forward   one workgroup = 4 waves = 4 x 32 queries of one (sequence, head); K / V blocks of 64 keys staged in LDS (two buffers, the next
//             block's global loads in flight under the current block's MFMAs); running max m and sum l per query row (online softmax, log2
//             domain).  With dropout, l sums the UN-dropped p while O accumulates the dropped, rescaled p (the normaliser is the softmax's).
//             lse (batch, H, L) in the layout of the whole-row kernels.  The precise [CLS] query (cls_q) is a companion launch,
//             attn_long_cls_kernel: the fp32 q row against the 16-bit K / V of every key, key 0 included (only the q third of cls_q is read).
//   backward  two kernels, no atomics, no workspace (bitwise reproducible):
//             dQ   one workgroup per 4 query tiles, sweeping K / V blocks:   dS^T = P^T o (dP^T - delta) * scale, dQ^T += K^T dS^T
//             dK/dV one workgroup per 4 key tiles, sweeping Q / dO blocks:   dV^T += dO^T P,  dK^T += Q^T dS
//             P is recomputed from Q, K and lse; delta = rowsum(dO o O) is formed on the fly (per query tile in the dQ kernel, per staged query
//             block in the dK/dV kernel) -- O already carries the dropout mask, so the identity holds with dropout too.
// LDS images are U tiles (attn_tile.hpp): one swizzle for row reads (ds_read_b128) and transposed reads (ds_read_b64_tr_b16).
#include "common.hpp"
#include "attn_tile.hpp"

namespace alpro {
namespace {

constexpr int NW = 4;     // waves per workgroup = 32-row tiles owned per workgroup
constexpr int KB = 64;    // rows per staged block (two 32-row tiles)

template <typename T> struct LCfg : TileCfg<T> {
  static constexpr int NLD = KB * TileCfg<T>::CPR / 256;  // chunks of one staged matrix per thread
  static constexpr int IMG = KB * TileCfg<T>::RB;         // bytes of one staged matrix
};

// (unit = sequence * H + head, group of NW tiles) of this workgroup.  Workgroups go to the 8 XCDs round-robin; when the grid is a multiple of 8,
// XCD x gets the contiguous id range [x, x+1) * grid/8, so the groups of one (sequence, head) -- which read the same K / V (Q / dO) blocks --
// share an L2.
__device__ __forceinline__ void long_unit(int ngrp, int& unit, int& grp) {
  const int nb = gridDim.x;
  int id = blockIdx.x;
  if ((nb & 7) == 0) id = (id & 7) * (nb >> 3) + (id >> 3);
  unit = id / ngrp;
  grp = id - unit * ngrp;
}

// One staged block of two matrices (rows r0 .. r0+63 of a sequence; rows >= L zero-filled, never read): global loads into registers first
// (fetch, issued before the current block's MFMAs), LDS writes after them (put).
template <typename T> struct BlockPair {
  typedef LCfg<T> C;
  u32x4 a[C::NLD], b[C::NLD];
  __device__ __forceinline__ void fetch(const T* sa, int64_t lda, const T* sb, int64_t ldb, int r0, int L, int tid) {
#pragma unroll
    for (int i = 0; i < C::NLD; ++i) {
      const int c = tid + 256 * i, row = c / C::CPR, ch = c - row * C::CPR;
      a[i] = b[i] = mk4(0u, 0u, 0u, 0u);
      if (r0 + row < L) {
        a[i] = *(const u32x4*)(sa + (int64_t)(r0 + row) * lda + ch * C::CN);
        b[i] = *(const u32x4*)(sb + (int64_t)(r0 + row) * ldb + ch * C::CN);
      }
    }
  }
  __device__ __forceinline__ void put(char* ia, char* ib, int tid) const {
#pragma unroll
    for (int i = 0; i < C::NLD; ++i) {
      const int c = tid + 256 * i, row = c / C::CPR, ch = c - row * C::CPR;
      *(u32x4*)(ia + tile_off<T>(row, ch)) = a[i];
      *(u32x4*)(ib + tile_off<T>(row, ch)) = b[i];
    }
  }
};

// ================================================================================================
// forward: grid = batch * H * ceil(L / 128) workgroups of 256 threads
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int L, int H, float scale,
                                                            const float* __restrict__ key_bias, float* __restrict__ lse, float drop_p,
                                                            uint32_t drop_seed, int nqg) {
  typedef LCfg<T> C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Bs = (float*)(smem + 4 * C::IMG);  // [2][KB] key bias * log2(e); -inf past L
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int unit, qg;
  long_unit(nqg, unit, qg);
  const int b = unit / H, h = unit - b * H;
  const int64_t ldq = 3 * (int64_t)H * HD;
  const T* base = qkv + (int64_t)b * L * ldq + h * HD;
  const float* kbias = key_bias ? key_bias + (int64_t)b * L : nullptr;
  const int g = lane >> 5, ql = lane & 31;
  const int qt0 = (qg * NW + wave) * 32;
  const bool active = qt0 < L;   // wave-uniform: this wave owns a query tile
  const int q = qt0 + ql, qc = min(q, L - 1);
  const float sl = scale * LOG2E;
  u32x4 qf[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) qf[ks] = *(const u32x4*)(base + (int64_t)qc * ldq + (2 * ks + g) * C::CN);
  const uint32_t th = drop_thresh24(drop_p);
  const float dks = DROP ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t drow = ((((uint64_t)b * H + h) * L) + (uint64_t)qc) * (uint64_t)L;

  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int nkb = (L + KB - 1) / KB;
  BlockPair<T> st;
  float bnext = 0.f;
  auto fetch = [&](int kb) __attribute__((always_inline)) {
    st.fetch(base + H * HD, ldq, base + 2 * H * HD, ldq, kb * KB, L, tid);
    if (tid < KB) {
      const int key = kb * KB + tid;
      bnext = key < L ? (kbias ? kbias[key] * LOG2E : 0.f) : -INFINITY;
    }
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
    char* Ks = smem + buf * 2 * C::IMG;
    st.put(Ks, Ks + C::IMG, tid);
    if (tid < KB) Bs[buf * KB + tid] = bnext;
  };
  fetch(0);
  put(0);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    if (kb + 1 < nkb) fetch(kb + 1);
    if (active) {
      const char* Ks = smem + cur * 2 * C::IMG;
      const char* Vs = Ks + C::IMG;
      const float* Bb = Bs + cur * KB;
      const int nt = min(2, (L - kb * KB + 31) >> 5);   // key tiles of this block holding a key < L
      f32x16 s[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt < nt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
          const int krow = kt * 32 + ql;
#pragma unroll
          for (int ks = 0; ks < C::KS; ++ks) mma_chunk<T>(s[kt], *(const u32x4*)(Ks + tile_off<T>(krow, 2 * ks + g)), qf[ks]);
        }
      }
      float mb = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt < nt) {
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const float4 bq = *(const float4*)(Bb + kt * 32 + 8 * rq + 4 * g);
            const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = fmaf(s[kt][4 * rq + e], sl, bb[e]);
              s[kt][4 * rq + e] = v;
              mb = fmaxf(mb, v);
            }
          }
        }
      }
      mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
      const float mn = fmaxf(m, mb);                        // finite: every block holds a key < L, and key bias is finite
      const float alpha = __builtin_amdgcn_exp2f(m - mn);   // exp2(-inf) == 0 on the first block
      float ps = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt < nt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float p = __builtin_amdgcn_exp2f(s[kt][r] - mn);   // exp2(-inf) == 0 for keys past L
            ps += p;
            if (DROP) p = drop_keep(drop_seed, drow + (uint64_t)(kb * KB + kt * 32 + acc_row(r, lane)), th) ? p * dks : 0.f;
            s[kt][r] = p;
          }
        }
      }
      ps += __shfl_xor(ps, 32, 64);
      l = fmaf(l, alpha, ps);
      m = mn;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt < nt) {
#pragma unroll
          for (int cc = 0; cc < C::CPT; ++cc) {
            float pv[C::CN];
#pragma unroll
            for (int e = 0; e < C::CN; ++e) pv[e] = s[kt][cc * C::CN + e];
            const u32x4 bop = pack_chunk<T>(pv);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(o[dt], load_t_chunk<T>(Vs, kt * 32, cc, lane, dt), bop);
          }
        }
      }
    }
    if (kb + 1 < nkb) put(cur ^ 1);
    __syncthreads();
  }
  if (active && q < L) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= inv;
    store_row64<T>(out + ((int64_t)b * L + q) * H * HD + h * HD, o, lane);
    if (lse && g == 0) lse[((int64_t)b * H + h) * L + q] = (m + __log2f(l)) * LN2;
  }
}

// ================================================================================================
// precise [CLS] query: out[s, h*64:(h+1)*64] = softmax(q_cls K^T * scale + key_bias) V in fp32, q_cls = the q third of cls_q row s / group
// (UNROUNDED), K / V of EVERY key -- key 0 included -- from the 16-bit qkv tensor; dropout under the mask the forward draws for query 0.
// One wave per (sequence, head): lane = (key slot g = lane >> 3, 8-element head chunk e = lane & 7); the 8 key slots keep independent online
// softmax states merged once at the end.  grid = ceil(batch * H / 4) workgroups of 256 threads.
template <typename T>
__global__ __launch_bounds__(256) void attn_long_cls_kernel(const T* __restrict__ qkv, const float* __restrict__ cls_q, const float* __restrict__ key_bias,
                                                            float* __restrict__ out, int batch, int L, int H, int group, float scale, float drop_p,
                                                            uint32_t drop_seed) {
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= batch * H) return;
  const int s = unit / H, h = unit - s * H;
  const int g = lane >> 3, e = lane & 7;
  const int64_t ldq = 3 * (int64_t)H * HD;
  float q[8];
  {
    const float* cq = cls_q + (int64_t)(s / group) * ldq + h * HD + e * 8;
    const float sl = scale * LOG2E;
    const float4 a = *(const float4*)cq, c = *(const float4*)(cq + 4);
    q[0] = a.x * sl; q[1] = a.y * sl; q[2] = a.z * sl; q[3] = a.w * sl; q[4] = c.x * sl; q[5] = c.y * sl; q[6] = c.z * sl; q[7] = c.w * sl;
  }
  const T* base = qkv + (int64_t)s * L * ldq + h * HD + e * 8;
  const float* kb = key_bias ? key_bias + (int64_t)s * L : nullptr;
  const uint32_t th = drop_thresh24(drop_p);
  const float ks = drop_seed ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t drop_base = (((uint64_t)s * H + h) * L) * (uint64_t)L;   // query 0 of (s, h)
  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  const int nit = (L + 7) >> 3;
  for (int it = 0; it < nit; ++it) {
    const int j = it * 8 + g;
    const bool live = j < L;   // (uniform over the 8 lanes of a key slot)
    const int jc = live ? j : L - 1;
    float kf[8], vf[8];
    unpack_chunk<T>(*(const u32x4*)(base + (int64_t)jc * ldq + H * HD), kf);
    unpack_chunk<T>(*(const u32x4*)(base + (int64_t)jc * ldq + 2 * H * HD), vf);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    if (live) {
      if (kb) d = fmaf(kb[j], LOG2E, d);
      const float mn = fmaxf(m, d);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);   // exp2(-inf) == 0 on the first key of the slot
      const float p = __builtin_amdgcn_exp2f(d - mn);
      l = fmaf(l, alpha, p);
      float pd = p;
      if (drop_seed) pd = drop_keep(drop_seed, drop_base + (uint64_t)j, th) ? p * ks : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(acc[i], alpha, pd * vf[i]);
      m = mn;
    }
  }
  // merge the 8 key slots (lanes with equal e): global maximum, rescale, sum
  float M = m;
  M = fmaxf(M, __shfl_xor(M, 8, 64));
  M = fmaxf(M, __shfl_xor(M, 16, 64));
  M = fmaxf(M, __shfl_xor(M, 32, 64));
  const float w = __builtin_amdgcn_exp2f(m - M);
  l *= w;
  l += __shfl_xor(l, 8, 64);
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float a = acc[i] * w;
    a += __shfl_xor(a, 8, 64);
    a += __shfl_xor(a, 16, 64);
    a += __shfl_xor(a, 32, 64);
    acc[i] = a * inv;
  }
  if (g == 0) {
    float* o = out + (int64_t)s * H * HD + h * HD + e * 8;
    *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *(float4*)(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

// ================================================================================================
// backward, dQ: grid = batch * H * ceil(L / 128); a wave owns 32 queries (lane = query) and sweeps the K / V blocks
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void attn_long_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                           const float* __restrict__ lse, T* __restrict__ dqkv, int L, int H, float scale,
                                                           const float* __restrict__ key_bias, float drop_p, uint32_t drop_seed, int nqg) {
  typedef LCfg<T> C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Bs = (float*)(smem + 4 * C::IMG);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int unit, qg;
  long_unit(nqg, unit, qg);
  const int b = unit / H, h = unit - b * H;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const T* base = qkv + (int64_t)b * L * ldq + h * HD;
  const T* ob = out + (int64_t)b * L * ldo + h * HD;
  const T* dob = dout + (int64_t)b * L * ldo + h * HD;
  const float* kbias = key_bias ? key_bias + (int64_t)b * L : nullptr;
  const int g = lane >> 5, ql = lane & 31;
  const int qt0 = (qg * NW + wave) * 32;
  const bool active = qt0 < L;
  const int q = qt0 + ql, qc = min(q, L - 1);
  const float sl = scale * LOG2E;
  u32x4 qf[C::KS], dof[C::KS];
  float delta = 0.f;
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    const int off = (2 * ks + g) * C::CN;
    qf[ks] = *(const u32x4*)(base + (int64_t)qc * ldq + off);
    dof[ks] = *(const u32x4*)(dob + (int64_t)qc * ldo + off);
    float a[C::CN], c2[C::CN];
    unpack_chunk<T>(dof[ks], a);
    unpack_chunk<T>(*(const u32x4*)(ob + (int64_t)qc * ldo + off), c2);
#pragma unroll
    for (int e = 0; e < C::CN; ++e) delta = fmaf(a[e], c2[e], delta);
  }
  delta += __shfl_xor(delta, 32, 64);
  const float lq = lse[((int64_t)b * H + h) * L + qc] * LOG2E;
  const uint32_t th = drop_thresh24(drop_p);
  const float dks = DROP ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t drow = ((((uint64_t)b * H + h) * L) + (uint64_t)qc) * (uint64_t)L;
  f32x16 dq[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;

  const int nkb = (L + KB - 1) / KB;
  BlockPair<T> st;
  float bnext = 0.f;
  auto fetch = [&](int kb) __attribute__((always_inline)) {
    st.fetch(base + H * HD, ldq, base + 2 * H * HD, ldq, kb * KB, L, tid);
    if (tid < KB) {
      const int key = kb * KB + tid;
      bnext = key < L ? (kbias ? kbias[key] * LOG2E : 0.f) : -INFINITY;
    }
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
    char* Ks = smem + buf * 2 * C::IMG;
    st.put(Ks, Ks + C::IMG, tid);
    if (tid < KB) Bs[buf * KB + tid] = bnext;
  };
  fetch(0);
  put(0);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    if (kb + 1 < nkb) fetch(kb + 1);
    if (active) {
      const char* Ks = smem + cur * 2 * C::IMG;
      const char* Vs = Ks + C::IMG;
      const float* Bb = Bs + cur * KB;
      const int nt = min(2, (L - kb * KB + 31) >> 5);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt < nt) {
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
          const int krow = kt * 32 + ql;
#pragma unroll
          for (int ks = 0; ks < C::KS; ++ks) {
            mma_chunk<T>(s, *(const u32x4*)(Ks + tile_off<T>(krow, 2 * ks + g)), qf[ks]);
            mma_chunk<T>(dp, *(const u32x4*)(Vs + tile_off<T>(krow, 2 * ks + g)), dof[ks]);
          }
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const float4 bq = *(const float4*)(Bb + kt * 32 + 8 * rq + 4 * g);
            const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 4 * rq + e;
              const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sl, bb[e]) - lq);
              float gd = dp[r];
              if (DROP) gd = drop_keep(drop_seed, drow + (uint64_t)(kb * KB + kt * 32 + 8 * rq + 4 * g + e), th) ? gd * dks : 0.f;
              s[r] = p * (gd - delta) * scale;   // dS^T
            }
          }
#pragma unroll
          for (int cc = 0; cc < C::CPT; ++cc) {
            float v[C::CN];
#pragma unroll
            for (int e = 0; e < C::CN; ++e) v[e] = s[cc * C::CN + e];
            const u32x4 bop = pack_chunk<T>(v);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) mma_chunk<T>(dq[dt], load_t_chunk<T>(Ks, kt * 32, cc, lane, dt), bop);
          }
        }
      }
    }
    if (kb + 1 < nkb) put(cur ^ 1);
    __syncthreads();
  }
  if (active && q < L) store_row64<T>(dqkv + ((int64_t)b * L + q) * ldq + h * HD, dq, lane);
}

// ================================================================================================
// backward, dK / dV: grid = batch * H * ceil(L / 128); a wave owns 32 keys (lane = key) and sweeps the Q / dO blocks.  delta of a staged query
// block is formed while it is staged: the CPR consecutive threads that load one row's chunks also load its O chunks and add up their products.
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void attn_long_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                            const float* __restrict__ lse, T* __restrict__ dqkv, int L, int H, float scale,
                                                            const float* __restrict__ key_bias, float drop_p, uint32_t drop_seed, int nkg) {
  typedef LCfg<T> C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ls = (float*)(smem + 4 * C::IMG);  // [2][KB] lse * log2(e); +inf past L
  float* Ds = Ls + 2 * KB;                  // [2][KB] delta; 0 past L
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int unit, kg;
  long_unit(nkg, unit, kg);
  const int b = unit / H, h = unit - b * H;
  const int64_t ldq = 3 * (int64_t)H * HD, ldo = (int64_t)H * HD;
  const T* base = qkv + (int64_t)b * L * ldq + h * HD;
  const T* ob = out + (int64_t)b * L * ldo + h * HD;
  const T* dob = dout + (int64_t)b * L * ldo + h * HD;
  const float* lse_b = lse + ((int64_t)b * H + h) * L;
  const int g = lane >> 5, ql = lane & 31;
  const int kt0 = (kg * NW + wave) * 32;
  const bool active = kt0 < L;
  const int key = kt0 + ql, kc = min(key, L - 1);
  const float sl = scale * LOG2E;
  u32x4 kf[C::KS], vf[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    const int off = (2 * ks + g) * C::CN;
    kf[ks] = *(const u32x4*)(base + (int64_t)kc * ldq + H * HD + off);
    vf[ks] = *(const u32x4*)(base + (int64_t)kc * ldq + 2 * H * HD + off);
  }
  const float kbv = key < L ? (key_bias ? key_bias[(int64_t)b * L + key] * LOG2E : 0.f) : -INFINITY;
  const uint32_t th = drop_thresh24(drop_p);
  const float dks = DROP ? 1.0f / (1.0f - drop_p) : 1.0f;
  const uint64_t dbase = ((uint64_t)b * H + h) * (uint64_t)L;   // + q, then * L + key
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;

  const int nqb = (L + KB - 1) / KB;
  BlockPair<T> st;
  u32x4 oc[C::NLD];
  float lnext = 0.f;
  auto fetch = [&](int qb) __attribute__((always_inline)) {
    st.fetch(base, ldq, dob, ldo, qb * KB, L, tid);
#pragma unroll
    for (int i = 0; i < C::NLD; ++i) {
      const int c = tid + 256 * i, row = c / C::CPR, ch = c - row * C::CPR;
      oc[i] = qb * KB + row < L ? *(const u32x4*)(ob + (int64_t)(qb * KB + row) * ldo + ch * C::CN) : mk4(0u, 0u, 0u, 0u);
    }
    if (tid < KB) {
      const int qq = qb * KB + tid;
      lnext = qq < L ? lse_b[qq] * LOG2E : INFINITY;
    }
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
    char* Qs = smem + buf * 2 * C::IMG;
    st.put(Qs, Qs + C::IMG, tid);
#pragma unroll
    for (int i = 0; i < C::NLD; ++i) {   // delta of row (tid + 256 i) / CPR: its CPR chunks sit in CPR consecutive lanes
      float a[C::CN], c2[C::CN];
      unpack_chunk<T>(st.b[i], a);
      unpack_chunk<T>(oc[i], c2);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < C::CN; ++e) d = fmaf(a[e], c2[e], d);
#pragma unroll
      for (int o = C::CPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      const int c = tid + 256 * i;
      if (c % C::CPR == 0) Ds[buf * KB + c / C::CPR] = d;   // rows past L: zero-filled chunks -> 0
    }
    if (tid < KB) Ls[buf * KB + tid] = lnext;
  };
  fetch(0);
  put(0);
  __syncthreads();
  for (int qb = 0; qb < nqb; ++qb) {
    const int cur = qb & 1;
    if (qb + 1 < nqb) fetch(qb + 1);
    if (active) {
      const char* Qs = smem + cur * 2 * C::IMG;
      const char* Os = Qs + C::IMG;   // dO
      const float* Lb = Ls + cur * KB;
      const float* Db = Ds + cur * KB;
      const int nt = min(2, (L - qb * KB + 31) >> 5);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        if (qt < nt) {
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
          const int qrow = qt * 32 + ql;
#pragma unroll
          for (int ks = 0; ks < C::KS; ++ks) {
            mma_chunk<T>(s, *(const u32x4*)(Qs + tile_off<T>(qrow, 2 * ks + g)), kf[ks]);
            mma_chunk<T>(dp, *(const u32x4*)(Os + tile_off<T>(qrow, 2 * ks + g)), vf[ks]);
          }
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const float4 lq4 = *(const float4*)(Lb + qt * 32 + 8 * rq + 4 * g);
            const float4 dd4 = *(const float4*)(Db + qt * 32 + 8 * rq + 4 * g);
            const float ll[4] = {lq4.x, lq4.y, lq4.z, lq4.w}, dd[4] = {dd4.x, dd4.y, dd4.z, dd4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 4 * rq + e;
              const float p = __builtin_amdgcn_exp2f(fmaf(s[r], sl, kbv) - ll[e]);   // 0 for queries (+inf) or keys (-inf) past L
              float dm = 1.0f;
              if (DROP) {
                const int qq = min(qb * KB + qt * 32 + 8 * rq + 4 * g + e, L - 1);
                dm = drop_keep(drop_seed, (dbase + (uint64_t)qq) * L + (uint64_t)kc, th) ? dks : 0.f;
              }
              s[r] = p * dm;                              // dropped P (feeds dV)
              dp[r] = p * (dm * dp[r] - dd[e]) * scale;   // dS
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
              mma_chunk<T>(dv[dt], load_t_chunk<T>(Os, qt * 32, cc, lane, dt), pb);
              mma_chunk<T>(dk[dt], load_t_chunk<T>(Qs, qt * 32, cc, lane, dt), sb);
            }
          }
        }
      }
    }
    if (qb + 1 < nqb) put(cur ^ 1);
    __syncthreads();
  }
  if (active && key < L) {
    store_row64<T>(dqkv + ((int64_t)b * L + key) * ldq + H * HD + h * HD, dk, lane);
    store_row64<T>(dqkv + ((int64_t)b * L + key) * ldq + 2 * H * HD + h * HD, dv, lane);
  }
}

template <typename T>
int launch_long_fwd(const void* qkv, void* out, int batch, int L, int H, float scale, const float* key_bias, float* lse, float dp, uint32_t ds,
                    const float* cls_q, int cls_group, float* cls_out, hipStream_t st) {
  typedef LCfg<T> C;
  const size_t lds = 4 * (size_t)C::IMG + 2 * KB * sizeof(float);
  const int nqg = (L + NW * 32 - 1) / (NW * 32);
  const dim3 grid((unsigned)(batch * H * nqg));
  if (ds) {
    static DeviceOnce once;
    set_lds_once(once, attn_long_fwd_kernel<T, true>, lds);
    hipLaunchKernelGGL((attn_long_fwd_kernel<T, true>), grid, dim3(256), lds, st, (const T*)qkv, (T*)out, L, H, scale, key_bias, lse, dp, ds, nqg);
  } else {
    static DeviceOnce once;
    set_lds_once(once, attn_long_fwd_kernel<T, false>, lds);
    hipLaunchKernelGGL((attn_long_fwd_kernel<T, false>), grid, dim3(256), lds, st, (const T*)qkv, (T*)out, L, H, scale, key_bias, lse, 0.f, 0u, nqg);
  }
  const int rc = check_launch("alpro_attn_fwd (L > 256)");
  if constexpr (sizeof(T) == 2) {   // (the precise CLS query is a 16-bit-mode side path: alpro_attn_fwd refuses cls_q with fp32 operands)
    if (rc != ALPRO_OK || !cls_q) return rc;
    hipLaunchKernelGGL((attn_long_cls_kernel<T>), dim3((unsigned)((batch * H + 3) / 4)), dim3(256), 0, st, (const T*)qkv, cls_q, key_bias, cls_out,
                       batch, L, H, cls_group, scale, dp, ds);
    return check_launch("alpro_attn_fwd (L > 256, CLS query)");
  }
  return rc;
}

template <typename T>
int launch_long_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int batch, int L, int H, float scale,
                    const float* key_bias, float dp, uint32_t ds, hipStream_t st) {
  typedef LCfg<T> C;
  const size_t lds_q = 4 * (size_t)C::IMG + 2 * KB * sizeof(float);
  const size_t lds_k = 4 * (size_t)C::IMG + 4 * KB * sizeof(float);
  const int ng = (L + NW * 32 - 1) / (NW * 32);
  const dim3 grid((unsigned)(batch * H * ng));
#define ALPRO_LONG_BWD(DROP_)                                                                                                                   \
  {                                                                                                                                             \
    static DeviceOnce once_q, once_k;                                                                                                           \
    set_lds_once(once_q, attn_long_dq_kernel<T, DROP_>, lds_q);                                                                                 \
    set_lds_once(once_k, attn_long_dkv_kernel<T, DROP_>, lds_k);                                                                                \
    hipLaunchKernelGGL((attn_long_dq_kernel<T, DROP_>), grid, dim3(256), lds_q, st, (const T*)qkv, (const T*)out, (const T*)dout, lse, (T*)dqkv, \
                       L, H, scale, key_bias, dp, ds, ng);                                                                                      \
    const int rc = check_launch("alpro_attn_bwd (L > 256, dQ)");                                                                                \
    if (rc != ALPRO_OK) return rc;                                                                                                              \
    hipLaunchKernelGGL((attn_long_dkv_kernel<T, DROP_>), grid, dim3(256), lds_k, st, (const T*)qkv, (const T*)out, (const T*)dout, lse,        \
                       (T*)dqkv, L, H, scale, key_bias, dp, ds, ng);                                                                            \
  }
  if (ds) ALPRO_LONG_BWD(true) else ALPRO_LONG_BWD(false)
#undef ALPRO_LONG_BWD
  return check_launch("alpro_attn_bwd (L > 256, dK / dV)");
}

}  // namespace

// entry points of alpro_attn_fwd / alpro_attn_bwd for 256 < L <= ALPRO_ATTN_MAX_L (arguments checked by the callers)
int attn_long_fwd(const void* qkv, void* out, int dtype, int batch, int L, int H, float scale, const float* key_bias, float* lse, float drop_p,
                  uint32_t drop_seed, const float* cls_q, int cls_group, float* cls_out, hipStream_t st) {
  ALPRO_DISPATCH_DTYPE(dtype, T, return launch_long_fwd<T>(qkv, out, batch, L, H, scale, key_bias, lse, drop_p, drop_seed, cls_q, cls_group, cls_out, st));
  return ALPRO_OK;
}
int attn_long_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int batch, int L, int H, float scale,
                  const float* key_bias, float drop_p, uint32_t drop_seed, hipStream_t st) {
  ALPRO_DISPATCH_DTYPE(dtype, T, return launch_long_bwd<T>(qkv, out, dout, lse, dqkv, batch, L, H, scale, key_bias, drop_p, drop_seed, st));
  return ALPRO_OK;
}

}  // namespace alpro
