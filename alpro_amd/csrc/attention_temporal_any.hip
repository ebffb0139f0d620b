// Temporal attention over a frame count T that does NOT divide 32 (3 <= T <= ALPRO_ATTN_MAX_T, head_dim 64): the path alpro_attn_temporal_fwd /
// alpro_attn_temporal_bwd take when a frame group may cross a 32-row boundary.  T | 32 keeps the block-diagonal kernels of attention.hip /
// attention_bwd.hip, bit for bit.
//
// Unit = 32 consecutive rows r0 .. r0+31 x one head, as in those kernels; one wave per unit, four independent waves per workgroup, LDS
// wave-private, units handed out grid-stride.  The unit's rows touch the frame groups of the WINDOW
//     [floor(r0 / T) T, min(rows, ceil((r0 + 32) / T) T))      (at most 32 + 2 (T - 1) rows: <= 3 tiles of 32 below T = 32, <= 9 at T = 128)
// and a window row and a unit row see each other iff they share a group (absolute row / T).  The mask is symmetric, so one window serves
// both directions:
//   forward   lane = query of the unit; the window's keys in 32-row tiles (K fragments straight from global, V staged in LDS for the transposed
//             read), online softmax in the log2 domain.  lse ((rows + 31) / 32, H, 32), row c * 32 + r of head h at [c, h, r], as the divisor
//             kernels write it.
//   backward  one launch, two phases per unit, no atomics, no workspace (bitwise reproducible); every (row, head) of dqkv written once:
//             dQ     lane = query of the unit, over the window's keys:    dS^T = P^T o (dP^T - delta) * scale,  dQ^T += K^T dS^T
//             dK/dV  lane = key of the unit, over the window's queries:   dV^T += dO^T P,  dK^T += Q^T dS
//             P is recomputed from Q, K and lse; delta = rowsum(dO o O) -- from registers for the unit's queries, while staging for the window's.
// MFMA forms: 32x32x16 (bf16 / f16) and 32x32x2 f32, as in the other attention kernels.  LDS images are U tiles (attn_tile.hpp).
#include "common.hpp"
#include "attn_tile.hpp"

namespace alpro {
namespace {

template <typename T> struct TCfg : TileCfg<T> {
  static constexpr int NLD = 32 * TileCfg<T>::CPR / 64;  // chunks of one staged 32-row tile per lane
  static constexpr int IMG = 32 * TileCfg<T>::RB;        // bytes of one staged tile
};

// The wave's LDS traffic so far has completed, and the compiler moves no memory access across this point.  A wave's DS operations execute
// in order, so this is all the ordering a wave-private tile needs (write -> read and read -> next write).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// rows row0 .. row0+31 of one head's 64 columns (row stride ld elements) -> LDS tile; rows >= rend zero-filled
template <typename T> __device__ __forceinline__ void stage_tile(char* tile, const T* src, int64_t ld, int64_t row0, int64_t rend, int lane) {
  typedef TCfg<T> C;
  u32x4 v[C::NLD];
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int c = lane + 64 * i, row = c / C::CPR, ch = c - row * C::CPR;
    v[i] = row0 + row < rend ? *(const u32x4*)(src + (row0 + row) * ld + ch * C::CN) : mk4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int c = lane + 64 * i, row = c / C::CPR, ch = c - row * C::CPR;
    *(u32x4*)(tile + tile_off<T>(row, ch)) = v[i];
  }
}

// the unit's window: rows [w0, w1) (every frame group one of the unit's rows r0 .. rend-1 belongs to)
__device__ __forceinline__ void tattn_window(int64_t r0, int64_t rows, int Tn, int64_t& rend, int64_t& w0, int64_t& w1) {
  rend = min(rows, r0 + 32);
  w0 = r0 / Tn * Tn;
  w1 = min(rows, (rend + Tn - 1) / Tn * Tn);
}

// ================================================================================================
// forward: grid-stride over units = ceil(rows / 32) * H, 4 waves per workgroup
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 3 : 2) void tattn_any_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int64_t rows, int Tn, int H, float scale,
                                                            int64_t units, float* __restrict__ lse) {
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
      l = fmaf(l, alpha, ps);
      m = mn;
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
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void tattn_any_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                            const float* __restrict__ lse, T* __restrict__ dqkv, int64_t rows, int Tn, int H,
                                                            float scale, int64_t units) {
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
    const T* base = qkv + h * HD;
    const T* ob = out + h * HD;
    const T* dob = dout + h * HD;

    // ---- dQ: the unit's queries against the window's keys
    {
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
            s[r] = p;                                // P (feeds dV)
            dp[r] = p * (dp[r] - dd[e]) * scale;     // dS
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

int64_t tattn_grid(int64_t units) {
  const int64_t grid = (units + 3) / 4;
  return grid < 256 * 8 ? grid : 256 * 8;
}

template <typename T>
int launch_tattn_any_fwd(const void* qkv, void* out, int64_t rows, int Tn, int H, float scale, float* lse, hipStream_t st) {
  const size_t lds = 4 * (size_t)TCfg<T>::IMG;
  const int64_t units = ((rows + 31) / 32) * H;
  static DeviceOnce once;
  set_lds_once(once, tattn_any_fwd_kernel<T>, lds);
  hipLaunchKernelGGL((tattn_any_fwd_kernel<T>), dim3((unsigned)tattn_grid(units)), dim3(256), lds, st, (const T*)qkv, (T*)out, rows, Tn, H, scale, units, lse);
  return check_launch("alpro_attn_temporal_fwd (T not dividing 32)");
}

template <typename T>
int launch_tattn_any_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int64_t rows, int Tn, int H, float scale,
                         hipStream_t st) {
  const size_t lds = 4 * (2 * (size_t)TCfg<T>::IMG + 64 * sizeof(float));
  const int64_t units = ((rows + 31) / 32) * H;
  static DeviceOnce once;
  set_lds_once(once, tattn_any_bwd_kernel<T>, lds);
  hipLaunchKernelGGL((tattn_any_bwd_kernel<T>), dim3((unsigned)tattn_grid(units)), dim3(256), lds, st, (const T*)qkv, (const T*)out, (const T*)dout, lse,
                     (T*)dqkv, rows, Tn, H, scale, units);
  return check_launch("alpro_attn_temporal_bwd (T not dividing 32)");
}

}  // namespace

// entry points of alpro_attn_temporal_fwd / alpro_attn_temporal_bwd for 32 % T != 0, T <= ALPRO_ATTN_MAX_T (arguments checked by the callers)
int attn_temporal_any_fwd(const void* qkv, void* out, int dtype, int64_t rows, int T, int H, float scale, float* lse, hipStream_t st) {
  ALPRO_DISPATCH_DTYPE(dtype, T_, return launch_tattn_any_fwd<T_>(qkv, out, rows, T, H, scale, lse, st));
  return ALPRO_OK;
}
int attn_temporal_any_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int64_t rows, int T, int H,
                          float scale, hipStream_t st) {
  ALPRO_DISPATCH_DTYPE(dtype, T_, return launch_tattn_any_bwd<T_>(qkv, out, dout, lse, dqkv, rows, T, H, scale, st));
  return ALPRO_OK;
}

}  // namespace alpro
