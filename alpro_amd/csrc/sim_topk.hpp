// What the two top-k searches share (sim_topk.hip: one feature row per gallery entry; sim_topk_clips.hip: several clips per video, pooled):
// the 64-bit candidate keys, the wave maximum, the staging of a query tile and the MFMA sub-tile of phase 1, the selection of a sub-pass,
// the merge kernel of phase 2 with its launch loop, and the plan (chunking, workspace levels).
//
// Order.  Every candidate is ONE 64-bit key: high word = the monotone map of the value's float bits (-0.0 canonicalised to +0.0 first),
// low word = the complement of the gallery index.  A larger key is a larger value or, on equal values, a smaller index: a total order on
// distinct candidates, so "the k largest keys, descending" is unique -- whatever the chunking, the grid or the order in which partial lists meet.
// Key 0 is "no candidate" (a valid key's low word is >= 2^31): it decodes to idx -1 / val -inf, the tail of a row when the gallery is shorter than k.
#pragma once
#include <limits.h>

#include "common.hpp"

namespace alpro {
namespace {

constexpr int TK_D = 256;            // embed_dim of the model (alpro_models.py:43)
constexpr int TK_QT = 32;            // query rows per workgroup
constexpr int TK_TILE = 512;         // gallery rows per sub-pass
constexpr int TK_TS = TK_TILE + 4;   // LDS tile row stride in words (rows stay 16-byte aligned)
constexpr int TK_P1_THREADS = 512;
constexpr int TK_QS_BYTES = TK_QT * TK_D * 4;
constexpr int TK_P1_LDS = TK_QS_BYTES + TK_QT * TK_TS * 4;   // 32768 + 66048 = 98816 bytes
constexpr int TK_LISTS_PER_THREAD = 8;
constexpr int TK_MERGE_G = 4 * 64 * TK_LISTS_PER_THREAD;     // lists one merge workgroup takes (2048)
constexpr int TK_MAX_LEVELS = 4;     // 2048^3 lists > 2^31 / 32 chunks: three merge levels always suffice

__device__ __forceinline__ uint32_t mono_key(float v) {
  uint32_t b = f2u(v);
  if (b == 0x80000000u) b = 0u;   // -0.0 -> +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mono_value(uint32_t m) { return u2f((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m); }
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// Maximum of a 64-bit key over the wave, the same value in every lane.  0 is the identity (keys are unsigned), so a DPP read that has no source
// lane simply contributes 0: four row_shr steps leave each 16-lane row's maximum in its last lane, row_bcast:15 carries it into rows 1 and 3,
// row_bcast:31 into the upper half, and lane 63 holds the wave's.  Six DPP steps instead of six LDS-crossbar shuffles per 32-bit half.
__device__ __forceinline__ uint64_t dpp_max_step(uint64_t v, uint32_t lo, uint32_t hi) { return max64(v, ((uint64_t)hi << 32) | lo); }
#define TK_DPP_MAX(v, ctrl, rows)                                                                                              \
  v = dpp_max_step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v), ctrl, rows, 0xf, false),                   \
                   (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((v) >> 32), ctrl, rows, 0xf, false))
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  TK_DPP_MAX(v, 0x111, 0xf);   // row_shr:1
  TK_DPP_MAX(v, 0x112, 0xf);   // row_shr:2
  TK_DPP_MAX(v, 0x114, 0xf);   // row_shr:4
  TK_DPP_MAX(v, 0x118, 0xf);   // row_shr:8
  TK_DPP_MAX(v, 0x142, 0xa);   // row_bcast:15 into rows 1 and 3
  TK_DPP_MAX(v, 0x143, 0xc);   // row_bcast:31 into rows 2 and 3
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

// The query tile of a workgroup into LDS in MFMA operand order, Qs[k >> 3][k & 1][row][(k >> 1) & 3]: one 16-byte read feeds four MFMA steps.
// Tile row r is query row q0 + r; rows past nq repeat the last query (their results are never written).
__device__ __forceinline__ void tk_stage_queries(float* Qs, const float* __restrict__ q, int64_t q0, int nq, int tid) {
#pragma unroll 4
  for (int it = 0; it < TK_QT * TK_D / TK_P1_THREADS; ++it) {
    const int idx = it * TK_P1_THREADS + tid, row = idx >> 8, k = idx & 255;
    const int64_t qr = min(q0 + row, (int64_t)nq - 1);
    Qs[(((k >> 3) * 2 + (k & 1)) * TK_QT + row) * 4 + ((k >> 1) & 3)] = q[(size_t)qr * TK_D + k];
  }
}

// One 32 (gallery) x 32 (query) tile with 128 v_mfma_f32_32x32x2_f32: gp is this lane's gallery row (row l31 of the sub-tile), lane half h
// supplies k = 2s + h at step s, so every element is the k-ordered fp32 fmaf chain from 0.  The gallery row comes straight from global memory:
// the two lanes of a row load alternate 16-byte pieces and one v_permlane32_swap per register pair sorts the k of parity h into lane half h
// (half the load instructions of "both lanes load everything and pick").
// Accumulator register r: gallery row (r & 3) + 8 (r >> 2) + 4 h of the sub-tile, query l31.
__device__ __forceinline__ f32x16 tk_subtile(const float* Qs, const f32x4* __restrict__ gp, int l31, int h) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < 32; c0 += 8) {
    f32x4 a[8];   // lane half h loads k = 8 i + 4 h .. + 3 of its row: the two halves of the wave split every 32 bytes between them
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = gp[(c0 + i) * 2 + h];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4 b = *(const f32x4*)&Qs[(((c0 + i) * 2 + h) * TK_QT + l31) * 4];
      // one half exchange per pair of registers puts k = 8 i + 2 j + h into lane half h, the operand order of step j:
      // (x | y) -> (k0 from the lower half, k1 moved up) and (k4 moved down, k5 from the upper half); (z | w) -> (k2, k3) and (k6, k7)
      const auto xy = __builtin_amdgcn_permlane32_swap(f2u(a[i].x), f2u(a[i].y), false, false);
      const auto zw = __builtin_amdgcn_permlane32_swap(f2u(a[i].z), f2u(a[i].w), false, false);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(xy[0]), b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(zw[0]), b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(xy[1]), b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(zw[1]), b.w, acc, 0, 0, 0);
    }
  }
  return acc;
}

// One sub-pass of selection for the first NV queries of a wave (NV of them run interleaved: the rounds are latency-bound).  rows: the wave's
// first tile row, value keys; a lane takes tile columns 8 lane .. 8 lane + 7 (candidate sub + column) and the entries of rank lane and
// lane + 64 of each running list.
template <int NV>
__device__ __forceinline__ void tk_select(const uint32_t* rows, int lane, int nvalid, int64_t sub, int kp, uint64_t (&run)[4][2]) {
  uint64_t key[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const uint32_t* row = rows + i * TK_TS + lane * 8;
    const u32x4 v0 = *(const u32x4*)row, v1 = *(const u32x4*)(row + 4);
    const uint32_t v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = lane * 8 + j;   // (columns past nvalid were never written: masked here)
      key[i][j] = col < nvalid ? (((uint64_t)v[j] << 32) | (uint32_t)~(uint32_t)(sub + col)) : 0ull;
    }
  }
  uint64_t nr[NV][2];
#pragma unroll
  for (int i = 0; i < NV; ++i) nr[i][0] = nr[i][1] = 0;
  for (int r = 0; r < kp; ++r) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      uint64_t local = max64(run[i][0], run[i][1]);
#pragma unroll
      for (int j = 0; j < 8; ++j) local = max64(local, key[i][j]);
      const uint64_t gm = wave_max_u64(local);
      // keys are distinct, so exactly one register of one lane holds gm (none when gm == 0: everything is taken)
#pragma unroll
      for (int j = 0; j < 8; ++j) key[i][j] = key[i][j] == gm ? 0ull : key[i][j];
      run[i][0] = run[i][0] == gm ? 0ull : run[i][0];
      run[i][1] = run[i][1] == gm ? 0ull : run[i][1];
      if (lane == (r & 63)) {
        if (r < 64) nr[i][0] = gm;
        else nr[i][1] = gm;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) { run[i][0] = nr[i][0]; run[i][1] = nr[i][1]; }
}

// tk_select for the first nv (0..4, wave-uniform) queries of a wave.  A macro: as a function that passes `run` on, the lists left the
// registers (40 bytes of scratch per lane in the compiler's report).
#define TK_SELECT_NV(nv, rows, lane, nvalid, sub, kp, run)                 \
  do {                                                                     \
    if ((nv) == 4) tk_select<4>(rows, lane, nvalid, sub, kp, run);         \
    else if ((nv) == 3) tk_select<3>(rows, lane, nvalid, sub, kp, run);    \
    else if ((nv) == 2) tk_select<2>(rows, lane, nvalid, sub, kp, run);    \
    else if ((nv) == 1) tk_select<1>(rows, lane, nvalid, sub, kp, run);    \
  } while (0)

// The running lists of a wave's first nv queries (lists list0 .. list0 + nv - 1) to the workspace: ws[list][chunk c][kp]
__device__ __forceinline__ void tk_write_lists(uint64_t* __restrict__ ws, int64_t list0, int nv, int nchunks, int c, int kp, int lane, const uint64_t (&run)[4][2]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < nv) {
      uint64_t* out = ws + ((size_t)(list0 + i) * nchunks + c) * kp;
      if (lane < kp) out[lane] = run[i][0];
      if (lane + 64 < kp) out[lane + 64] = run[i][1];
    }
  }
}

// in: (nq, nlists, len) sorted lists.  Workgroup (query, grp) merges lists [grp * NT * 8, ...) into k keys: out_keys (nq, ngroups, k), or -- the last
// level, ngroups == 1 and out_keys == nullptr -- the decoded out_val (= value * scale, one fp32 multiply) / out_idx (nq, k).
template <int NW>
__global__ __launch_bounds__(NW * 64) void sim_topk_merge_kernel(const uint64_t* __restrict__ in, int nlists, int len, int ngroups, int k,
                                                                 uint64_t* __restrict__ out_keys, float* __restrict__ out_val,
                                                                 int32_t* __restrict__ out_idx, float scale) {
  constexpr int NT = NW * 64;
  __shared__ uint64_t smax[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = blockIdx.x / ngroups, grp = blockIdx.x % ngroups;
  const int l0 = grp * (NT * TK_LISTS_PER_THREAD);
  const uint64_t* base = in + (size_t)qi * nlists * len;
  uint64_t head[TK_LISTS_PER_THREAD];
  int pos[TK_LISTS_PER_THREAD];
#pragma unroll
  for (int j = 0; j < TK_LISTS_PER_THREAD; ++j) {
    const int L = l0 + j * NT + tid;
    pos[j] = 0;
    head[j] = L < nlists ? base[(size_t)L * len] : 0ull;
  }
  for (int r = 0; r < k; ++r) {
    uint64_t local = head[0];
#pragma unroll
    for (int j = 1; j < TK_LISTS_PER_THREAD; ++j) local = max64(local, head[j]);
    uint64_t gm = wave_max_u64(local);
    if (NW > 1) {
      // one barrier per round: round r + 2 rewrites the slot of round r only after every thread has passed the barrier of round r + 1
      if (lane == 0) smax[r & 1][wave] = gm;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < NW; ++w) gm = max64(gm, smax[r & 1][w]);
    }
    if (tid == 0) {
      if (out_keys) {
        out_keys[((size_t)qi * ngroups + grp) * k + r] = gm;
      } else {
        out_val[(size_t)qi * k + r] = gm ? mono_value((uint32_t)(gm >> 32)) * scale : -INFINITY;
        out_idx[(size_t)qi * k + r] = gm ? (int32_t)~(uint32_t)gm : -1;
      }
    }
    if (gm != 0 && local == gm) {   // the one thread whose list gave the maximum moves that list on
#pragma unroll
      for (int j = 0; j < TK_LISTS_PER_THREAD; ++j) {
        if (head[j] == gm) {
          ++pos[j];
          head[j] = pos[j] < len ? base[(size_t)(l0 + j * NT + tid) * len + pos[j]] : 0ull;
        }
      }
    }
  }
}

struct TopkPlan {
  int chunk, nchunks, nqt, kp;
  int nlevels;                       // workspace levels: level 0 = phase 1's lists, level i > 0 = the output of merge pass i
  int lists[TK_MAX_LEVELS];          // lists per query at each level
  size_t off[TK_MAX_LEVELS], total;
};

inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }

// nq result lists over ng gallery entries, `per_tile` lists per phase-1 workgroup.  chunk 0 is the library's choice, a function of the shape
// alone: 512 entries, fewer (down to 128) while the grid would leave most of the chip idle.
// false (with the error text set) for arguments the kernels do not take.
inline bool topk_plan(const char* who, int nq, int ng, int k, int chunk, TopkPlan& p, int per_tile = TK_QT) {
  if (nq < 1) { set_error("%s: nq=%d queries (need >= 1)", who, nq); return false; }
  if (ng < 1) { set_error("%s: ng=%d gallery rows (need >= 1)", who, ng); return false; }
  if (k < 1 || k > ALPRO_TOPK_MAX_K) { set_error("%s: k=%d (need 1..%d = ALPRO_TOPK_MAX_K)", who, k, ALPRO_TOPK_MAX_K); return false; }
  if (chunk < 0 || chunk % 32 != 0) { set_error("%s: chunk=%d (0 = the library's choice, or a positive multiple of 32)", who, chunk); return false; }
  p.nqt = (int)(((int64_t)nq + per_tile - 1) / per_tile);
  if (chunk == 0) {
    chunk = TK_TILE;
    while (chunk > 128 &&(int64_t)p.nqt * (((int64_t)ng + chunk - 1) / chunk) < 256) chunk /= 2;
  }
  p.chunk = chunk;
  p.nchunks = (int)(((int64_t)ng + chunk - 1) / chunk);
  p.kp = k < chunk ? k : chunk;
  if ((int64_t)p.nqt * p.nchunks > INT_MAX || (int64_t)nq * ((p.nchunks + TK_MERGE_G - 1) / TK_MERGE_G) > INT_MAX) {
    set_error("%s: nq=%d x ng=%d with chunk=%d needs more than 2^31 - 1 workgroups", who, nq, ng, chunk);
    return false;
  }
  p.nlevels = 1;
  p.lists[0] = p.nchunks;
  p.off[0] = 0;
  p.total = round256((size_t)nq * p.nchunks * p.kp * sizeof(uint64_t));
  while (p.lists[p.nlevels - 1] > TK_MERGE_G) {
    p.lists[p.nlevels] = (p.lists[p.nlevels - 1] + TK_MERGE_G - 1) / TK_MERGE_G;
    p.off[p.nlevels] = p.total;
    p.total += round256((size_t)nq * p.lists[p.nlevels] * k * sizeof(uint64_t));
    ++p.nlevels;
  }
  return true;
}

// Phase 2: the merge passes over the workspace levels of the plan; the last one decodes to out_val / out_idx (nq, k).
inline int topk_merge(const char* what, const TopkPlan& p, int nq, int k, float scale, float* out_val, int32_t* out_idx, unsigned char* ws, hipStream_t st) {
  int len = p.kp;
  for (int lv = 0; lv < p.nlevels; ++lv) {
    const bool last = lv == p.nlevels - 1;
    const uint64_t* in = (const uint64_t*)(ws + p.off[lv]);
    uint64_t* out_keys = last ? nullptr : (uint64_t*)(ws + p.off[lv + 1]);
    const int nlists = p.lists[lv], ngroups = last ? 1 : p.lists[lv + 1];
    const dim3 grid((unsigned)(nq * ngroups));
    if (nlists <= 64 * TK_LISTS_PER_THREAD)   // (only ever the last level: one wave, no barrier)
      hipLaunchKernelGGL(sim_topk_merge_kernel<1>, grid, dim3(64), 0, st, in, nlists, len, ngroups, k, out_keys, out_val, out_idx, scale);
    else
      hipLaunchKernelGGL(sim_topk_merge_kernel<4>, grid, dim3(256), 0, st, in, nlists, len, ngroups, k, out_keys, out_val, out_idx, scale);
    const int rc = check_launch(what);
    if (rc) return rc;
    len = k;
  }
  return ALPRO_OK;
}

}  // namespace
}  // namespace alpro
