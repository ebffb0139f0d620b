// Top-k by POOLED similarity without the matrix (stage 1 of rerank_retrieval with inference_n_clips > 1): a video is n clips, rows v n + j of
// its feature matrix; the value of a (video, caption) pair is P = pool_j (s_j * scale), s_j the clip's fp32 fmaf chain (tk_subtile, the chain
// of alpro_sim_topk), pooled by mean / max / lse with the arithmetic of alpro_clip_pool (clip_pool.hpp).  Either side may carry the clips:
//   GALLERY (text -> video): g is (nvid n, 256); the candidates of a query row are the videos.
//   QUERY   (video -> text): q is (nvid n, 256); a result list belongs to a video, the candidates are the rows of g.
// Order, keys, selection, merge and plan are sim_topk.hpp's; `chunk` and every candidate index count gallery ENTRIES (videos / rows).
//
// Phase 1 (sim_topk_clips_partial_kernel): sim_topk_partial_kernel with one more step.  The MFMA sub-tiles store x = s * scale as fp32 into the
// LDS tile [query row][gallery row of the sub-pass]; a pooling pass then turns it IN PLACE into the value keys [list][entry] that tk_select reads:
//   GALLERY: a sub-pass holds floor(512 / n) whole videos, so the n clips of entry e are the tile columns e n .. e n + n - 1 (n need not divide
//            the 32-row MFMA sub-tile: pooling happens after the tile is in LDS).  Wave w pools the rows of its own queries 4w .. 4w+3, 64 entries
//            at a time: every lane reads its n columns, then -- behind a barrier -- writes column e <= e n.  Batches after the first read
//            columns >= 64 (b + 1), past everything written so far.
//   QUERY:   a query tile holds floor(32 / n) whole videos, tile rows v n .. v n + n - 1.  Thread t owns column t and walks the videos in
//            ascending order: video v reads rows v n .. and writes row v <= v n of the same column, which no later video reads.
// The merge decodes with scale 1 (P * 1.0f = P, -0.0 already canonicalised by the key).  No atomics; one writer per output element.
#include "clip_pool.hpp"
#include "sim_topk.hpp"

namespace alpro {
namespace {

template <class Load>
__device__ __forceinline__ float pool_any(int mode, int n, Load x) {
  if (mode == ALPRO_POOL_MEAN) return clip_pool_value<ALPRO_POOL_MEAN>(n, x);
  if (mode == ALPRO_POOL_MAX) return clip_pool_value<ALPRO_POOL_MAX>(n, x);
  return clip_pool_value<ALPRO_POOL_LSE>(n, x);
}

// nlists result lists (SIDE GALLERY: the nq query rows; QUERY: nq / n videos), nent gallery entries (GALLERY: ng / n videos; QUERY: ng rows)
template <int SIDE>
__global__ __launch_bounds__(TK_P1_THREADS) void sim_topk_clips_partial_kernel(const float* __restrict__ q, int nq, const float* __restrict__ g, int ng,
                                                                               int n, int mode, float scale, int chunk, int nchunks, int nqt, int kp,
                                                                               uint64_t* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  float* Qs = (float*)tk_smem;                            // the tile's 32 query rows in MFMA operand order (tk_stage_queries)
  uint32_t* tile = (uint32_t*)(tk_smem + TK_QS_BYTES);    // [query row][gallery row of the sub-pass] x as fp32, pooled in place to [list][entry] keys
  const float* xt = (const float*)tile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % nqt, c = blockIdx.x / nqt;
  constexpr bool GAL = SIDE == ALPRO_TOPK_CLIPS_GALLERY;
  const int per_tile = GAL ? TK_QT : TK_QT / n;           // result lists of a query tile
  const int nlists = GAL ? nq : nq / n, nent = GAL ? ng / n : ng;
  const int rows_per_ent = GAL ? n : 1;                   // rows of g per gallery entry
  const int ent_per_sub = GAL ? TK_TILE / n : TK_TILE;    // gallery entries per sub-pass
  const int64_t list0 = (int64_t)qt * per_tile;
  tk_stage_queries(Qs, q, GAL ? list0 : list0 * n, nq, tid);
  __syncthreads();
  const int64_t c_begin = (int64_t)c * chunk;
  const int64_t c_end = min((int64_t)nent, c_begin + chunk);
  const int tile_lists = (int)min((int64_t)per_tile, nlists - list0);   // the real lists of this tile (>= 1)
  const int nv = min(4, max(0, tile_lists - wave * 4));                 // wave-uniform: the real lists among this wave's four
  uint64_t run[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) run[i][0] = run[i][1] = 0;

  for (int64_t sub = c_begin; sub < c_end; sub += ent_per_sub) {
    const int nvalid = (int)min((int64_t)ent_per_sub, c_end - sub);   // entries of this sub-pass
    const int nrows = nvalid * rows_per_ent;                          // <= 512 rows of g
    const int nst = (nrows + 31) >> 5;
    for (int st = wave; st < nst; st += TK_P1_THREADS / 64) {
      const int64_t grow = min(sub * rows_per_ent + st * 32 + l31, (int64_t)ng - 1);   // rows past ng repeat the last row; never pooled
      const f32x16 acc = tk_subtile(Qs, (const f32x4*)(g + (size_t)grow * TK_D), l31, h);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *(u32x4*)&tile[l31 * TK_TS + st * 32 + 8 * g4 + 4 * h] =
            mk4(f2u(acc[4 * g4] * scale), f2u(acc[4 * g4 + 1] * scale), f2u(acc[4 * g4 + 2] * scale), f2u(acc[4 * g4 + 3] * scale));
    }
    __syncthreads();
    if (GAL) {
      for (int b = 0; b < nvalid; b += 64) {   // (block-uniform trip count: the barrier inside is reached by every thread)
        const int e = b + lane;
        float r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          r[i] = 0.f;
          if (i < nv && e < nvalid) {
            const float* x = xt + (wave * 4 + i) * TK_TS + e * n;
            r[i] = pool_any(mode, n, [&](int j) { return x[j]; });
          }
        }
        __syncthreads();   // every read of this batch is done before column e (<= e n) is overwritten
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nv && e < nvalid) tile[(wave * 4 + i) * TK_TS + e] = mono_key(r[i]);
      }
    } else if (tid < nvalid) {
      for (int v = 0; v < tile_lists; ++v) {
        const float* x = xt + v * n * TK_TS + tid;
        const float r = pool_any(mode, n, [&](int j) { return x[j * TK_TS]; });
        tile[v * TK_TS + tid] = mono_key(r);   // row v <= v n: read by this thread alone, for videos <= v
      }
    }
    __syncthreads();
    TK_SELECT_NV(nv, tile + wave * 4 * TK_TS, lane, nvalid, sub, kp, run);
    __syncthreads();   // the next sub-pass overwrites the tile
  }
  tk_write_lists(ws, list0 + wave * 4, nv, nchunks, c, kp, lane, run);
}

struct ClipsPlan {
  int nlists, nent;
  TopkPlan t;
};

// false (with the error text set) for arguments the kernels do not take
bool clips_plan(const char* who, int nq, int ng, int k, int clips, int side, int chunk, ClipsPlan& p) {
  if (clips < 1 || clips > ALPRO_TOPK_MAX_CLIPS) { set_error("%s: clips=%d (need 1..%d = ALPRO_TOPK_MAX_CLIPS)", who, clips, ALPRO_TOPK_MAX_CLIPS); return false; }
  if (side != ALPRO_TOPK_CLIPS_GALLERY && side != ALPRO_TOPK_CLIPS_QUERY) {
    set_error("%s: side=%d (0 = ALPRO_TOPK_CLIPS_GALLERY, 1 = ALPRO_TOPK_CLIPS_QUERY)", who, side);
    return false;
  }
  if (nq < 1) { set_error("%s: nq=%d queries (need >= 1)", who, nq); return false; }
  if (ng < 1) { set_error("%s: ng=%d gallery rows (need >= 1)", who, ng); return false; }
  const bool gal = side == ALPRO_TOPK_CLIPS_GALLERY;
  if (gal && ng % clips != 0) { set_error("%s: ng=%d gallery rows are not a whole number of videos of clips=%d", who, ng, clips); return false; }
  if (!gal && nq % clips != 0) { set_error("%s: nq=%d query rows are not a whole number of videos of clips=%d", who, nq, clips); return false; }
  p.nlists = gal ? nq : nq / clips;
  p.nent = gal ? ng / clips : ng;
  // (the library's chunk is alpro_sim_topk's, 512 .. 128, in ENTRIES: a GALLERY chunk of videos is walked in sub-passes of floor(512 / clips))
  return topk_plan(who, p.nlists, p.nent, k, chunk, p.t, gal ? TK_QT : TK_QT / clips);
}

DeviceOnce g_clips_once[2];

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" size_t alpro_sim_topk_clips_workspace_bytes(int nq, int ng, int k, int clips, int side, int chunk) {
  ClipsPlan p;
  return clips_plan("alpro_sim_topk_clips_workspace_bytes", nq, ng, k, clips, side, chunk, p) ? p.t.total : 0;
}

extern "C" int alpro_sim_topk_clips(const float* q, int nq, const float* g, int ng, int d, int k, float scale, int clips, int side, int mode, int chunk,
                                    float* out_val, int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
  ALPRO_CHECK(d == TK_D, "alpro_sim_topk_clips: d=%d (the kernel is built for the model's embed_dim, %d)", d, TK_D);
  ALPRO_CHECK(mode == ALPRO_POOL_MEAN || mode == ALPRO_POOL_MAX || mode == ALPRO_POOL_LSE, "alpro_sim_topk_clips: mode=%d (0 = mean, 1 = max, 2 = lse)", mode);
  ClipsPlan p;
  if (!clips_plan("alpro_sim_topk_clips", nq, ng, k, clips, side, chunk, p)) return ALPRO_ERR_INVALID;
  ALPRO_CHECK(q && g && out_val && out_idx && workspace, "alpro_sim_topk_clips: null pointer");
  ALPRO_CHECK(((uintptr_t)q % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)out_val % 4) == 0 && ((uintptr_t)out_idx % 4) == 0,
              "alpro_sim_topk_clips: misaligned pointers (q, g: 16 bytes)");
  ALPRO_CHECK(((uintptr_t)workspace % 256) == 0, "alpro_sim_topk_clips: workspace %p is not 256-byte aligned", workspace);
  ALPRO_CHECK(workspace_bytes >= p.t.total, "alpro_sim_topk_clips: workspace_bytes=%zu, need %zu (alpro_sim_topk_clips_workspace_bytes)", workspace_bytes,
              p.t.total);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  const dim3 grid((unsigned)(p.t.nqt * p.t.nchunks));
  if (side == ALPRO_TOPK_CLIPS_GALLERY) {
    set_lds_once(g_clips_once[0], sim_topk_clips_partial_kernel<ALPRO_TOPK_CLIPS_GALLERY>, TK_P1_LDS);
    hipLaunchKernelGGL(sim_topk_clips_partial_kernel<ALPRO_TOPK_CLIPS_GALLERY>, grid, dim3(TK_P1_THREADS), TK_P1_LDS, st, q, nq, g, ng, clips, mode, scale,
                       p.t.chunk, p.t.nchunks, p.t.nqt, p.t.kp, (uint64_t*)ws);
  } else {
    set_lds_once(g_clips_once[1], sim_topk_clips_partial_kernel<ALPRO_TOPK_CLIPS_QUERY>, TK_P1_LDS);
    hipLaunchKernelGGL(sim_topk_clips_partial_kernel<ALPRO_TOPK_CLIPS_QUERY>, grid, dim3(TK_P1_THREADS), TK_P1_LDS, st, q, nq, g, ng, clips, mode, scale,
                       p.t.chunk, p.t.nchunks, p.t.nqt, p.t.kp, (uint64_t*)ws);
  }
  const int rc = check_launch("alpro_sim_topk_clips (partial)");
  if (rc) return rc;
  return topk_merge("alpro_sim_topk_clips (merge)", p.t, p.nlists, k, 1.0f, out_val, out_idx, ws, st);
}
