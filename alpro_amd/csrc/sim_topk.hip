// Similarity + top-k in one pass (stage 1 of the two-stage retrieval search, alpro_amd/retrieval_eval.py rerank_retrieval): for every query row
// of q (nq, 256) the k largest fp32 dot products with the rows of g (ng, 256) and their gallery indices, WITHOUT the (nq, ng) matrix.
//
// The order of the candidates (one 64-bit key each) and everything shared with the multi-clip search is in sim_topk.hpp.
//
// Phase 1 (sim_topk_partial_kernel): one workgroup (8 waves) per (32-query tile, gallery chunk).  The 32 query rows are staged once into LDS in
// MFMA operand order; the chunk is walked in sub-passes of up to 512 gallery rows.  Per sub-pass the waves share its 32-row sub-tiles: a wave
// computes a 32 (gallery) x 32 (query) tile with 128 v_mfma_f32_32x32x2_f32 -- lane half h supplies k = 2s + h at step s, so every element is the
// k-ordered fp32 fmaf chain from 0 -- and stores the 32-bit value keys into the LDS tile [query][gallery row of the sub-pass].  The gallery rows
// come straight from global memory, a row per lane: the two lanes of a row load alternate 16-byte pieces and one v_permlane32_swap per register
// pair sorts the k of parity h into lane half h (half the load instructions of "both lanes load everything and pick").  Then wave w selects
// for its real queries among 4w .. 4w+3 (interleaved: a round is a chain of dependent cross-lane steps): each lane builds the 64-bit keys of 8 tile columns, adds its
// 2 entries of the query's running list (registers, rank = lane and lane + 64), and min(k, chunk) rounds of "wave maximum, the owner drops it"
// produce the new running list in order.  After the last sub-pass the list goes to the workspace: ws[query][chunk][min(k, chunk)].
// Phase 2 (sim_topk_merge_kernel): one workgroup per (query, group of up to 8 lists per thread).  The lists are sorted, so a thread only tracks
// the head of each of its lists; k rounds of "workgroup maximum, the owner advances that list" emit the merged list in order -- to the next
// workspace level while more than one group is left, else decoded to out_val (= s * scale, one fp32 multiply) / out_idx.
// No atomics anywhere; every output element has exactly one writer.
#include "sim_topk.hpp"

namespace alpro {
namespace {

__global__ __launch_bounds__(TK_P1_THREADS) void sim_topk_partial_kernel(const float* __restrict__ q, int nq, const float* __restrict__ g, int ng,
                                                                         int chunk, int nchunks, int nqt, int kp, uint64_t* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  float* Qs = (float*)tk_smem;                            // the 32 queries in MFMA operand order (tk_stage_queries)
  uint32_t* tile = (uint32_t*)(tk_smem + TK_QS_BYTES);    // [query][gallery row of the sub-pass], value keys
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % nqt, c = blockIdx.x / nqt;
  const int q0 = qt * TK_QT;
  tk_stage_queries(Qs, q, q0, nq, tid);
  __syncthreads();
  const int64_t c_begin = (int64_t)c * chunk;
  const int64_t c_end = min((int64_t)ng, c_begin + chunk);
  const int nv = min(4, max(0, nq - (q0 + wave * 4)));   // wave-uniform: the real queries among this wave's four
  uint64_t run[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) run[i][0] = run[i][1] = 0;

  for (int64_t sub = c_begin; sub < c_end; sub += TK_TILE) {
    const int nvalid = (int)min((int64_t)TK_TILE, c_end - sub);
    const int nst = (nvalid + 31) >> 5;
    for (int st = wave; st < nst; st += TK_P1_THREADS / 64) {
      const int64_t grow = min(sub + st * 32 + l31, (int64_t)ng - 1);   // rows past ng repeat the last row; masked when the keys are built
      const f32x16 acc = tk_subtile(Qs, (const f32x4*)(g + (size_t)grow * TK_D), l31, h);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *(u32x4*)&tile[l31 * TK_TS + st * 32 + 8 * g4 + 4 * h] =
            mk4(mono_key(acc[4 * g4]), mono_key(acc[4 * g4 + 1]), mono_key(acc[4 * g4 + 2]), mono_key(acc[4 * g4 + 3]));
    }
    __syncthreads();
    TK_SELECT_NV(nv, tile + wave * 4 * TK_TS, lane, nvalid, sub, kp, run);
    __syncthreads();   // the next sub-pass overwrites the tile
  }
  tk_write_lists(ws, q0 + wave * 4, nv, nchunks, c, kp, lane, run);
}

DeviceOnce g_partial_once;

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" size_t alpro_sim_topk_workspace_bytes(int nq, int ng, int k, int chunk) {
  TopkPlan p;
  return topk_plan("alpro_sim_topk_workspace_bytes", nq, ng, k, chunk, p) ? p.total : 0;
}

extern "C" int alpro_sim_topk(const float* q, int nq, const float* g, int ng, int d, int k, float scale, int chunk, float* out_val, int32_t* out_idx,
                              void* workspace, size_t workspace_bytes, void* stream) {
  ALPRO_CHECK(d == TK_D, "alpro_sim_topk: d=%d (the kernel is built for the model's embed_dim, %d)", d, TK_D);
  TopkPlan p;
  if (!topk_plan("alpro_sim_topk", nq, ng, k, chunk, p)) return ALPRO_ERR_INVALID;
  ALPRO_CHECK(q && g && out_val && out_idx && workspace, "alpro_sim_topk: null pointer");
  ALPRO_CHECK(((uintptr_t)q % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)out_val % 4) == 0 && ((uintptr_t)out_idx % 4) == 0,
              "alpro_sim_topk: misaligned pointers (q, g: 16 bytes)");
  ALPRO_CHECK(((uintptr_t)workspace % 256) == 0, "alpro_sim_topk: workspace %p is not 256-byte aligned", workspace);
  ALPRO_CHECK(workspace_bytes >= p.total, "alpro_sim_topk: workspace_bytes=%zu, need %zu (alpro_sim_topk_workspace_bytes)", workspace_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  set_lds_once(g_partial_once, sim_topk_partial_kernel, TK_P1_LDS);
  hipLaunchKernelGGL(sim_topk_partial_kernel, dim3((unsigned)(p.nqt * p.nchunks)), dim3(TK_P1_THREADS), TK_P1_LDS, st, q, nq, g, ng, p.chunk, p.nchunks,
                     p.nqt, p.kp, (uint64_t*)ws);
  const int rc = check_launch("alpro_sim_topk (partial)");
  if (rc) return rc;
  return topk_merge("alpro_sim_topk (merge)", p, nq, k, scale, out_val, out_idx, ws, st);
}
