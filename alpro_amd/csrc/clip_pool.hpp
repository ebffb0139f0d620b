// The one pooling rule of multi-clip evaluation (run_video_qa.py:269-279, score_agg_func), shared by alpro_clip_pool (qa_pool.hip: QA and
// retrieval logits, similarity matrices) and alpro_sim_topk_clips (sim_topk_clips.hip: top-k by pooled similarity), so the two cannot drift:
// a value pooled here and a value pooled there from the same fp32 inputs have the same bits.
#pragma once
#include "common.hpp"

namespace alpro {

// x(c) = clip c's value, c = 0 .. C - 1, C >= 1.
//   mean: sequential fp32 sum from 0 in ascending c, then / (float)C
//   max:  fmaxf in ascending c
//   lse:  m + logf(sum_c expf(x_c - m)), m the maximum, sum in ascending c; all clips -inf -> -inf (torch.logsumexp), a +inf clip -> +inf
template <int MODE, class Load>
__device__ __forceinline__ float clip_pool_value(int C, Load x) {
  if (MODE == ALPRO_POOL_MEAN) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += x(c);
    return s / (float)C;
  }
  float m = x(0);
  for (int c = 1; c < C; ++c) m = fmaxf(m, x(c));
  if (MODE == ALPRO_POOL_MAX || m == -INFINITY || m == INFINITY) return m;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(x(c) - m);
  return m + logf(s);
}

}  // namespace alpro
