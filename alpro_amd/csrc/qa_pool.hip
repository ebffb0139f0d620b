// Multi-clip pooling of video-QA logits (run_video_qa.py:249-276, score_agg_func): the per-clip answer logits of one question -- C rows of A
// labels, question-major -- pooled by mean / max / logsumexp, and the answer = the first index of the pooled row's maximum (torch's max(-1)[1]).
// The reference stacks the clips' logits on the host and pools there; here it is one launch over the device logits, and one host copy of the
// (B,) answers follows.  One workgroup per question: each thread pools its columns over the C clips in clip order, then a fixed-shape tree
// (wave shuffles, then 4 wave results through LDS) finds the argmax.  Memory-bound (B*C*A floats read once), no atomics: bitwise reproducible.
#include "clip_pool.hpp"

namespace alpro {
namespace {

// (value, index) pair order of the argmax: larger value, then the smaller index (first occurrence, as torch.max)
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <int MODE>
__global__ __launch_bounds__(256) void clip_pool_kernel(const float* __restrict__ logits, int64_t ld, float* __restrict__ pooled, int64_t ldo,
                                                        int64_t* __restrict__ pred, int C, int A) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)b * C * ld;
  float* out = pooled + (int64_t)b * ldo;
  float best = -INFINITY;
  int best_i = A;   // past every column: loses to any real one
  for (int j = tid; j < A; j += 256) {
    const float r = clip_pool_value<MODE>(C, [&](int c) { return x[(int64_t)c * ld + j]; });
    out[j] = r;
    take_better(best, best_i, r, j);   // j grows: a later column wins only on a larger value
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(best_i, off, 64);
    take_better(best, best_i, ov, oi);
  }
  if (lane == 0) { sv[wave] = best; si[wave] = best_i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) take_better(best, best_i, sv[w], si[w]);
    pred[b] = best_i < A ? (int64_t)best_i : 0;   // (only an all -inf / NaN row has no strict winner: answer 0, as torch.argmax of all -inf)
  }
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_clip_pool(const float* logits, int64_t ld, float* pooled, int64_t ldo, int64_t* pred, int B, int C, int A, int mode, void* stream) {
  ALPRO_CHECK(logits && pooled && pred && B > 0 && A > 0, "alpro_clip_pool: bad args");
  ALPRO_CHECK(C >= 1, "alpro_clip_pool: C=%d clips per question (need >= 1)", C);
  ALPRO_CHECK(ld >= A && ldo >= A, "alpro_clip_pool: row strides ld=%lld / ldo=%lld shorter than A=%d", (long long)ld, (long long)ldo, A);
  ALPRO_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)pooled % 4) == 0 && ((uintptr_t)pred % 8) == 0, "alpro_clip_pool: misaligned pointers");
  ALPRO_CHECK(mode == ALPRO_POOL_MEAN || mode == ALPRO_POOL_MAX || mode == ALPRO_POOL_LSE, "alpro_clip_pool: mode %d (0 = mean, 1 = max, 2 = lse)", mode);
  hipStream_t st = (hipStream_t)stream;
  if (mode == ALPRO_POOL_MEAN) hipLaunchKernelGGL(clip_pool_kernel<ALPRO_POOL_MEAN>, dim3(B), dim3(256), 0, st, logits, ld, pooled, ldo, pred, C, A);
  else if (mode == ALPRO_POOL_MAX) hipLaunchKernelGGL(clip_pool_kernel<ALPRO_POOL_MAX>, dim3(B), dim3(256), 0, st, logits, ld, pooled, ldo, pred, C, A);
  else hipLaunchKernelGGL(clip_pool_kernel<ALPRO_POOL_LSE>, dim3(B), dim3(256), 0, st, logits, ld, pooled, ldo, pred, C, A);
  return check_launch("alpro_clip_pool");
}
