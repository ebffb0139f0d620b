// Step epilogue of the data-parallel training loop on flat fp32 buffers: global gradient norm and the
// reference's HF-style AdamW (src/optimization/adamw.py:40-103) with the clip_grad_norm_ coefficient
// (run_pretrain_sparse.py:633) folded in.  One pass over (param, grad, m, v): 16 B/param read + 12 B/param written.
#include "common.hpp"
#include <algorithm>
#include <type_traits>

namespace alpro {
namespace {

// part == nullptr: out += sum(x^2) through one fp32 atomic per workgroup (order varies run to run).  part given: workgroup b leaves its sum in
// part[b] and sumsq_finish_kernel adds the slots in a fixed order -- the squared norm feeds the clip coefficient of EVERY parameter, so a
// last-bit difference here would make two identical steps differ everywhere.
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out, float* __restrict__ part) {
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      const float4 v = *(const float4*)(x + i);
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    } else {
      for (int64_t k = i; k < n; ++k) s += x[k] * x[k];
    }
  }
  s = wave_sum(s);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = sh[0] + sh[1] + sh[2] + sh[3];
    if (part) part[blockIdx.x] = t;
    else atomicAdd(out, t);
  }
}

// out += sum of part[0 .. n): one workgroup, thread t adds slots t, t + 256, ... in ascending order, then a fixed tree.
__global__ __launch_bounds__(256) void sumsq_finish_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum(s);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out += (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- the pieces adamw_kernel and adamw_groups_kernel share (profiles/r12_rowwise_isa.txt: which ones, and why not the others) ----------------
// torch.nn.utils.clip_grad_norm_ folded into the gradient coefficient: ONE coefficient from the global norm, over all parameters
__device__ __forceinline__ float adamw_clip(float coef, const float* gnorm_sq, float max_norm) {
  if (gnorm_sq && max_norm > 0.f) {
    const float total = sqrtf(*gnorm_sq) * coef;
    coef *= fminf(max_norm / (total + 1e-6f), 1.0f);
  }
  return coef;
}

// one whole chunk back to memory.  LP: storage type of the optional 16-bit mirror of the parameters (float = none)
template <typename LP>
__device__ __forceinline__ void adamw_store4(float* p, float* g, float* m, float* v, LP* lp, int zero_grad, int64_t i, const float (&pv)[4],
                                             const float (&mv)[4], const float (&vv)[4]) {
  *(float4*)(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
  *(float4*)(m + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
  *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
  if (zero_grad) *(float4*)(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);   // optimizer.zero_grad() folded in (round 4): no separate 0.94 GB memset
  if constexpr (sizeof(LP) == 2) {
    if (lp) *(u32x2*)(lp + i) = mk2(pack2(pv[0], pv[1], (LP*)0), pack2(pv[2], pv[3], (LP*)0));   // the same roundings as alpro_cast_from_f32
  }
}

// LP: storage type of the optional 16-bit mirror of the parameters (the GEMM operands' flat copy, alpro_adamw_step_lp; float = none).
template <typename LP>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float beta1, float beta2, float eps,
                                                    float weight_decay, float step_size, const float* __restrict__ gnorm_sq,
                                                    float max_norm, float grad_scale, const float* __restrict__ dyn, int grads_scaled,
                                                    int correct_bias, int zero_grad, LP* __restrict__ lp) {
  float coef = grad_scale;
  if (dyn) {
    // dynamic loss scaling (fp16 operands; apex.amp semantics, run_pretrain_sparse.py:596-634 with fp16 = 1): dyn = {loss scale S,
    // growth tracker, completed optimizer steps}.  The gradients hold S * dL/dw (unless the caller already unscaled them); a non-finite
    // squared norm means some fp16 gradient operand overflowed: the whole update is skipped -- parameters, moments and the 16-bit mirror
    // untouched -- and alpro_loss_scale_update halves S.  The bias correction uses the DEVICE step counter, which only counts applied updates.
    if (!isfinite(*gnorm_sq)) {   // skipped step: nothing moves -- but a caller that asked for consumed gradients still gets them zeroed
      if (zero_grad) {
        const int64_t stride0 = (int64_t)gridDim.x * blockDim.x * 4;
        for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride0)
          for (int k = 0; k < 4 && i + k < n; ++k) g[i + k] = 0.f;
      }
      return;
    }
    if (grads_scaled) coef /= dyn[0];
    const float t = dyn[2] + 1.0f;
    step_size = correct_bias ? lr * sqrtf(1.0f - powf(beta2, t)) / (1.0f - powf(beta1, t)) : lr;
  }
  coef = adamw_clip(coef, gnorm_sq, max_norm);
  auto update = [&](float (&pv)[4], const float (&gv)[4], float (&mv)[4], float (&vv)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gv[k] * coef;
      mv[k] = mv[k] * beta1 + (1.0f - beta1) * gr;
      vv[k] = vv[k] * beta2 + (1.0f - beta2) * gr * gr;
      const float denom = sqrtf(vv[k]) + eps;
      pv[k] = pv[k] - step_size * (mv[k] / denom);
      if (weight_decay > 0.f) pv[k] = pv[k] - lr * weight_decay * pv[k];
    }
  };
  auto store4 = [&](int64_t i, const float (&pv)[4], const float (&mv)[4], const float (&vv)[4]) { adamw_store4<LP>(p, g, m, v, lp, zero_grad, i, pv, mv, vv); };
  // Two float4 of each array per iteration (round 6): all eight loads are issued before the first divide -- one float4 per array left the pass at
  // 5.1 TB/s with three quarters of the wave cycles stalled on memory.
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += 2 * stride) {
    const int64_t j = i + stride;
    if (j + 4 <= n) {   // (i + 4 <= n as well)
      const float4 a0 = *(const float4*)(p + i), b0 = *(const float4*)(g + i), c0 = *(const float4*)(m + i), d0 = *(const float4*)(v + i);
      const float4 a1 = *(const float4*)(p + j), b1 = *(const float4*)(g + j), c1 = *(const float4*)(m + j), d1 = *(const float4*)(v + j);
      float pv0[4] = {a0.x, a0.y, a0.z, a0.w}, mv0[4] = {c0.x, c0.y, c0.z, c0.w}, vv0[4] = {d0.x, d0.y, d0.z, d0.w};
      float pv1[4] = {a1.x, a1.y, a1.z, a1.w}, mv1[4] = {c1.x, c1.y, c1.z, c1.w}, vv1[4] = {d1.x, d1.y, d1.z, d1.w};
      const float gv0[4] = {b0.x, b0.y, b0.z, b0.w}, gv1[4] = {b1.x, b1.y, b1.z, b1.w};
      update(pv0, gv0, mv0, vv0);
      store4(i, pv0, mv0, vv0);
      update(pv1, gv1, mv1, vv1);
      store4(j, pv1, mv1, vv1);
      continue;
    }
    for (int64_t q = i; q < n && q <= j; q += stride) {   // the last one or two chunks of this thread, element by element where they are ragged
      const int cnt = (q + 4 <= n) ? 4 : (int)(n - q);
      float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < cnt; ++k) { pv[k] = p[q + k]; gv[k] = g[q + k]; mv[k] = m[q + k]; vv[k] = v[q + k]; }
      update(pv, gv, mv, vv);
      if (cnt == 4) {
        store4(q, pv, mv, vv);
      } else {
        for (int k = 0; k < cnt; ++k) {
          p[q + k] = pv[k]; m[q + k] = mv[k]; v[q + k] = vv[k];
          if (zero_grad) g[q + k] = 0.f;
          if constexpr (sizeof(LP) == 2) { if (lp) lp[q + k] = from_f32<LP>(pv[k]); }
        }
      }
    }
  }
}

// ---- parameter groups: adamw_kernel with the hyper-parameters of a chunk taken from a segment table (alpro_adamw_step_groups) ---------------
// The table sits in the kernel arguments and is only read.  A wave's 64 chunks are 256 consecutive elements, so all but the few waves that
// straddle a segment boundary (at most count - 1 per trip) need ONE segment per chunk.  The loop runs on the WAVE's base index (uniform
// control flow): per chunk in flight the wave keeps the range and the hyper-parameters of the segment it met last in scalar registers, a
// chunk inside that range costs two scalar compares and the update reads its hyper-parameters from SGPRs exactly as adamw_kernel reads its
// arguments.  A wave that leaves the range walks the table again -- its chunks ascend, so at most `count` times, the powf pair of the
// loss-scaling step size with it.  Straddling waves and the last, partial trip go one chunk at a time with a per-lane look-up.
struct SegHP {
  float lr, beta1, beta2, eps, weight_decay, step_size;
};

struct SegCache {   // wave-uniform: [lo, hi) of the cached segment (empty = nothing cached) and its hyper-parameters
  int64_t lo = 0, hi = 0;
  SegHP hp;
};

__device__ __forceinline__ int64_t first_lane_i64(int64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// dyn_t > 0: dynamic loss scaling, the step size comes from the DEVICE step counter (dyn_t = applied steps + 1) and this segment's own lr / betas
__device__ __forceinline__ SegHP seg_hp(const alpro_adamw_segment_t& s, float dyn_t) {
  SegHP h = {s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, s.step_size};
  if (dyn_t > 0.f) h.step_size = s.correct_bias ? s.lr * sqrtf(1.0f - powf(s.beta2, dyn_t)) / (1.0f - powf(s.beta1, dyn_t)) : s.lr;
  return h;
}

// qw: wave-uniform first element of a wave's 256.  True: all of [qw, qw + 256) lies in the segment c describes (found again if need be).
__device__ __forceinline__ bool seg_find(const alpro_adamw_segments_t& tab, int64_t qw, float dyn_t, SegCache& c) {
  if (qw >= c.lo && qw + 256 <= c.hi) return true;
  int s = 0;
  while (s < tab.count - 1 && qw >= tab.seg[s].end) ++s;
  const bool last = s == tab.count - 1;
  if (!last && qw + 256 > tab.seg[s].end) return false;   // a boundary inside the wave's 256 elements
  c.lo = s ? tab.seg[s - 1].end : 0;
  c.hi = last ? INT64_MAX : tab.seg[s].end;               // (the last end is n, which the wave's span may pass: its chunks do not)
  c.hp = seg_hp(tab.seg[s], dyn_t);
  c.hp.step_size = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c.hp.step_size)));   // computed on the vector ALU, equal in every lane
  return true;
}

// Per lane: the segment of the chunk that starts at q (a multiple of 4; so is every end but the last: a chunk has one segment).
__device__ __forceinline__ SegHP seg_of_lane(const alpro_adamw_segments_t& tab, int64_t q, float dyn_t) {
  int s = 0;
  for (int k = 0; k < tab.count - 1; ++k) s += (q >= tab.seg[k].end) ? 1 : 0;
  return seg_hp(tab.seg[s], dyn_t);
}

template <typename LP>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           int64_t n, const alpro_adamw_segments_t tab, const float* __restrict__ gnorm_sq,
                                                           float max_norm, float grad_scale, const float* __restrict__ dyn, int grads_scaled,
                                                           int zero_grad, LP* __restrict__ lp) {
  float coef = grad_scale;
  float dyn_t = 0.f;
  if (dyn) {   // as adamw_kernel: a non-finite norm skips EVERY segment, the gradients are still consumed when the caller asked for that
    if (!isfinite(*gnorm_sq)) {
      if (zero_grad) {
        const int64_t stride0 = (int64_t)gridDim.x * blockDim.x * 4;
        for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride0)
          for (int k = 0; k < 4 && i + k < n; ++k) g[i + k] = 0.f;
      }
      return;
    }
    if (grads_scaled) coef /= dyn[0];
    dyn_t = dyn[2] + 1.0f;
  }
  coef = adamw_clip(coef, gnorm_sq, max_norm);
  auto update = [&](const SegHP& h, float (&pv)[4], const float (&gv)[4], float (&mv)[4], float (&vv)[4]) {
    const float lr = h.lr, beta1 = h.beta1, beta2 = h.beta2, eps = h.eps, weight_decay = h.weight_decay, step_size = h.step_size;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // the statements of adamw_kernel, unchanged: equal hyper-parameters give equal bits
      const float gr = gv[k] * coef;
      mv[k] = mv[k] * beta1 + (1.0f - beta1) * gr;
      vv[k] = vv[k] * beta2 + (1.0f - beta2) * gr * gr;
      const float denom = sqrtf(vv[k]) + eps;
      pv[k] = pv[k] - step_size * (mv[k] / denom);
      if (weight_decay > 0.f) pv[k] = pv[k] - lr * weight_decay * pv[k];
    }
  };
  auto store4 = [&](int64_t i, const float (&pv)[4], const float (&mv)[4], const float (&vv)[4]) { adamw_store4<LP>(p, g, m, v, lp, zero_grad, i, pv, mv, vv); };
  auto one_chunk = [&](int64_t q) {   // a chunk on its own, element by element where it is ragged, its segment looked up by the lane
    if (q >= n) return;
    const int cnt = (q + 4 <= n) ? 4 : (int)(n - q);
    const SegHP h = seg_of_lane(tab, q, dyn_t);
    float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < cnt; ++k) { pv[k] = p[q + k]; gv[k] = g[q + k]; mv[k] = m[q + k]; vv[k] = v[q + k]; }
    update(h, pv, gv, mv, vv);
    if (cnt == 4) {
      store4(q, pv, mv, vv);
    } else {
      for (int k = 0; k < cnt; ++k) {
        p[q + k] = pv[k]; m[q + k] = mv[k]; v[q + k] = vv[k];
        if (zero_grad) g[q + k] = 0.f;
        if constexpr (sizeof(LP) == 2) { if (lp) lp[q + k] = from_f32<LP>(pv[k]); }
      }
    }
  };
  SegCache c0, c1;   // one per chunk in flight: the two are `stride` elements apart and usually in different segments
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  const int lane4 = (int)(threadIdx.x & 63) * 4;
  // the chunks of adamw_kernel's walk, thread for thread: i = ((blockIdx.x * blockDim.x + threadIdx.x) * 4 + trips * 2 * stride, j = i + stride
  for (int64_t iw = first_lane_i64(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4); iw < n; iw += 2 * stride) {
    const int64_t jw = iw + stride, i = iw + lane4, j = jw + lane4;
    if (jw + 256 <= n && seg_find(tab, iw, dyn_t, c0) && seg_find(tab, jw, dyn_t, c1)) {
      // two float4 of each array in flight as in adamw_kernel; every lane's two chunks are whole and each in ONE segment
      const float4 a0 = *(const float4*)(p + i), b0 = *(const float4*)(g + i), m0 = *(const float4*)(m + i), d0 = *(const float4*)(v + i);
      const float4 a1 = *(const float4*)(p + j), b1 = *(const float4*)(g + j), m1 = *(const float4*)(m + j), d1 = *(const float4*)(v + j);
      float pv0[4] = {a0.x, a0.y, a0.z, a0.w}, mv0[4] = {m0.x, m0.y, m0.z, m0.w}, vv0[4] = {d0.x, d0.y, d0.z, d0.w};
      float pv1[4] = {a1.x, a1.y, a1.z, a1.w}, mv1[4] = {m1.x, m1.y, m1.z, m1.w}, vv1[4] = {d1.x, d1.y, d1.z, d1.w};
      const float gv0[4] = {b0.x, b0.y, b0.z, b0.w}, gv1[4] = {b1.x, b1.y, b1.z, b1.w};
      update(c0.hp, pv0, gv0, mv0, vv0);
      store4(i, pv0, mv0, vv0);
      update(c1.hp, pv1, gv1, mv1, vv1);
      store4(j, pv1, mv1, vv1);
      continue;
    }
    one_chunk(i);
    one_chunk(j);
  }
}

// One thread: the loss-scale schedule of apex's dynamic LossScaler (scale_window 2000, halve on overflow, double after a window of
// clean steps, clamped), entirely on the device -- no host sync in the training loop.
__global__ void loss_scale_update_kernel(float* __restrict__ dyn, const float* __restrict__ gnorm_sq, float growth, float backoff,
                                         float window, float min_scale, float max_scale) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!isfinite(*gnorm_sq)) {
    dyn[0] = fmaxf(dyn[0] * backoff, min_scale);
    dyn[1] = 0.f;
    dyn[3] += 1.f;  // skipped steps
  } else {
    dyn[2] += 1.f;  // applied steps
    dyn[1] += 1.f;
    if (dyn[1] >= window) {
      dyn[0] = fminf(dyn[0] * growth, max_scale);
      dyn[1] = 0.f;
    }
  }
}

inline int grid_for(int64_t n) {
  int64_t g = (n / 4 + 255) / 256;
  if (g < 1) g = 1;
  if (g > 256 * 16) g = 256 * 16;
  return (int)g;
}

// what alpro_adamw_step_lp and alpro_adamw_step_groups ask of their buffers (`who`: the name the messages carry, `who_lp`: the mirror's)
int adamw_check_buffers(const char* who, const char* who_lp, const float* p, const float* g, const float* m, const float* v, const float* gnorm_sq,
                        const float* dyn_state, const void* lp, int lp_dtype) {
  ALPRO_CHECK(!dyn_state || gnorm_sq, "%s: dynamic loss scaling needs the squared gradient norm (overflow detection)", who);
  ALPRO_CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0, "%s: buffers must be 16-byte aligned", who);
  ALPRO_CHECK(!lp || ((lp_dtype == ALPRO_BF16 || lp_dtype == ALPRO_F16) && ((uintptr_t)lp % 8) == 0), "%s: the mirror is a 16-bit, 8-byte-aligned buffer", who_lp);
  return ALPRO_OK;
}

// launch(typed mirror pointer): bf16_t* / f16_t* for a 16-bit mirror, (float*)nullptr for none -- the kernel's LP is the pointee
template <typename F>
void adamw_launch_lp(void* lp, int lp_dtype, F&& launch) {
  if (lp && lp_dtype == ALPRO_BF16) launch((bf16_t*)lp);
  else if (lp) launch((f16_t*)lp);
  else launch((float*)nullptr);
}
}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_sumsq(const float* x, int64_t n, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ALPRO_CHECK(x && out && n > 0, "alpro_sumsq: bad args");
  ALPRO_CHECK(((uintptr_t)x % 16) == 0, "alpro_sumsq: x must be 16-byte aligned");
  ALPRO_CHECK(!workspace || (((uintptr_t)workspace % 4) == 0 && workspace_bytes >= sizeof(float)), "alpro_sumsq: bad workspace");
  int grid = grid_for(n);
  float* part = (float*)workspace;
  if (part) grid = (int)std::min<size_t>((size_t)grid, workspace_bytes / sizeof(float));
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, out, part);
  if (part) hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, grid, out);
  return check_launch("alpro_sumsq");
}

extern "C" int alpro_adamw_step_lp(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, float step_size, const float* gnorm_sq, float max_norm, float grad_scale,
                                   const float* dyn_state, int grads_scaled, int correct_bias, int zero_grad, void* lp, int lp_dtype, void* stream) {
  ALPRO_CHECK(p && g && m && v && n > 0, "alpro_adamw_step: bad args");
  if (int rc = adamw_check_buffers("alpro_adamw_step", "alpro_adamw_step_lp", p, g, m, v, gnorm_sq, dyn_state, lp, lp_dtype)) return rc;
  adamw_launch_lp(lp, lp_dtype, [&](auto* lpt) {
    hipLaunchKernelGGL(adamw_kernel<std::remove_pointer_t<decltype(lpt)>>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, step_size, gnorm_sq, max_norm, grad_scale, dyn_state, grads_scaled, correct_bias, zero_grad, lpt);
  });
  return check_launch("alpro_adamw_step");
}

#define ALPRO_STR_(x) #x
#define ALPRO_STR(x) ALPRO_STR_(x)

extern "C" int alpro_adamw_step_groups(float* p, float* g, float* m, float* v, int64_t n, const alpro_adamw_segments_t* segments,
                                       const float* gnorm_sq, float max_norm, float grad_scale, const float* dyn_state, int grads_scaled,
                                       int zero_grad, void* lp, int lp_dtype, void* stream) {
  ALPRO_CHECK(p && g && m && v && n > 0 && segments, "alpro_adamw_step_groups: bad args");
  ALPRO_CHECK(segments->count <= ALPRO_ADAMW_MAX_SEGMENTS,
              "alpro_adamw_step_groups: more than ALPRO_ADAMW_MAX_SEGMENTS = " ALPRO_STR(ALPRO_ADAMW_MAX_SEGMENTS) " segments (the table travels in the kernel arguments)");
  ALPRO_CHECK(segments->count >= 1, "alpro_adamw_step_groups: an empty segment table");
  if (int rc = adamw_check_buffers("alpro_adamw_step_groups", "alpro_adamw_step_groups", p, g, m, v, gnorm_sq, dyn_state, lp, lp_dtype)) return rc;
  alpro_adamw_segments_t tab = {};   // (a copy with the unused tail cleared: the kernel arguments carry no caller garbage)
  tab.count = segments->count;
  int64_t prev = 0;
  for (int k = 0; k < segments->count; ++k) {
    const alpro_adamw_segment_t& s = segments->seg[k];
    ALPRO_CHECK(s.end > prev && (s.end % 4 == 0 || k == segments->count - 1),
                "alpro_adamw_step_groups: segment ends must ascend strictly and, but for the last, be multiples of 4");
    prev = s.end;
    tab.seg[k] = s;
  }
  ALPRO_CHECK(prev == n, "alpro_adamw_step_groups: the segments must cover [0, n) exactly");
  adamw_launch_lp(lp, lp_dtype, [&](auto* lpt) {
    hipLaunchKernelGGL(adamw_groups_kernel<std::remove_pointer_t<decltype(lpt)>>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, tab, gnorm_sq,
                       max_norm, grad_scale, dyn_state, grads_scaled, zero_grad, lpt);
  });
  return check_launch("alpro_adamw_step_groups");
}

extern "C" int alpro_adamw_step(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                float weight_decay, float step_size, const float* gnorm_sq, float max_norm, float grad_scale,
                                const float* dyn_state, int grads_scaled, int correct_bias, int zero_grad, void* stream) {
  return alpro_adamw_step_lp(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step_size, gnorm_sq, max_norm, grad_scale, dyn_state, grads_scaled,
                             correct_bias, zero_grad, nullptr, ALPRO_F32, stream);
}

extern "C" int alpro_loss_scale_update(float* dyn_state, const float* gnorm_sq, float growth, float backoff, int window, float min_scale,
                                       float max_scale, void* stream) {
  ALPRO_CHECK(dyn_state && gnorm_sq && growth >= 1.f && backoff > 0.f && backoff <= 1.f && window > 0 && min_scale > 0.f && max_scale >= min_scale,
              "alpro_loss_scale_update: bad args");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dyn_state, gnorm_sq, growth, backoff, (float)window, min_scale, max_scale);
  return check_launch("alpro_loss_scale_update");
}
