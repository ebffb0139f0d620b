// Temporal attention probabilities of the visual encoder, materialised on request (TimeSformer.forward_features output_attentions; the tensor
// vit.py:92-93 hands to attn_drop on the (b h w) t m view of vit.py:147): P[g, h, q, k] = exp(scale * <q_(gT+q, h), k_(gT+k, h)> - lse[gT+q, h]),
// fp32, (rows / T, H, T, T); s = acc * scale (layout, orientation and the probability: attn_map.hpp).  alpro_attn_temporal_fwd and
// alpro_gemm_qkv_tattn leave lse in chunks of 32 rows, ((rows + 31) / 32, H, 32): row c * 32 + r of head h at [c, h, r].
//
// Two forms, one wave per work item in both:
//   T divides 32 (1, 2, 4, 8, 16, 32)  "unit" form, the temporal forward's: an item is a (32-row unit, head).  A unit holds 32 / T whole groups
//       (rows % T == 0, so the ragged last unit holds whole groups too); the wave forms the 32 x 32 S^T of the unit against itself ONCE -- the
//       same rows are the key and the query operand -- and stores only the block-diagonal entries (key and query of one group).  A 32 x 32
//       tile per (group, head) would leave 15 / 16 of every MFMA empty at T = 8.  T % 4 == 0: the four keys of a register group belong to one
//       group, one 16-byte store along k; T = 1, 2: 4-byte stores.
//   any other T <= 128                 "tile" form: an item is a (group, head, 32-query tile, 32-key tile), at most 4 x 4 tiles per (group, head).
//       Groups straddle the 32-row lse chunks: the lse row is addressed by its absolute row.
#include "attn_map.hpp"

namespace alpro {
namespace {

// T divides 32; sh = log2 T.  items = units * H, unit-major.
template <typename T>
__global__ __launch_bounds__(MAP_THREADS) void tprobs_unit_kernel(const T* __restrict__ qkv, const float* __restrict__ lse, float* __restrict__ out,
                                                                  int64_t rows, int sh, int H, float scale, int64_t items) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
  const int64_t item = (int64_t)blockIdx.x * MAP_WAVES + wave;
  if (item >= items) return;                   // wave-uniform
  const int64_t u = item / H;
  const int h = (int)(item - u * H);
  const int Tn = 1 << sh;
  const int64_t ld = (int64_t)3 * H * 64;
  const int64_t grow = u * 32 + l31;           // this lane's row: key row l31 of the A operand and query row l31 of the B operand
  const bool rok = grow < rows;                // (rows past the end repeat the last one and store nothing)
  const int64_t lrow = rok ? grow : rows - 1;
  u32x4 qf[MAP_NCH<T>], kf[MAP_NCH<T>];
  map_load_row(qf, qkv + lrow * ld + h * 64, hh);
  map_load_row(kf, qkv + lrow * ld + (H + h) * 64, hh);
  f32x16 acc;
  map_tile<T>(acc, kf, qf);
  const float lq = lse[(u * H + h) * 32 + (rok ? l31 : (int)(rows - 1 - u * 32))];
  // register r: key (r & 3) + 8 (r >> 2) + 4 hh of the unit, query l31
  const int qg = l31 >> sh;                    // group of the query inside the unit
  float* orow = out + ((((u * 32) >> sh) + qg) * H + h) * ((int64_t)Tn * Tn) + (int64_t)(l31 & (Tn - 1)) * Tn;
  if (sh >= 2) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kb = 8 * g + 4 * hh;
      if (rok && (kb >> sh) == qg)
        *(f32x4*)(orow + (kb & (Tn - 1))) = f32x4{map_prob(acc[4 * g] * scale, lq), map_prob(acc[4 * g + 1] * scale, lq), map_prob(acc[4 * g + 2] * scale, lq),
                                                 map_prob(acc[4 * g + 3] * scale, lq)};
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (rok && (kk >> sh) == qg) orow[kk & (Tn - 1)] = map_prob(acc[r] * scale, lq);
    }
  }
}

// any T; nt = (T + 31) / 32 tiles per side.  items = groups * H * nt * nt, group-major, then head, query tile, key tile.
template <typename T>
__global__ __launch_bounds__(MAP_THREADS) void tprobs_tile_kernel(const T* __restrict__ qkv, const float* __restrict__ lse, float* __restrict__ out,
                                                                  int Tn, int nt, int H, float scale, int64_t items) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
  const int64_t item = (int64_t)blockIdx.x * MAP_WAVES + wave;
  if (item >= items) return;                   // wave-uniform
  const int kt = (int)(item % nt), qt = (int)((item / nt) % nt);
  const int64_t gh = item / (nt * nt);
  const int64_t grp = gh / H;
  const int h = (int)(gh - grp * H);
  const int64_t ld = (int64_t)3 * H * 64;
  const int qi = qt * 32 + l31, kj = kt * 32 + l31;      // rows past T repeat the last one of the group and are masked at the store
  const int64_t qrow = grp * Tn + min(qi, Tn - 1), krow = grp * Tn + min(kj, Tn - 1);
  u32x4 qf[MAP_NCH<T>], kf[MAP_NCH<T>];
  map_load_row(qf, qkv + qrow * ld + h * 64, hh);
  map_load_row(kf, qkv + krow * ld + (H + h) * 64, hh);
  f32x16 acc;
  map_tile<T>(acc, kf, qf);
  const float lq = lse[((qrow >> 5) * H + h) * 32 + (qrow & 31)];
  float* orow = out + (gh * Tn + min(qi, Tn - 1)) * Tn;
  const bool full = (Tn & 3) == 0 && (kt + 1) * 32 <= Tn;   // wave-uniform; row starts of `out` are 16-byte aligned
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int kb = kt * 32 + 8 * g + 4 * hh;
    float p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = map_prob(acc[4 * g + j] * scale, lq);
    map_store4(orow, p, qi < Tn, kb, Tn, full);
  }
}

template <typename T>
int launch_tprobs(const void* qkv, const float* lse, float* out, int64_t rows, int Tn, int H, float scale, hipStream_t st) {
  const int64_t items = tp_items(rows, Tn, H);
  const dim3 grid((unsigned)((items + MAP_WAVES - 1) / MAP_WAVES));
  if (32 % Tn == 0) {
    int sh = 0;
    while ((1 << sh) < Tn) ++sh;
    hipLaunchKernelGGL((tprobs_unit_kernel<T>), grid, dim3(MAP_THREADS), 0, st, (const T*)qkv, lse, out, rows, sh, H, scale, items);
  } else {
    hipLaunchKernelGGL((tprobs_tile_kernel<T>), grid, dim3(MAP_THREADS), 0, st, (const T*)qkv, lse, out, Tn, (Tn + 31) / 32, H, scale, items);
  }
  return check_launch("alpro_attn_temporal_probs");
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_attn_temporal_probs(const void* qkv, const float* lse, float* out, int dtype, int64_t rows, int T, int H, float scale, void* stream) {
  // every check in front of the first HIP call: the refusals are testable without a device
  if (int rc = map_temporal_check("alpro_attn_temporal_probs", dtype, rows, T, H)) return rc;
  if (rows == 0) return ALPRO_OK;
  ALPRO_CHECK(qkv != nullptr, "alpro_attn_temporal_probs: null qkv");
  ALPRO_CHECK(lse != nullptr, "alpro_attn_temporal_probs: null lse");
  ALPRO_CHECK(out != nullptr, "alpro_attn_temporal_probs: null out");
  ALPRO_CHECK(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0, "alpro_attn_temporal_probs: qkv and out must be 16-byte aligned");
  ALPRO_CHECK(((uintptr_t)lse % 4) == 0, "alpro_attn_temporal_probs: lse must be 4-byte aligned");
  ALPRO_DISPATCH_DTYPE(dtype, T_, return launch_tprobs<T_>(qkv, lse, out, rows, T, H, scale, (hipStream_t)stream));
  return ALPRO_OK;
}
