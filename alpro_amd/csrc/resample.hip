// RandomResizedCrop on the device for the image-text stream (src/datasets/dataset_pretrain_sparse.py:125-193): crop a box out of each image
// of a batch of differently sized uint8 HWC images and resize it to S x S with PIL's 8-bit antialiased bicubic resampling, bit for bit, the
// horizontal flip folded into the store.  PIL's resize is separable -- a horizontal pass, the intermediate rounded to uint8, a vertical pass --
// and integer once its coefficients are fixed: out = clip8((2^21 + sum_t k[t] * pix[first + t]) >> 22).  The coefficients come from the HOST
// (alpro_amd.input_gpu.resample_coeffs, fp64 in numpy in PIL's order of operations), so there is no floating point in this file and nothing a
// contraction or a rounding mode could move.  Two launches over a planar uint8 workspace; byte work with no reuse worth staging, as in
// augment.hip: no LDS.  Measured times: DESIGN.md 4.12.
#include "common.hpp"

namespace alpro {
namespace {

constexpr int PRECISION_BITS = 22;   // PIL's 32 - 8 - 2
constexpr int META = 8;              // int64 per image: byte offset, H, W, top, left, h, w, flip

__device__ __forceinline__ int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
  const int v = (int)acc >> PRECISION_BITS;   // arithmetic shift, as PIL's
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Image b's geometry.  Every value comes from device memory and is clamped here, so that nothing there can move an address outside the packed
// buffer or the workspace (the Python wrapper refuses such values with a message; this is the bound itself): H x W x 3 bytes at `off` lie inside
// [0, src_bytes), the box lies inside the image, and its height inside the workspace's max_h rows.  An image that cannot lie inside the buffer
// at any offset is skipped (ok == false, workgroup-uniform).
struct Box {
  int64_t off;
  int W, top, left, h, w;
  bool flip, ok;
};
__device__ __forceinline__ Box box_of(const int64_t* __restrict__ meta, int b, int64_t src_bytes, int max_h) {
  const int64_t* m = meta + (int64_t)b * META;
  Box g;
  const int64_t H = clampl(m[1], 1, 1 << 20), W = clampl(m[2], 1, 1 << 20), bytes = H * W * 3;
  g.ok = bytes <= src_bytes;
  g.off = clampl(m[0], 0, g.ok ? src_bytes - bytes : 0);
  g.W = (int)W;
  g.h = (int)clampl(m[5], 1, H < max_h ? H : max_h);
  g.w = (int)clampl(m[6], 1, W);
  g.top = (int)clampl(m[3], 0, H - g.h);
  g.left = (int)clampl(m[4], 0, W - g.w);
  g.flip = m[7] != 0;
  return g;
}
// Row xx of image b's coefficient table on `axis` (0 horizontal, 1 vertical): {first tap relative to the crop, count, k[0..ktaps)}; first and
// count clamped into the crop extent `in` and the row's ktaps slots.
__device__ __forceinline__ const int* taps_of(const int* __restrict__ coef, int b, int axis, int xx, int S, int ktaps, int in, int& first, int& n) {
  const int* row = coef + (((int64_t)b * 2 + axis) * S + xx) * (2 + ktaps);
  first = row[0] < 0 ? 0 : (row[0] > in - 1 ? in - 1 : row[0]);
  const int room = in - first < ktaps ? in - first : ktaps;
  n = row[1] < 0 ? 0 : (row[1] > room ? room : row[1]);
  return row + 2;
}

// ---- horizontal pass: src (packed HWC images) -> tmp (B, max_h, 3, S) planar ------------------------------------------------------------
// Work item = one (crop row, output column) of one image, all three channels: the taps are 3 * n contiguous bytes of the interleaved source.
// blockIdx.x = image (geometry is workgroup-uniform: scalar loads), blockIdx.y strides over the image's h * S items.  Lanes of a wave hold
// consecutive output columns: their stores are consecutive bytes of a tmp row (reversed under the flip).
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ meta,
                                                         const int* __restrict__ coef, uint8_t* __restrict__ tmp, int S, int max_h, int ktaps) {
  const int b = blockIdx.x;
  const Box g = box_of(meta, b, src_bytes, max_h);
  if (!g.ok) return;
  const uint8_t* img = src + g.off + ((int64_t)g.top * g.W + g.left) * 3;   // pixel (0, 0) of the crop
  const uint32_t nitems = (uint32_t)g.h * (uint32_t)S;
  for (uint32_t it = blockIdx.y * 256u + threadIdx.x; it < nitems; it += gridDim.y * 256u) {
    const int y = (int)(it / (uint32_t)S), xx = (int)(it - (uint32_t)y * (uint32_t)S);
    int first, n;
    const int* k = taps_of(coef, b, 0, xx, S, ktaps, g.w, first, n);
    const uint8_t* p = img + ((int64_t)y * g.W + first) * 3;
    uint32_t a0 = 1u << (PRECISION_BITS - 1), a1 = a0, a2 = a0;   // unsigned: wraps like PIL's int32 would, never undefined
    for (int t = 0; t < n; ++t) {
      const uint32_t kt = (uint32_t)k[t];
      a0 += kt * p[3 * t];
      a1 += kt * p[3 * t + 1];
      a2 += kt * p[3 * t + 2];
    }
    uint8_t* o = tmp + ((int64_t)b * max_h + y) * 3 * S + (g.flip ? S - 1 - xx : xx);
    o[0] = (uint8_t)clip8(a0);
    o[S] = (uint8_t)clip8(a1);
    o[2 * S] = (uint8_t)clip8(a2);
  }
}

// ---- vertical pass: tmp -> dst (B, 1, 3, S, S) planar -------------------------------------------------------------------------------------
// Work item = four consecutive output pixels of one row of one channel plane: each tap is one aligned 32-bit load from a tmp row, the result
// one aligned 32-bit store (S % 4 == 0, tmp and dst 4-byte aligned: checked by the launcher).  blockIdx.x = image, blockIdx.y strides over the
// image's 3 * S * S / 4 items.
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ tmp, int64_t src_bytes, const int64_t* __restrict__ meta,
                                                         const int* __restrict__ coef, uint8_t* __restrict__ dst, int S, int max_h, int ktaps) {
  const int b = blockIdx.x;
  const Box g = box_of(meta, b, src_bytes, max_h);
  if (!g.ok) return;
  const uint32_t Q = (uint32_t)S / 4u, per_plane = (uint32_t)S * Q, nitems = 3u * per_plane;
  for (uint32_t it = blockIdx.y * 256u + threadIdx.x; it < nitems; it += gridDim.y * 256u) {
    const uint32_t c = it / per_plane, r = it - c * per_plane, yy = r / Q, q = r - yy * Q;
    int first, n;
    const int* k = taps_of(coef, b, 1, (int)yy, S, ktaps, g.h, first, n);
    const uint8_t* p = tmp + (((int64_t)b * max_h + first) * 3 + c) * S + 4 * q;
    uint32_t a0 = 1u << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int t = 0; t < n; ++t) {
      const uint32_t kt = (uint32_t)k[t], u = *(const uint32_t*)(p + (int64_t)t * 3 * S);
      a0 += kt * (u & 0xffu);
      a1 += kt * ((u >> 8) & 0xffu);
      a2 += kt * ((u >> 16) & 0xffu);
      a3 += kt * (u >> 24);
    }
    *(uint32_t*)(dst + (((int64_t)b * 3 + c) * S + yy) * S + 4 * q) = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
  }
}

bool overlap(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace
}  // namespace alpro

extern "C" int alpro_resized_crop(const uint8_t* src, int64_t src_bytes, const int64_t* meta, const int32_t* coef, uint8_t* tmp, uint8_t* dst, int B,
                                  int S, int max_h, int ktaps, void* stream) {
  using namespace alpro;
  ALPRO_CHECK(src && meta && coef && tmp && dst, "alpro_resized_crop: src, meta, coef, tmp and dst must not be NULL");
  ALPRO_CHECK(B > 0 && B < (1 << 30), "alpro_resized_crop: B %d must be positive", B);
  ALPRO_CHECK(src_bytes >= 3, "alpro_resized_crop: src_bytes %lld holds no pixel", (long long)src_bytes);
  ALPRO_CHECK(S >= 4 && S <= 32768 && S % 4 == 0, "alpro_resized_crop: output size %d must be a multiple of 4 in 4..32768 (the vertical pass stores whole words)", S);
  ALPRO_CHECK(max_h >= 1 && max_h <= 65536, "alpro_resized_crop: max_h %d outside 1..65536 (max_h * S items are counted in 32 bits)", max_h);
  ALPRO_CHECK(ktaps >= 1 && ktaps <= ALPRO_RESAMPLE_MAX_TAPS, "alpro_resized_crop: ktaps %d outside 1..%d (ALPRO_RESAMPLE_MAX_TAPS)", ktaps,
              ALPRO_RESAMPLE_MAX_TAPS);
  ALPRO_CHECK(((uintptr_t)meta & 7) == 0 && ((uintptr_t)coef & 3) == 0, "alpro_resized_crop: meta must be 8-byte and coef 4-byte aligned");
  ALPRO_CHECK(((uintptr_t)tmp & 3) == 0 && ((uintptr_t)dst & 3) == 0, "alpro_resized_crop: tmp and dst must be 4-byte aligned");
  const int64_t tmp_bytes = (int64_t)B * max_h * 3 * S, dst_bytes = (int64_t)B * 3 * S * S;
  ALPRO_CHECK(!overlap(dst, dst_bytes, src, src_bytes), "alpro_resized_crop: dst overlaps src");
  ALPRO_CHECK(!overlap(tmp, tmp_bytes, src, src_bytes) && !overlap(tmp, tmp_bytes, dst, dst_bytes), "alpro_resized_crop: tmp overlaps src or dst");
  const int64_t hb = ((int64_t)max_h * S + 255) / 256, vb = (3ll * S * S / 4 + 255) / 256;
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)B, (unsigned)(hb < 64 ? hb : 64)), dim3(256), 0, (hipStream_t)stream, src, src_bytes, meta,
                     coef, tmp, S, max_h, ktaps);
  if (int rc = check_launch("alpro_resized_crop (horizontal)")) return rc;
  hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)B, (unsigned)(vb < 64 ? vb : 64)), dim3(256), 0, (hipStream_t)stream, tmp, src_bytes, meta, coef,
                     dst, S, max_h, ktaps);
  return check_launch("alpro_resized_crop (vertical)");
}
