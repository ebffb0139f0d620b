// Clip augmentation on the device: one op stage of TemporalConsistentRandomAugment (src/datasets/randaugment.py) over a whole batch per launch,
// with VideoRandomSquareCrop (src/datasets/data_utils.py:310-336) folded into the read side, and the per-frame statistics Contrast needs.
// uint8 in, uint8 out; every frame of a clip gets the clip's op, different clips of one launch may hold different ops.  Byte work with no reuse
// worth staging: no LDS in the stage kernel, 4-byte stores wherever four output pixels sit on an aligned word.  Measured times, and why four
// bytes per lane keep the pointwise stages below the HBM rate: DESIGN.md 4.11.
//
// No contraction anywhere in this file: the pointwise ops are DEFINED by their sequence of roundings (a multiply and an add fused into one
// rounding changes grey levels); where a fused multiply-add is meant, fmaf() says so.  The __f*_rn / __d*_rn intrinsics name the rounding at
// each site; on this toolchain they are plain operators inside inline functions, so it is the pragma that binds the compiler.
#pragma clang fp contract(off)
#include "common.hpp"

namespace alpro {
namespace {

constexpr int AUG_FILL = 128;  // replace_value of randaugment.py:299, every channel

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// reflect-101 (cv2.BORDER_DEFAULT): -1 -> 1, n -> n-2; always inside [0, n-1], also for n == 1 and for indices further out
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return clampi(i, 0, n - 1);
}
// n (1..4) consecutive bytes at p, byte k in bits 8k.  Never touches a byte outside [p, p + n).  The 4- and 2-byte forms go through memcpy: p
// has no alignment (a crop window starts at any column), and the compiler turns the copy into one load where the target allows unaligned
// global access (gfx950 under HSA does) and into byte loads where it does not -- correct either way.
__device__ __forceinline__ uint32_t load_span(const uint8_t* p, int n) {
  uint32_t u = 0;
  if (n == 4) __builtin_memcpy(&u, p, 4);
  else for (int k = 0; k < n; ++k) u |= (uint32_t)p[k] << (8 * k);
  return u;
}
__device__ __forceinline__ uint32_t load_pair(const uint8_t* p) {
  uint16_t u;
  __builtin_memcpy(&u, p, 2);
  return u;
}
__device__ __forceinline__ uint32_t trunc_u8(float v) { return (uint32_t)fminf(fmaxf(v, 0.f), 255.f); }

// The crop window of clip b inside its (Hs, Ws) frames.  Offsets come from device memory: clamped here, so that no value there can move a read
// outside the frame (the Python wrapper refuses such offsets with a message; this is the bound itself).
__device__ __forceinline__ void crop_of(const int* __restrict__ crop, int b, int Hs, int Ws, int Hc, int Wc, int& top, int& left) {
  top = left = 0;
  if (crop) {
    top = clampi(crop[2 * b], 0, Hs - Hc);
    left = clampi(crop[2 * b + 1], 0, Ws - Wc);
  }
}

// ---- one op stage ---------------------------------------------------------------------------------------------------------------------
// Work item = up to four consecutive pixels of one row of one (frame, channel) plane of dst, placed so that a full item is one ALIGNED 32-bit
// word of dst: a row that does not start on a word boundary (Wc % 4 != 0) begins with a 1-3 pixel item, and rows end with one; those are stored
// byte by byte.  G items per row.  blockIdx.x = plane (frame * 3 + channel): clip, op, arguments and crop window are workgroup-uniform -- scalar
// loads, a uniform branch on the op, one integer division per item; blockIdx.y strides over the plane's Hc * G items.
__global__ __launch_bounds__(256) void augment_stage_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int* __restrict__ crop,
                                                            const int* __restrict__ ops, const double* __restrict__ args,
                                                            const uint8_t* __restrict__ tables, int T, int Hs, int Ws, int Hc, int Wc, uint32_t G) {
  const int64_t plane_s = (int64_t)Hs * Ws;
  const uint32_t pc = blockIdx.x, bt = pc / 3u, nitems = (uint32_t)Hc * G;
  const int c = (int)(pc - 3u * bt), b = (int)(bt / (uint32_t)T);
  const int op = ops[b];
  const double a0 = args[2 * b], a1 = args[2 * b + 1];
  int top, left;
  crop_of(crop, b, Hs, Ws, Hc, Wc, top, left);
  const uint8_t* frame = src + (int64_t)bt * 3 * plane_s + (int64_t)top * Ws + left;   // pixel (0, 0) of the window, channel 0
  const uint8_t* plane = frame + c * plane_s;
  for (uint32_t base = blockIdx.y * 256u; base < nitems; base += gridDim.y * 256u) {   // base is workgroup-uniform: every lane stays in the loop
    const uint32_t it = base + threadIdx.x;
    bool active = it < nitems;
    const uint32_t yy = active ? it / G : 0u, g = active ? it - yy * G : 0u;
    const int y = (int)yy;
    const int64_t row = (int64_t)pc * Hc + y;
    uint8_t* drow = dst + row * Wc;
    const int head = (int)((4 - ((uintptr_t)drow & 3)) & 3);
    const int start = (head ? head - 4 : 0) + 4 * (int)g;
    const int x0 = start < 0 ? 0 : start;
    const int n = (start + 4 < Wc ? start + 4 : Wc) - x0;   // pixels of this item
    active = active && n > 0;
    const uint8_t* prow = plane + (int64_t)y * Ws;
    uint32_t out = 0;   // pixel x0 + k in bits 8k

    if (op >= ALPRO_AUG_TRANSLATE_X && op <= ALPRO_AUG_ROTATE) {
      // dst(x, y) = src(sx, sy), (sx, sy) affine in (x, y), fp32; four taps, a tap outside the window holds the fill.  Coordinates are taken
      // relative to (ox, oy) -- the rotation centre, 0 otherwise -- so that the products stay small.
      float m00 = 1.f, m01 = 0.f, m10 = 0.f, m11 = 1.f, ox = 0.f, oy = 0.f, tx = 0.f, ty = 0.f;
      const float f0 = (float)a0, f1 = (float)a1;
      if (op == ALPRO_AUG_TRANSLATE_X) tx = f0;
      else if (op == ALPRO_AUG_TRANSLATE_Y) ty = f0;
      else if (op == ALPRO_AUG_SHEAR_X) m01 = -f0;
      else if (op == ALPRO_AUG_SHEAR_Y) m10 = -f0;
      else {   // inverse of [[a, b, (1-a)cx - b cy], [-b, a, b cx + (1-a)cy]], a = cos d = a0, b = sin d = a1: (sx, sy) = c + [[a, -b], [b, a]] (p - c)
        m00 = f0; m01 = -f1; m10 = f1; m11 = f0;
        ox = tx = 0.5f * (float)Wc;
        oy = ty = 0.5f * (float)Hc;
      }
      const float yr = (float)y - oy;
      const float rx = fmaf(m01, yr, tx), ry = fmaf(m11, yr, ty);   // constant along the row
      float sx[4], sy[4];
      int ix[4], iy[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xr = (float)(x0 + k) - ox;
        // the clamp keeps the integer parts representable whatever the argument arrays hold; it is far outside the window plus one tap
        sx[k] = fminf(fmaxf(fmaf(m00, xr, rx), -4.f), (float)Wc + 4.f);
        sy[k] = fminf(fmaxf(fmaf(m10, xr, ry), -4.f), (float)Hc + 4.f);
        const float flx = floorf(sx[k]), fly = floorf(sy[k]);
        ix[k] = (int)flx; iy[k] = (int)fly;
        sx[k] -= flx; sy[k] -= fly;   // the weights of the right / lower taps
      }
      // sx and sy are monotone along a row (one correctly rounded fma of x each, clamped), so the end pixels bound the middle ones: when both
      // ends have all four taps inside the window, so has every pixel of the item.  Decided per wave: only waves that touch the border of the
      // source take the path with the fill selects.
      const bool inside = !active || (min(ix[0], ix[3]) >= 0 && max(ix[0], ix[3]) <= Wc - 2 && min(iy[0], iy[3]) >= 0 && max(iy[0], iy[3]) <= Hc - 2);
      if (__builtin_amdgcn_ballot_w64(!inside) == 0) {
        if (active) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint8_t* p = plane + (int64_t)iy[k] * Ws + ix[k];
            const uint32_t pa = load_pair(p), pb = load_pair(p + Ws);   // taps (ix, ix + 1) of the two rows
            const float v00 = (float)(pa & 0xffu), v01 = (float)(pa >> 8), v10 = (float)(pb & 0xffu), v11 = (float)(pb >> 8);
            const float t = fmaf(sx[k], v01 - v00, v00), u = fmaf(sx[k], v11 - v10, v10);
            out |= min((uint32_t)(fmaf(sy[k], u - t, t) + 0.5f), 255u) << (8 * k);
          }
        }
      } else if (active) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int xa = clampi(ix[k], 0, Wc - 1), xb = clampi(ix[k] + 1, 0, Wc - 1), ya = clampi(iy[k], 0, Hc - 1), yb = clampi(iy[k] + 1, 0, Hc - 1);
          const bool xa_in = ix[k] >= 0 && ix[k] < Wc, xb_in = ix[k] + 1 >= 0 && ix[k] + 1 < Wc;
          const bool ya_in = iy[k] >= 0 && iy[k] < Hc, yb_in = iy[k] + 1 >= 0 && iy[k] + 1 < Hc;
          const uint8_t *pa = plane + (int64_t)ya * Ws, *pb = plane + (int64_t)yb * Ws;   // clamped addresses: always inside the window
          const uint8_t r00 = pa[xa], r01 = pa[xb], r10 = pb[xa], r11 = pb[xb];
          const float v00 = (xa_in && ya_in) ? (float)r00 : (float)AUG_FILL, v01 = (xb_in && ya_in) ? (float)r01 : (float)AUG_FILL;
          const float v10 = (xa_in && yb_in) ? (float)r10 : (float)AUG_FILL, v11 = (xb_in && yb_in) ? (float)r11 : (float)AUG_FILL;
          const float t = fmaf(sx[k], v01 - v00, v00), u = fmaf(sx[k], v11 - v10, v10);
          out |= min((uint32_t)(fmaf(sy[k], u - t, t) + 0.5f), 255u) << (8 * k);
        }
      }
    } else if (active) {
      switch (op) {
        case ALPRO_AUG_HFLIP: {
          const uint32_t u = load_span(prow + (Wc - x0 - n), n);   // source pixels Wc-1-(x0+n-1) .. Wc-1-x0
          for (int k = 0; k < n; ++k) out |= ((u >> (8 * (n - 1 - k))) & 0xffu) << (8 * k);
          break;
        }
        case ALPRO_AUG_BRIGHTNESS: {
          const uint32_t u = load_span(prow + x0, n);
          const float f = (float)a0;
#pragma unroll
          for (int k = 0; k < 4; ++k) out |= trunc_u8(__fmul_rn((float)((u >> (8 * k)) & 0xffu), f)) << (8 * k);
          break;
        }
        case ALPRO_AUG_CONTRAST: {
          const uint32_t u = load_span(prow + x0, n);
          const uint8_t* tb = tables + (int64_t)bt * 256;
#pragma unroll
          for (int k = 0; k < 4; ++k) out |= (uint32_t)tb[(u >> (8 * k)) & 0xffu] << (8 * k);
          break;
        }
        case ALPRO_AUG_SOLARIZE: {
          const uint32_t u = load_span(prow + x0, n), t = (uint32_t)clampi((int)a0, 0, 256);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t el = (u >> (8 * k)) & 0xffu;
            out |= (el < t ? el : 255u - el) << (8 * k);
          }
          break;
        }
        case ALPRO_AUG_POSTERIZE: {
          const uint32_t m = (255u << (8 - clampi((int)a0, 0, 8))) & 255u;
          out = load_span(prow + x0, n) & (m * 0x01010101u);
          break;
        }
        case ALPRO_AUG_COLOR: {
          // out_c = sum_i img_i * (A[i][c] * f + w[i]), A = I - w 1^T with the reference's weights on channels 0, 1, 2 in stored order
          const float f = (float)a0;
          const float w[3] = {0.114f, 0.587f, 0.299f};
          const float A[3][3] = {{0.886f, -0.114f, -0.114f}, {-0.587f, 0.413f, -0.587f}, {-0.299f, -0.299f, 0.701f}};
          const float m0 = __fadd_rn(__fmul_rn(A[0][c], f), w[0]), m1 = __fadd_rn(__fmul_rn(A[1][c], f), w[1]), m2 = __fadd_rn(__fmul_rn(A[2][c], f), w[2]);
          const int64_t o = (int64_t)y * Ws + x0;
          const uint32_t u0 = load_span(frame + o, n), u1 = load_span(frame + plane_s + o, n), u2 = load_span(frame + 2 * plane_s + o, n);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float v = fmaf((float)((u2 >> (8 * k)) & 0xffu), m2, fmaf((float)((u1 >> (8 * k)) & 0xffu), m1, (float)((u0 >> (8 * k)) & 0xffu) * m0));
            out |= trunc_u8(v) << (8 * k);
          }
          break;
        }
        case ALPRO_AUG_SHARPNESS: {
          if (a0 == 1.0) { out = load_span(prow + x0, n); break; }
          // deg = round(S / 13), S = sum of the 3x3 neighbourhood + 4 * centre (never a tie: 13 is odd) -> (2S + 13) / 26 in integers
          int xi[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) xi[j] = reflect101(x0 - 1 + j, Wc);
          const uint8_t* rp[3] = {plane + (int64_t)reflect101(y - 1, Hc) * Ws, prow, plane + (int64_t)reflect101(y + 1, Hc) * Ws};
          uint32_t colsum[6], mid[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            mid[j] = rp[1][xi[j]];
            colsum[j] = (uint32_t)rp[0][xi[j]] + mid[j] + (uint32_t)rp[2][xi[j]];
          }
          const float f = (float)a0;
          const bool row_in = y >= 1 && y <= Hc - 2;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t S = colsum[k] + colsum[k + 1] + colsum[k + 2] + 4u * mid[k + 1], deg = (2u * S + 13u) / 26u, s = mid[k + 1];
            uint32_t r = s;   // the one-pixel frame keeps src
            if (a0 == 0.0) r = deg;
            else if (row_in && x0 + k >= 1 && x0 + k <= Wc - 2)
              r = trunc_u8(__fadd_rn((float)deg, __fmul_rn(f, __fsub_rn((float)s, (float)deg))));   // out of 0..255 only for f > 1: clamped
            out |= r << (8 * k);
          }
          break;
        }
        default:   // ALPRO_AUG_IDENTITY, -1 (the draw skipped the op) and any code this library does not know: copy
          out = load_span(prow + x0, n);
      }
    }
    if (active) {
      if (n == 4) *(uint32_t*)(drow + x0) = out;   // aligned by construction of the items
      else for (int k = 0; k < n; ++k) drow[x0 + k] = (uint8_t)(out >> (8 * k));
    }
  }
}

// ---- per-frame statistics: exact channel sums and the Contrast table ---------------------------------------------------------------------
// One workgroup of 16 waves per frame; frames of clips whose op is not Contrast return at once.  Integer sums: exact, so the fixed order (lane
// partials, xor-shuffle tree, waves 0..15 added in order) makes them reproducible by construction rather than by luck; no atomics.  Then thread
// el < 256 forms table[el] = trunc(clip((el - mean) * f + mean)) in fp64, mean = (m0 * 0.114 + m1 * 0.587) + m2 * 0.299, m_c = sum_c / (Hc * Wc).
constexpr int STATS_THREADS = 1024, STATS_WAVES = STATS_THREADS / 64;
__global__ __launch_bounds__(STATS_THREADS) void augment_stats_kernel(const uint8_t* __restrict__ src, const int* __restrict__ crop,
                                                                      const int* __restrict__ ops, const double* __restrict__ args,
                                                                      unsigned long long* __restrict__ sums, uint8_t* __restrict__ tables, int T, int Hs,
                                                                      int Ws, int Hc, int Wc) {
  const int bt = blockIdx.x, b = bt / T;
  if (ops[b] != ALPRO_AUG_CONTRAST) return;   // workgroup-uniform
  __shared__ unsigned long long part[3][STATS_WAVES];
  int top, left;
  crop_of(crop, b, Hs, Ws, Hc, Wc, top, left);
  const int64_t plane_s = (int64_t)Hs * Ws;
  const uint8_t* frame = src + (int64_t)bt * 3 * plane_s + (int64_t)top * Ws + left;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t Q = (uint32_t)(Wc + 3) / 4, nitems = (uint32_t)Hc * Q;   // items of up to four pixels, Q per row
  for (int c = 0; c < 3; ++c) {
    unsigned long long acc = 0;
    for (uint32_t it = threadIdx.x; it < nitems; it += STATS_THREADS) {
      const uint32_t y = it / Q, q = it - y * Q;
      const int n = Wc - 4 * (int)q < 4 ? Wc - 4 * (int)q : 4;
      const uint32_t u = load_span(frame + c * plane_s + (int64_t)y * Ws + 4 * q, n);
      acc += (u & 0xffu) + ((u >> 8) & 0xffu) + ((u >> 16) & 0xffu) + (u >> 24);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)acc, o, 64), hi = __shfl_xor((uint32_t)(acc >> 32), o, 64);
      acc += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) part[c][wave] = acc;
  }
  __syncthreads();
  if (threadIdx.x >= 256) return;
  unsigned long long tot[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    tot[c] = 0;
#pragma unroll
    for (int w = 0; w < STATS_WAVES; ++w) tot[c] += part[c][w];
  }
  if (threadIdx.x < 3) sums[(int64_t)bt * 3 + threadIdx.x] = threadIdx.x == 0 ? tot[0] : (threadIdx.x == 1 ? tot[1] : tot[2]);
  const double npix = (double)((int64_t)Hc * Wc), f = args[2 * b];
  const double m0 = (double)tot[0] / npix, m1 = (double)tot[1] / npix, m2 = (double)tot[2] / npix;
  const double mean = __dadd_rn(__dadd_rn(__dmul_rn(m0, 0.114), __dmul_rn(m1, 0.587)), __dmul_rn(m2, 0.299));
  const double v = __dadd_rn(__dmul_rn(__dsub_rn((double)threadIdx.x, mean), f), mean);
  tables[(int64_t)bt * 256 + threadIdx.x] = (uint8_t)fmin(fmax(v, 0.0), 255.0);
}

int check_shapes(const char* who, const void* src, int B, int T, int Hs, int Ws, int Hc, int Wc) {
  ALPRO_CHECK(src, "%s: src is NULL", who);
  ALPRO_CHECK(B > 0 && T > 0, "%s: B %d and T %d must be positive", who, B, T);
  ALPRO_CHECK(Hs >= 1 && Ws >= 1 && Hs <= 32768 && Ws <= 32768, "%s: frame %d x %d outside 1..32768 (fp32 coordinates are exact up to there)", who, Hs, Ws);
  ALPRO_CHECK(Hc >= 1 && Hc <= Hs, "%s: crop height %d does not fit the frame height %d", who, Hc, Hs);
  ALPRO_CHECK(Wc >= 1 && Wc <= Ws, "%s: crop width %d does not fit the frame width %d", who, Wc, Ws);
  return ALPRO_OK;
}

}  // namespace
}  // namespace alpro

extern "C" int alpro_augment_stage(const uint8_t* src, uint8_t* dst, const int32_t* crop_offsets, const int32_t* ops, const double* args,
                                   const uint8_t* tables, int B, int T, int Hs, int Ws, int Hc, int Wc, void* stream) {
  using namespace alpro;
  if (int rc = check_shapes("alpro_augment_stage", src, B, T, Hs, Ws, Hc, Wc)) return rc;
  ALPRO_CHECK(dst && ops && args && tables, "alpro_augment_stage: dst, ops, args and tables must not be NULL");
  ALPRO_CHECK(crop_offsets || (Hc == Hs && Wc == Ws), "alpro_augment_stage: output %d x %d differs from the frame %d x %d but there are no crop offsets", Hc, Wc,
              Hs, Ws);
  const int64_t src_bytes = (int64_t)B * T * 3 * Hs * Ws, dst_bytes = (int64_t)B * T * 3 * Hc * Wc;
  ALPRO_CHECK(dst + dst_bytes <= src || src + src_bytes <= dst, "alpro_augment_stage: dst overlaps src (a stage reads neighbours of the pixel it writes)");
  const bool whole_words = Wc % 4 == 0 && ((uintptr_t)dst & 3) == 0;   // every row starts on a word: no head items
  const int64_t G = whole_words ? Wc / 4 : (Wc + 3) / 4 + 1, planes = (int64_t)B * T * 3, blocks = ((int64_t)Hc * G + 255) / 256;
  ALPRO_CHECK(planes < (1ll << 31), "alpro_augment_stage: %lld planes (B %d, T %d) exceed 2^31 - 1", (long long)planes, B, T);
  hipLaunchKernelGGL(augment_stage_kernel, dim3((unsigned)planes, (unsigned)(blocks < 64 ? blocks : 64)), dim3(256), 0, (hipStream_t)stream, src, dst,
                     crop_offsets, ops, args, tables, T, Hs, Ws, Hc, Wc, (uint32_t)G);
  return check_launch("alpro_augment_stage");
}

extern "C" int alpro_augment_stats(const uint8_t* src, const int32_t* crop_offsets, const int32_t* ops, const double* args, uint64_t* sums,
                                   uint8_t* tables, int B, int T, int Hs, int Ws, int Hc, int Wc, void* stream) {
  using namespace alpro;
  if (int rc = check_shapes("alpro_augment_stats", src, B, T, Hs, Ws, Hc, Wc)) return rc;
  ALPRO_CHECK(ops && args && sums && tables, "alpro_augment_stats: ops, args, sums and tables must not be NULL");
  ALPRO_CHECK(crop_offsets || (Hc == Hs && Wc == Ws), "alpro_augment_stats: window %d x %d differs from the frame %d x %d but there are no crop offsets", Hc, Wc,
              Hs, Ws);
  ALPRO_CHECK(((uintptr_t)sums & 7) == 0, "alpro_augment_stats: sums must be 8-byte aligned");
  ALPRO_CHECK((int64_t)B * T < (1ll << 31), "alpro_augment_stats: %lld frames (B %d, T %d) exceed 2^31 - 1", (long long)B * T, B, T);
  hipLaunchKernelGGL(augment_stats_kernel, dim3((unsigned)(B * T)), dim3(STATS_THREADS), 0, (hipStream_t)stream, src, crop_offsets, ops, args, (unsigned long long*)sums,
                     tables, T, Hs, Ws, Hc, Wc);
  return check_launch("alpro_augment_stats");
}
