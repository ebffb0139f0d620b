// alpro_unpatchify: the inverse data movement of alpro_patchify (core.hip) -- the (BT*N, C*256) rows of the stride-16 conv's im2col back into
// a (BT, C, H, W) fp32 image.  It ends the pixel gradient: drows @ W of the patch embedding lands here (vit.py _embed_backward).
// Pure movement: every image element is written once, as the widened value of one source element.  No arithmetic, no atomics, no LDS.
#include "common.hpp"

namespace alpro {
namespace {

// Threads walk the IMAGE, not the rows: unit u is the u-th piece of Chunk<T>::N consecutive pixels of the image in memory order, so neighbouring
// lanes store neighbouring pieces (fp32 rows: lane l's 16 bytes follow lane l-1's, one wave instruction = 1 KiB of consecutive image bytes;
// 16-bit rows: a lane's 16-byte source chunk is 8 pixels = two 16-byte stores, its 32 bytes follow lane l-1's, and the two stores of a wave fill
// the same 2 KiB back to back).  The gather is on the read side, where a patch row is 16 pixels = 64 (32) consecutive bytes of one source row:
// 4 (2) neighbouring lanes read one such run, the next run is the neighbouring patch's, C*256 elements further on.
template <typename T>
__global__ __launch_bounds__(256) void unpatchify_kernel(const T* __restrict__ rows, float* __restrict__ img, int BT, int C, int H, int W) {
  constexpr int E = Chunk<T>::N;   // pixels per 16-byte source chunk: 4 or 8, both divide the 16-pixel patch row
  const int gw = W / 16, N = (H / 16) * gw, K = C * 256;
  const int upr = W / E;           // units per image row
  const int64_t total = (int64_t)BT * C * H * upr;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t line = u / upr;                          // (bt*C + c)*H + y
    const int x = (int)(u - line * upr) * E;
    const int64_t plane = line / H;                        // bt*C + c
    const int y = (int)(line - plane * H);
    const int bt = (int)(plane / C), c = (int)(plane - (int64_t)bt * C);
    const int64_t row = (int64_t)bt * N + (y >> 4) * gw + (x >> 4);
    const u32x4 chunk = *(const u32x4*)(rows + row * K + c * 256 + (y & 15) * 16 + (x & 15));
    float v[E];
    unpack_chunk<T>(chunk, v);
    float* dst = img + line * W + x;
#pragma unroll
    for (int e = 0; e < E; e += 4) *(f32x4*)(dst + e) = f32x4{v[e], v[e + 1], v[e + 2], v[e + 3]};
  }
}

inline int grid_for(int64_t work_items, int per_block, int cap) {
  int64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

}  // namespace
}  // namespace alpro

using namespace alpro;

extern "C" int alpro_unpatchify(const void* rows, int dtype, float* img, int BT, int C, int Himg, int Wimg, void* stream) {
  // every check in front of the first HIP call: the refusals are testable without a device
  ALPRO_CHECK(dtype == ALPRO_F32 || dtype == ALPRO_BF16 || dtype == ALPRO_F16, "alpro_unpatchify: dtype=%d (ALPRO_F32, ALPRO_BF16 or ALPRO_F16)", dtype);
  ALPRO_CHECK(rows != nullptr, "alpro_unpatchify: null rows");
  ALPRO_CHECK(img != nullptr, "alpro_unpatchify: null img");
  ALPRO_CHECK(BT > 0 && C > 0, "alpro_unpatchify: BT=%d C=%d (need >= 1)", BT, C);
  ALPRO_CHECK(Himg > 0 && Wimg > 0 && Himg % 16 == 0 && Wimg % 16 == 0, "alpro_unpatchify: image %dx%d not a multiple of the 16x16 patch", Himg, Wimg);
  ALPRO_CHECK((int64_t)C * 256 <= INT32_MAX && (int64_t)BT * (Himg / 16) * (Wimg / 16) <= INT32_MAX, "alpro_unpatchify: BT=%d C=%d image %dx%d: more than 2^31 - 1 rows or columns", BT, C, Himg, Wimg);
  ALPRO_CHECK(((uintptr_t)rows % 16) == 0 && ((uintptr_t)img % 16) == 0, "alpro_unpatchify: rows and img must be 16-byte aligned");
  const int64_t pixels = (int64_t)BT * C * Himg * Wimg;
  ALPRO_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(unpatchify_kernel<T>, dim3(grid_for(pixels / Chunk<T>::N, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream, (const T*)rows, img, BT, C, Himg, Wimg));
  return check_launch("alpro_unpatchify");
}
