// Multi-scale training's resample (reference models/yolo/detect/train.py:57-74, DetectionTrainer.preprocess_batch
// with multi_scale): the dataloader's uint8 batch -> the resized fp32 batch the network reads, in one launch:
//
//   F.interpolate(img.float() / 255, size=(oh, ow), mode="bilinear", align_corners=False)
//
// The reference writes the fp32 image at the source size first (315 MB at bs 64, 640^2) and reads it back; here the
// source is read as bytes and only the resized fp32 batch is written. The arithmetic is ATen's (UpSample.h
// area_pixel_compute_scale / area_pixel_compute_source_index, UpSampleKernel.cpp's two-level linear interpolate), in
// fp32 without contraction, the same restatement adr_tta.hip samples its views with:
//   v = (float)u8 * fp32(1/255)       (torch's device division by a scalar; adr_stem.hip img_val)
//   scale = (float)in / (float)out;  src = max(scale * (dst + 0.5f) - 0.5f, 0)
//   i0 = min((int)src, in - 1);  i1 = min(i0 + 1, in - 1);  l1 = src - i0;  l0 = 1 - l1
//   out = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)
//
// Work mapping. The kernel is store-bound (4 output bytes per pixel against at most 4 one-byte taps that mostly hit
// the L1), so it is shaped around the stores: a wave owns one output row of one plane — its row taps and weights are
// wave-uniform — and a lane owns one 16-byte-aligned group of 4 consecutive output columns, written with one 16-byte
// store; a wave writes 1 KiB contiguous. A row starts at element (plane * oh + y) * ow of the output, which is
// 16-byte aligned only when ow % 4 == 0 (and the buffer is): the columns are therefore grouped from the row's first
// aligned element — lane slot s owns columns [head - 4 + 4 s, head + 4 s) with head = the 0-3 elements before that
// boundary — and the slots that stick out of the row on the left (the head) or on the right (the tail) store their
// inside columns one by one. Plain loads, vector stores, no LDS. The grid is flat over (plane, row block, slot
// block), and the host splits the planes over several launches where one grid could not index them: any B.
#include "adr_common.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace adr {

namespace {

constexpr int MS_ROWS = 4;  // rows (= waves) per block

// ATen's source indices and weights of one output index (align_corners=False, no scale_factor)
__device__ __forceinline__ void ms_tap(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

__device__ __forceinline__ float ms_px(const uint8_t* p) { return (float)*p * (1.f / 255.f); }

}  // namespace

// img: `planes` uint8 planes of H x W; out: the same planes at oh x ow, fp32. mis: (out address / 4) % 4, the
// position of out[0] inside its 16-byte group. grid.x = planes * yblocks * xblocks.
__global__ void __launch_bounds__(256) multiscale_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ out,
                                                             int H, int W, int oh, int ow, float scale_h,
                                                             float scale_w, int mis, int xblocks, int yblocks) {
  const unsigned bid = blockIdx.x;
  const int xb = (int)(bid % (unsigned)xblocks);
  const unsigned t = bid / (unsigned)xblocks;
  const int yb = (int)(t % (unsigned)yblocks);
  const long plane = (long)(t / (unsigned)yblocks);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int y = yb * MS_ROWS + wave;
  if (y >= oh) return;
  const long row = (plane * oh + y) * (long)ow;  // first element of this output row
  const int head = (int)((4 - ((row + mis) & 3)) & 3);
  const int xs = head - 4 + 4 * (xb * 64 + (int)(threadIdx.x & 63));
  if (xs >= ow || xs + 4 <= 0) return;
  int y0, y1;
  float l0y, l1y;
  ms_tap(y, H, scale_h, y0, y1, l0y, l1y);
  const uint8_t* s = img + plane * ((long)H * W);
  const uint8_t* row0 = s + (long)y0 * W;
  const uint8_t* row1 = s + (long)y1 * W;
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x = min(max(xs + i, 0), ow - 1);  // a column outside the row is computed at the edge and not stored
    int x0, x1;
    float l0x, l1x;
    ms_tap(x, W, scale_w, x0, x1, l0x, l1x);
    const float a = ms_px(row0 + x0), b = ms_px(row0 + x1);
    const float c = ms_px(row1 + x0), d = ms_px(row1 + x1);
    r[i] = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d);
  }
  float* o = out + row;
  if (xs >= 0 && xs + 4 <= ow) {
    *reinterpret_cast<f32x4*>(o + xs) = r;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (xs + i >= 0 && xs + i < ow) o[xs + i] = r[i];
  }
}

}  // namespace adr

using namespace adr;

extern "C" int adr_multiscale_u8(const uint8_t* img, int B, int H, int W, float* out, int oh, int ow, void* stream) {
  ADR_REQUIRE(img && out, "multiscale_u8: null argument");
  ADR_REQUIRE(B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0, "multiscale_u8: B=%d H=%d W=%d oh=%d ow=%d", B, H, W, oh,
              ow);
  ADR_REQUIRE(((uintptr_t)out & 3) == 0, "multiscale_u8: out must be 4-byte aligned");
  // slots of a row: the aligned groups of 4 that overlap it, at most one more than ceil(ow / 4) (a head and a tail)
  const long xblocks = ((long)ow / 4 + 2 + 63) / 64;
  const long yblocks = ((long)oh + MS_ROWS - 1) / MS_ROWS;
  const long per_plane = xblocks * yblocks;
  const long grid_max = (1l << 31) - 1;
  ADR_REQUIRE(per_plane <= grid_max, "multiscale_u8: oh=%d ow=%d is beyond one launch grid", oh, ow);
  const float scale_h = (float)H / (float)oh, scale_w = (float)W / (float)ow;
  const long planes = 3l * B, step = grid_max / per_plane;
  for (long p0 = 0; p0 < planes; p0 += step) {
    const long np = planes - p0 < step ? planes - p0 : step;
    const uint8_t* src = img + p0 * ((long)H * W);
    float* dst = out + p0 * ((long)oh * ow);
    hipLaunchKernelGGL(multiscale_u8_kernel, dim3((unsigned)(np * per_plane)), dim3(64 * MS_ROWS), 0,
                       (hipStream_t)stream, src, dst, H, W, oh, ow, scale_h, scale_w,
                       (int)(((uintptr_t)dst >> 2) & 3), (int)xblocks, (int)yblocks);
  }
  return check_launch("adr_multiscale_u8");
}
