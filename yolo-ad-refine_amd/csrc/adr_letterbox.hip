// LetterBox pixels in one launch (reference data/augment.py LetterBox :1475-1640, the predictor's pre_transform +
// preprocess engine/predictor.py:125, 144-156): for a batch of source images of different sizes,
//
//   cv2.resize(INTER_LINEAR) to the unpadded size (nw, nh)
//   -> cv2.copyMakeBorder(BORDER_CONSTANT, 114) to (H, W), the resized image at (left, top)
//   -> optional BGR -> RGB, HWC -> CHW
//
// written straight into the uint8 (B, 3, H, W) tensor the network reads; the resized and the padded images never
// exist. The resize is OpenCV's 8-bit INTER_LINEAR in fixed point (INTER_RESIZE_COEF_BITS 11): the host computes the
// per-column tables sx[nw], a0[nw], a1[nw] and the per-row tables sy[nh], b0[nh], b1[nh] exactly as OpenCV does
// (adrefine/data/augment.py resize_linear_tables) and the kernel is integer only:
//   horizontal  D = S[sx] * a0 + S[min(sx + 1, sw - 1)] * a1
//   vertical    dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
// and, when sw == 2 nw and sh == 2 nh, INTER_LINEAR's area fast path (s00 + s01 + s10 + s11 + 2) >> 2.
// OpenCV itself is not installed: this restatement from OpenCV 4.x's published algorithm is PARITY UNPINNED against
// real OpenCV (as warpAffine and cvtColor in adr_augment.hip are); parity is defined by the numpy restatement in
// tests/letterbox_util.py.
//
// One thread per 4 adjacent output x (one 32-bit store per plane, coalesced) when W % 4 == 0, one thread per output
// pixel otherwise. The source taps of neighbouring outputs are neighbouring source pixels (L2 / TA hits).
//
// adr_scale_boxes: ops.scale_boxes (utils/ops.py:88-123) + clip_boxes (:315-334) in place on the padded NMS output.
#include "adr_common.h"
#include "adr_resize_sample.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace adr {

enum LbMode { LB_COPY = RS_COPY, LB_LINEAR = RS_LINEAR, LB_AREA2 = RS_AREA2 };  // adr_resize_sample.h

struct LbDesc {
  long long off;   // byte offset of the source image (HWC BGR uint8) in the pool
  int sw, sh;      // source size
  int nw, nh;      // unpadded (resized) size; nw == 0: the whole image is 114 (empty slot of a batch)
  int left, top;   // where the resized image sits in the output
  int mode;        // LbMode
  int tab_off;     // LB_LINEAR: sx[nw], a0[nw], a1[nw], sy[nh], b0[nh], b1[nh] (ints) at tables + tab_off
  int rgb;         // 1: planes in R, G, B order
  int pad_;
};

namespace {

// one output pixel (x, y) of image d as BGR; the resize arithmetic is adr_resize_sample.h's, shared with adr_resize_u8
__device__ __forceinline__ void lb_pixel(const uint8_t* pool, const LbDesc& d, const int* tabs, int x, int y,
                                         int v[3]) {
  const int dx = x - d.left, dy = y - d.top;
  if (dx < 0 || dy < 0 || dx >= d.nw || dy >= d.nh) {
    v[0] = v[1] = v[2] = 114;
    return;
  }
  const ResizeTaps t = resize_taps(pool + d.off, d.sw, d.sh, d.nw, d.nh, d.mode, tabs + d.tab_off, dx, dy);
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = resize_sample(t, d.mode, k);
}

}  // namespace

// VEC = 4: thread = 4 adjacent x of one row (W % 4 == 0, out 4-byte aligned); VEC = 1: thread = one pixel
template <int VEC>
__global__ void __launch_bounds__(256) letterbox_u8_kernel(const uint8_t* pool, const LbDesc* descs, const int* tabs,
                                                            uint8_t* out, int H, int W) {
  const int b = blockIdx.y;
  const int p = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (p >= H * W) return;
  const LbDesc d = descs[b];
  const int y = p / W, x = p - y * W;
  const long plane = (long)H * W;
  uint8_t* o = out + (long)b * 3 * plane + p;
  if constexpr (VEC == 4) {
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int v[3];
      lb_pixel(pool, d, tabs, x + i, y, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) w[c] |= (uint32_t)v[d.rgb ? 2 - c : c] << (8 * i);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(o + c * plane) = w[c];
  } else {
    int v[3];
    lb_pixel(pool, d, tabs, x, y, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (uint8_t)v[d.rgb ? 2 - c : c];
  }
}

struct BoxRow {
  float gain, padx, pady, w0, h0;
};

// one thread per (image, row): x = (x - pad) / gain (IEEE fp32 division, as torch's `boxes /= gain`), clamped
__global__ void __launch_bounds__(256) scale_boxes_kernel(float* boxes, const int* counts, const BoxRow* tab, int B,
                                                           int rows, int cols, int xywh) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * rows) return;
  const int b = i / rows, r = i - b * rows;
  if (counts != nullptr && r >= counts[b]) return;
  const BoxRow t = tab[b];
  float* p = boxes + (long)i * cols;
  const float px[4] = {t.padx, t.pady, xywh ? 0.f : t.padx, xywh ? 0.f : t.pady};
  const float hi[4] = {t.w0, t.h0, t.w0, t.h0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float v = (p[k] - px[k]) / t.gain;
    p[k] = fminf(fmaxf(v, 0.f), hi[k]);
  }
}

}  // namespace adr

using namespace adr;

extern "C" int adr_letterbox_desc_size(void) { return (int)sizeof(LbDesc); }

extern "C" int adr_letterbox_u8(const void* pool, size_t pool_bytes, const void* descs, const void* descs_host, int B,
                                const int* tables, int ntab, void* out, int H, int W, void* stream) {
  ADR_REQUIRE(B > 0 && H > 0 && W > 0 && (long)H * W < (1l << 30), "letterbox: B=%d H=%d W=%d", B, H, W);
  ADR_REQUIRE(pool && descs && descs_host && tables && out && ntab >= 0, "letterbox: null argument");
  const LbDesc* hd = (const LbDesc*)descs_host;
  for (int b = 0; b < B; ++b) {
    const LbDesc& d = hd[b];
    if (d.nw == 0) continue;
    ADR_REQUIRE(d.sw > 0 && d.sh > 0 && d.nw > 0 && d.nh > 0 && d.left >= 0 && d.top >= 0,
                "letterbox: image %d sizes sw=%d sh=%d nw=%d nh=%d left=%d top=%d", b, d.sw, d.sh, d.nw, d.nh, d.left,
                d.top);
    ADR_REQUIRE(d.nw <= W - d.left && d.nh <= H - d.top, "letterbox: image %d (%d x %d at %d, %d) outside %d x %d", b,
                d.nw, d.nh, d.left, d.top, W, H);
    ADR_REQUIRE(d.off >= 0 && (size_t)d.off + (size_t)d.sw * d.sh * 3 <= pool_bytes,
                "letterbox: image %d source outside the pool", b);
    if (d.mode == LB_LINEAR)
      ADR_REQUIRE(d.tab_off >= 0 && (long)d.tab_off + 3l * (d.nw + d.nh) <= ntab, "letterbox: image %d tables", b);
    else if (d.mode == LB_AREA2)
      ADR_REQUIRE(d.sw == 2 * d.nw && d.sh == 2 * d.nh, "letterbox: image %d area path needs an exact 2x", b);
    else
      ADR_REQUIRE(d.mode == LB_COPY && d.sw == d.nw && d.sh == d.nh, "letterbox: image %d copy mode / size", b);
  }
  const long npx = (long)H * W;
  if (W % 4 == 0 && ((uintptr_t)out & 3) == 0)
    hipLaunchKernelGGL(letterbox_u8_kernel<4>, dim3(cdiv(npx / 4, 256), B), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)pool, (const LbDesc*)descs, tables, (uint8_t*)out, H, W);
  else
    hipLaunchKernelGGL(letterbox_u8_kernel<1>, dim3(cdiv(npx, 256), B), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)pool, (const LbDesc*)descs, tables, (uint8_t*)out, H, W);
  return check_launch("adr_letterbox_u8");
}

extern "C" int adr_scale_boxes(float* boxes, const int* counts, const float* table, int B, int rows, int cols, int xywh,
                               void* stream) {
  ADR_REQUIRE(boxes && table && B > 0 && rows >= 0 && cols >= 4 && (long)B * rows < (1l << 30),
              "scale_boxes: B=%d rows=%d cols=%d", B, rows, cols);
  if (rows == 0) return ADR_OK;
  hipLaunchKernelGGL(scale_boxes_kernel, dim3(cdiv((long)B * rows, 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                     counts, (const BoxRow*)table, B, rows, cols, xywh);
  return check_launch("adr_scale_boxes");
}
