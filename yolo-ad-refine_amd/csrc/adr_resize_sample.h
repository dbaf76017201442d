// cv2.resize(INTER_LINEAR) of one 8-bit HWC 3-channel image, one output sample at a time: the arithmetic shared by
// adr_letterbox_u8 (csrc/adr_letterbox.hip) and adr_resize_u8 (csrc/adr_resize.hip). Both kernels take their taps
// and their samples from the two functions below and from nothing else, so they cannot disagree. Integer only.
// The algorithm (OpenCV 4.x imgproc/resize.cpp restated, PARITY UNPINNED) is described in adr_letterbox.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adr {

enum ResizeMode { RS_COPY = 0, RS_LINEAR = 1, RS_AREA2 = 2 };

// the source taps of output pixel (dx, dy): two source rows, two byte offsets of the left / right pixel in them, the
// horizontal (a) and vertical (b) coefficients
struct ResizeTaps {
  const uint8_t* r0;
  const uint8_t* r1;
  int o0, o1;
  int a0, a1, b0, b1;
};

__device__ __forceinline__ int rs_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// S: the source image (sw x sh, pitch sw * 3); (nw, nh): the output size; t: LINEAR: sx[nw], a0[nw], a1[nw], sy[nh],
// b0[nh], b1[nh]; 0 <= dx < nw, 0 <= dy < nh. Every index is clamped into the source, so that a wrong table or
// descriptor cannot read outside the image.
__device__ __forceinline__ ResizeTaps resize_taps(const uint8_t* S, int sw, int sh, int nw, int nh, int mode,
                                                  const int* t, int dx, int dy) {
  ResizeTaps p;
  const long pitch = (long)sw * 3;
  if (mode == RS_LINEAR) {
    const int sx0 = rs_clampi(t[dx], 0, sw - 1), sx1 = min(sx0 + 1, sw - 1);
    p.a0 = t[nw + dx];
    p.a1 = t[2 * nw + dx];
    const int* u = t + 3 * nw;
    const int sy0 = rs_clampi(u[dy], 0, sh - 1), sy1 = min(sy0 + 1, sh - 1);
    p.b0 = u[nh + dy];
    p.b1 = u[2 * nh + dy];
    p.r0 = S + sy0 * pitch;
    p.r1 = S + sy1 * pitch;
    p.o0 = sx0 * 3;
    p.o1 = sx1 * 3;
  } else if (mode == RS_AREA2) {
    const int sx = min(2 * dx, sw - 2), sy = min(2 * dy, sh - 2);
    p.r0 = S + sy * pitch;
    p.r1 = p.r0 + pitch;
    p.o0 = sx * 3;
    p.o1 = p.o0 + 3;
    p.a0 = p.a1 = p.b0 = p.b1 = 0;
  } else {
    p.r0 = p.r1 = S + min(dy, sh - 1) * pitch;
    p.o0 = p.o1 = min(dx, sw - 1) * 3;
    p.a0 = p.a1 = p.b0 = p.b1 = 0;
  }
  return p;
}

// channel k (0..2, BGR order of the source) of the output pixel whose taps are p
__device__ __forceinline__ int resize_sample(const ResizeTaps& p, int mode, int k) {
  if (mode == RS_LINEAR) {
    const int D0 = p.r0[p.o0 + k] * p.a0 + p.r0[p.o1 + k] * p.a1;
    const int D1 = p.r1[p.o0 + k] * p.a0 + p.r1[p.o1 + k] * p.a1;
    const int q = (((p.b0 * (D0 >> 4)) >> 16) + ((p.b1 * (D1 >> 4)) >> 16) + 2) >> 2;
    return rs_clampi(q, 0, 255);
  }
  if (mode == RS_AREA2) return (p.r0[p.o0 + k] + p.r0[p.o1 + k] + p.r1[p.o0 + k] + p.r1[p.o1 + k] + 2) >> 2;
  return p.r0[p.o0 + k];
}

}  // namespace adr
