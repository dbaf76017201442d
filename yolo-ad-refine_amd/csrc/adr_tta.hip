// Test-time augmentation around the eval forward (reference nn/tasks.py DetectionModel._predict_augment :357-372):
// the scaled / flipped image views before the three forwards, and the merge of the three decoded outputs after them.
//
// adr_tta_views: scale_img (utils/torch_utils.py:439-448) of the optionally left-right flipped batch for every
// non-identity view in one launch:
//   F.interpolate(x.flip(3) or x, size=(int(H*s), int(W*s)), mode="bilinear", align_corners=False)
//   -> F.pad(right, bottom, value=0.447) to the multiple of the stride
// written as the fp32 NCHW batch the network reads. The interpolation is ATen's (UpSample.h
// area_pixel_compute_scale / area_pixel_compute_source_index, UpSampleKernel.cpp compute_source_index_and_lambda and
// the two-level linear interpolate), in fp32 without contraction:
//   scale = (float)in / out;  src = max(scale * (dst + 0.5f) - 0.5f, 0);  i0 = (int)src;  i1 = i0 + (i0 < in - 1)
//   l1 = src - i0;  l0 = 1 - l1;  out = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)
// The flip is a source column index W - 1 - x: no flipped copy of the batch exists. A uint8 source is divided by 255
// in fp32 first (the predictor's preprocess, engine/predictor.py:130-141), as a multiplication by fp32(1/255).
// One thread per 4 adjacent output x of one row for the three planes (the padded width is a multiple of 4: one
// 16-byte store per plane); the row taps and weights are computed once per thread, the column taps once per pixel.
//
// adr_tta_merge: _descale_pred (:374-383) + _clip_augmented (:385-394) + torch.cat(y, -1) (:372) in one launch.
#include "adr_common.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace adr {

struct TtaView {
  long long out_off;  // element offset of this view's (B, 3, ph, pw) fp32 batch in the output buffer
  int rh, rw;         // resized size (int(H * s), int(W * s))
  int ph, pw;         // padded size
  int flip;           // 1: the source is read left-right flipped
  int pad_;
};

static constexpr float TTA_PAD = 0.447f;  // torch_utils.py:448
static constexpr int TTA_MAX_VIEWS = 8;

namespace {

__device__ __forceinline__ float tta_px(const float* p) { return *p; }
// x * fp32(1/255): torch's device division by a scalar, as adr_stem.hip / adr_pack.hip read a uint8 batch — view 0
// goes through those, and the views of a uint8 batch equal the views of the same batch divided on the device
__device__ __forceinline__ float tta_px(const uint8_t* p) { return (float)*p * (1.f / 255.f); }

// ATen's source index and weights of one output index (align_corners=False, no scale_factor)
__device__ __forceinline__ void tta_tap(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256) tta_views_kernel(const T* img, const TtaView* views, float* out, int H, int W) {
  const TtaView v = views[blockIdx.z];
  const int b = blockIdx.y;
  const long p = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const long plane = (long)v.ph * v.pw;
  if (p >= plane) return;
  const int y = (int)(p / v.pw), x = (int)(p - (long)y * v.pw);  // pw % 4 == 0: the 4 pixels share the row
  float* o = out + v.out_off + (long)b * 3 * plane + p;
  f32x4 r[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = f32x4{TTA_PAD, TTA_PAD, TTA_PAD, TTA_PAD};
  if (y < v.rh && x < v.rw) {
    int y0, y1;
    float l0h, l1h;
    tta_tap(y, H, v.rh, y0, y1, l0h, l1h);
    const T* s = img + (long)b * 3 * H * W;
    const T* row0 = s + (long)y0 * W;
    const T* row1 = s + (long)y1 * W;
    const long splane = (long)H * W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x + i >= v.rw) continue;
      int x0, x1;
      float l0w, l1w;
      tta_tap(x + i, W, v.rw, x0, x1, l0w, l1w);
      if (v.flip) {
        x0 = W - 1 - x0;
        x1 = W - 1 - x1;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = tta_px(row0 + c * splane + x0), bb = tta_px(row0 + c * splane + x1);
        const float cc = tta_px(row1 + c * splane + x0), d = tta_px(row1 + c * splane + x1);
        r[c][i] = l0h * (l0w * a + l1w * bb) + l1h * (l0w * cc + l1w * d);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = r[c];
}

struct TtaMergeArgs {
  const float* y[3];
  int A[3];     // columns of each view's output
  int k0[3];    // first kept column
  int off[4];   // first output column of each view; off[3] = A_total
  float s[3];   // scale the boxes are divided by
  int flip[3];  // 1: row 0 becomes img_w - x
  float img_w;
  int rows;
};

// one thread per output element, threads along the anchor axis (coalesced loads and stores)
__global__ void __launch_bounds__(256) tta_merge_kernel(TtaMergeArgs a, float* out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int A_total = a.off[3];
  if (j >= A_total) return;
  const int r = blockIdx.y, b = blockIdx.z;
  const int v = j >= a.off[2] ? 2 : (j >= a.off[1] ? 1 : 0);
  const int col = a.k0[v] + (j - a.off[v]);
  float val = a.y[v][((long)b * a.rows + r) * a.A[v] + col];
  if (r < 4) {
    val = val / a.s[v];  // IEEE fp32 division, as `p[:, :4] /= scale`
    if (r == 0 && a.flip[v]) val = a.img_w - val;
  }
  out[((long)b * a.rows + r) * A_total + j] = val;
}

}  // namespace adr

using namespace adr;

extern "C" int adr_tta_view_size(void) { return (int)sizeof(TtaView); }

extern "C" int adr_tta_views(int dtype, const void* img, int B, int H, int W, const void* views,
                             const void* views_host, int nviews, void* out, size_t out_elems, void* stream) {
  ADR_REQUIRE(dtype == 0 || dtype == 1, "tta_views: dtype code %d (0: fp32, 1: uint8)", dtype);
  ADR_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)B * 3 * H * W < (1l << 31), "tta_views: B=%d H=%d W=%d",
              B, H, W);
  ADR_REQUIRE(img && views && views_host && out && nviews > 0 && nviews <= TTA_MAX_VIEWS,
              "tta_views: null argument or nviews=%d", nviews);
  ADR_REQUIRE(((uintptr_t)out & 15) == 0, "tta_views: out must be 16-byte aligned");
  const TtaView* hv = (const TtaView*)views_host;
  long maxq = 0;
  for (int i = 0; i < nviews; ++i) {
    const TtaView& v = hv[i];
    ADR_REQUIRE(v.rh > 0 && v.rw > 0 && v.ph > 0 && v.pw > 0 && v.rh <= v.ph && v.rw <= v.pw,
                "tta_views: view %d sizes resized %d x %d padded %d x %d", i, v.rh, v.rw, v.ph, v.pw);
    ADR_REQUIRE(v.pw % 4 == 0 && (long)v.ph * v.pw < (1l << 30), "tta_views: view %d padded width %d", i, v.pw);
    ADR_REQUIRE(v.flip == 0 || v.flip == 1, "tta_views: view %d flip %d", i, v.flip);
    const long n = (long)B * 3 * v.ph * v.pw;
    ADR_REQUIRE(v.out_off >= 0 && v.out_off % 4 == 0 && (size_t)v.out_off + (size_t)n <= out_elems,
                "tta_views: view %d output outside the buffer", i);
    for (int k = 0; k < i; ++k) {
      const long nk = (long)B * 3 * hv[k].ph * hv[k].pw;
      ADR_REQUIRE(v.out_off + n <= hv[k].out_off || hv[k].out_off + nk <= v.out_off,
                  "tta_views: views %d and %d overlap in the output", k, i);
    }
    const long q = (long)v.ph * v.pw / 4;
    maxq = q > maxq ? q : maxq;
  }
  const dim3 grid(cdiv(maxq, 256), B, nviews);
  if (dtype == 1)
    hipLaunchKernelGGL(tta_views_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)img,
                       (const TtaView*)views, (float*)out, H, W);
  else
    hipLaunchKernelGGL(tta_views_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)img,
                       (const TtaView*)views, (float*)out, H, W);
  return check_launch("adr_tta_views");
}

extern "C" int adr_tta_merge(const float* y0, const float* y1, const float* y2, const int* anchors, const int* keep0,
                             const int* keep1, const float* scales, const int* flips, float img_w, float* out, int B,
                             int rows, int A_total, void* stream) {
  ADR_REQUIRE(y0 && y1 && y2 && anchors && keep0 && keep1 && scales && flips && out, "tta_merge: null argument");
  ADR_REQUIRE(B > 0 && B <= 65535 && rows >= 4 && rows <= 65535 && A_total > 0, "tta_merge: B=%d rows=%d A_total=%d", B,
              rows, A_total);
  TtaMergeArgs a;
  a.y[0] = y0;
  a.y[1] = y1;
  a.y[2] = y2;
  long off = 0;
  for (int v = 0; v < 3; ++v) {
    ADR_REQUIRE(anchors[v] > 0 && keep0[v] >= 0 && keep0[v] <= keep1[v] && keep1[v] <= anchors[v] &&
                    (long)B * rows * anchors[v] < (1l << 40),
                "tta_merge: view %d keeps [%d, %d) of %d columns", v, keep0[v], keep1[v], anchors[v]);
    ADR_REQUIRE(scales[v] > 0.f && (flips[v] == 0 || flips[v] == 1), "tta_merge: view %d scale %g flip %d", v,
                (double)scales[v], flips[v]);
    a.A[v] = anchors[v];
    a.k0[v] = keep0[v];
    a.off[v] = (int)off;
    a.s[v] = scales[v];
    a.flip[v] = flips[v];
    off += keep1[v] - keep0[v];
  }
  ADR_REQUIRE(off == A_total, "tta_merge: the kept columns sum to %ld, A_total is %d", off, A_total);
  a.off[3] = A_total;
  a.img_w = img_w;
  a.rows = rows;
  hipLaunchKernelGGL(tta_merge_kernel, dim3(cdiv(A_total, 256), rows, B), dim3(256), 0, (hipStream_t)stream, a, out);
  return check_launch("adr_tta_merge");
}
