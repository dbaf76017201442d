// Detection validator, per-image bookkeeping after NMS in one launch per batch (reference
// models/yolo/detect/val.py:104-161 _prepare_batch / update_metrics, engine/validator.py:221-261 match_predictions,
// utils/metrics.py:52-72 box_iou, :932-989 ConfusionMatrix.process_batch). One 320-thread workgroup per image:
//
//   a. labels to native space: xywh2xyxy, * (W, H, W, H), scale_boxes with the image's ratio_pad ((v - pad) / gain
//      with a true fp32 division, clip to the source image) -> gt_xyxy; the fp32 operations of the reference in its
//      order.
//   b. TP matching at T IoU thresholds, the rule of adr_match_predictions: each detection's best same-class label
//      (exact IoU ties: the larger label index); at threshold t a detection is correct iff its best IoU >= t and no
//      lower-index detection with the same best label also reaches t.
//   c. confusion matrix: detections with conf > cm_conf; class-agnostic pairs with IoU > cm_iou; each such detection
//      keeps its highest-IoU pair, each label then the highest-IoU surviving pair. Matched label: [det_cls, gt_cls];
//      unmatched label: [nc, gt_cls]; kept detection without a match: [det_cls, nc] only when the image has at least
//      one match (the reference's `if n:`). Exact IoU ties between candidate pairs (numpy's unstable sort decides
//      them in the reference: PARITY UNPINNED): a detection prefers the larger label index, a label the lower
//      detection index.
//   d. tallies: nt_per_class (labels per class), nt_per_image (images with at least one label of the class).
//
// Data flow: the image's detection rows are staged in LDS (coalesced) and each of the first n threads takes one row
// into registers; the labels are converted and staged through LDS in chunks of VAL_GCHUNK, and every detection
// thread walks the chunk (all lanes read the same label: LDS broadcast) computing the IoU on the fly in
// box_iou_kernel's operation order. No (G, P) matrix exists anywhere. The label side of both matchings is resolved
// per detection against the other detections' (best label, best IoU) in LDS, O(P^2) with P <= 300, so labels need no
// per-label state and their number is unbounded. cm and the tallies are accumulated with integer global atomics:
// order-free, deterministic. Compiled without FMA contraction / SLP packing (Makefile), as adr_nms.hip.
#include "adr_common.h"

#pragma clang fp contract(off)

namespace adr {

static constexpr int VAL_THREADS = 320;   // 5 waves: one thread per detection row (rows <= 300, the adr_nms cap)
static constexpr int VAL_PMAX = 300;
static constexpr int VAL_TMAX = 16;
static constexpr int VAL_GCHUNK = 256;    // labels staged in LDS per pass
static constexpr int VAL_NCMAX = 1024;    // class bitmap of nt_per_image (the adr_nms class limit)
static constexpr float VAL_EPS = 1e-7f;   // box_iou's eps (utils/metrics.py:52)

struct ValRow {
  float gain, padx, pady, w0, h0;
};

struct ValArgs {
  const float* det;      // (B, rows, 6) native space
  const int* counts;     // [B]
  const float* cls;      // [N]
  const float* bboxes;   // [N, 4] normalised xywh
  const int* gt_off;     // [B + 1]
  const ValRow* tab;     // [B]
  const float* thr;      // [T]
  float* gt_xyxy;        // [N, 4]
  unsigned char* correct;  // (B, rows, T)
  int* cm;               // (nc + 1, nc + 1) or null
  int* nt_class;         // [nc]
  int* nt_image;         // [nc]
  int B, rows, N, T, nc;
  float W, H, cm_conf, cm_iou;
};

__device__ __forceinline__ int clamp_cls(float c, int nc) { return min(max((int)c, 0), nc); }

__global__ void __launch_bounds__(VAL_THREADS) val_match_kernel(ValArgs a) {
  __shared__ float sdet[VAL_PMAX * 6];
  __shared__ float gbox[VAL_GCHUNK][4];
  __shared__ float gcl[VAL_GCHUNK];
  __shared__ int bg[VAL_THREADS];     // TP: best same-class label (index within the image)
  __shared__ float bv[VAL_THREADS];   //     and its IoU
  __shared__ int cg[VAL_THREADS];     // CM: best label with IoU > cm_iou, -1 none / detection not kept
  __shared__ float cv[VAL_THREADS];
  __shared__ unsigned char gflag[VAL_GCHUNK]; // CM: label of the current chunk is matched
  __shared__ unsigned seen[VAL_NCMAX / 32];   // classes with a label in this image
  __shared__ float th[VAL_TMAX];
  __shared__ int any_match;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int rows = a.rows, T = a.T, nc = a.nc;
  const int n = min(max(a.counts[b], 0), rows);
  // host-validated; the clamps keep a device copy that differs from the validated host copy in bounds
  const int g_lo = min(max(a.gt_off[b], 0), a.N);
  const int G = max(min(a.gt_off[b + 1], a.N) - g_lo, 0);
  const ValRow t = a.tab[b];
  const bool do_cm = a.cm != nullptr;

  if (tid < T) th[tid] = a.thr[tid];
  if (tid < VAL_NCMAX / 32) seen[tid] = 0u;
  if (tid == 0) any_match = 0;
  const float* drow = a.det + (long)b * rows * 6;
  for (int i = tid; i < n * 6; i += VAL_THREADS) sdet[i] = drow[i];
  __syncthreads();

  const bool live = tid < n;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, dconf = 0.f, dcls = -1.f;
  if (live) {
    d0 = sdet[tid * 6];
    d1 = sdet[tid * 6 + 1];
    d2 = sdet[tid * 6 + 2];
    d3 = sdet[tid * 6 + 3];
    dconf = sdet[tid * 6 + 4];
    dcls = sdet[tid * 6 + 5];
  }
  const float area_d = (d2 - d0) * (d3 - d1);
  const bool kept = live && do_cm && dconf > a.cm_conf;
  float best = -1.f, cbest = 0.f;
  int g_best = 0, cg_best = -1;

  // ---- pass 1 over the label chunks: stage a (+ gt_xyxy), tallies, each detection's best labels ----
  for (int c0 = 0; c0 < G; c0 += VAL_GCHUNK) {
    const int gn = min(VAL_GCHUNK, G - c0);
    for (int i = tid; i < gn; i += VAL_THREADS) {
      const long g = (long)g_lo + c0 + i;
      const float x = a.bboxes[4 * g], y = a.bboxes[4 * g + 1];
      const float hw = a.bboxes[4 * g + 2] / 2.f, hh = a.bboxes[4 * g + 3] / 2.f;  // xywh2xyxy (ops.py:412-429)
      float v[4] = {(x - hw) * a.W, (y - hh) * a.H, (x + hw) * a.W, (y + hh) * a.H};
      const float pad[4] = {t.padx, t.pady, t.padx, t.pady};
      const float hi[4] = {t.w0, t.h0, t.w0, t.h0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = fminf(fmaxf((v[k] - pad[k]) / t.gain, 0.f), hi[k]);  // scale_boxes + clip_boxes (ops.py:88-123)
        gbox[i][k] = v[k];
        a.gt_xyxy[4 * g + k] = v[k];
      }
      const float c = a.cls[g];
      gcl[i] = c;
      const int ci = (int)c;
      if (ci >= 0 && ci < nc) {
        atomicAdd(&a.nt_class[ci], 1);
        if (ci < VAL_NCMAX && !(atomicOr(&seen[ci >> 5], 1u << (ci & 31)) & (1u << (ci & 31))))
          atomicAdd(&a.nt_image[ci], 1);
      }
    }
    __syncthreads();
    if (live) {
      for (int i = 0; i < gn; ++i) {
        // box_iou_kernel's order: a = label, b = detection
        const float ax1 = gbox[i][0], ay1 = gbox[i][1], ax2 = gbox[i][2], ay2 = gbox[i][3];
        const float iw = fmaxf(fminf(ax2, d2) - fmaxf(ax1, d0), 0.f);
        const float ih = fmaxf(fminf(ay2, d3) - fmaxf(ay1, d1), 0.f);
        const float inter = iw * ih;
        const float area_a = (ax2 - ax1) * (ay2 - ay1);
        const float iou = inter / (area_a + area_d - inter + VAL_EPS);
        const float v = gcl[i] == dcls ? iou : 0.f;
        if (v >= best) {  // ties: the larger label index
          best = v;
          g_best = c0 + i;
        }
        if (kept && iou > a.cm_iou && iou >= cbest) {  // ties: the larger label index
          cbest = iou;
          cg_best = c0 + i;
        }
      }
    }
    __syncthreads();
  }
  bg[tid] = live ? g_best : -1;
  bv[tid] = live ? best : -1.f;
  cg[tid] = cg_best;
  cv[tid] = cbest;
  __syncthreads();

  // ---- label side, per detection against the others (LDS broadcast reads) ----
  float prior = -1.f;  // TP: best IoU among lower-index detections with the same best label
  bool lost = false;   // CM: another detection holds this label with a larger IoU (ties: the lower index)
  if (live) {
    for (int p = 0; p < n; ++p) {
      if (p < tid && bg[p] == g_best) prior = fmaxf(prior, bv[p]);
      if (cg_best >= 0 && p != tid && cg[p] == cg_best && (cv[p] > cbest || (cv[p] == cbest && p < tid))) lost = true;
    }
  }
  unsigned char* crow = a.correct + ((long)b * rows) * T;
  for (int i = tid; i < rows * T; i += VAL_THREADS)
    if (i >= n * T) crow[i] = 0;  // rows past the image's count
  if (live)
    for (int k = 0; k < T; ++k) crow[tid * T + k] = (unsigned char)(best >= th[k] && !(prior >= th[k]));
  if (!do_cm) return;  // block-uniform

  const bool win = live && cg_best >= 0 && !lost;
  if (win) any_match = 1;  // benign race: every writer stores 1
  __syncthreads();
  const int N1 = nc + 1;
  if (kept && !win && any_match) atomicAdd(&a.cm[(long)clamp_cls(dcls, nc) * N1 + nc], 1);

  // ---- pass 2 over the label chunks: matched labels [det_cls, gt_cls], the rest [nc, gt_cls] ----
  for (int c0 = 0; c0 < G; c0 += VAL_GCHUNK) {
    const int gn = min(VAL_GCHUNK, G - c0);
    for (int i = tid; i < gn; i += VAL_THREADS) gflag[i] = 0;
    __syncthreads();
    if (win && cg_best >= c0 && cg_best < c0 + gn) {
      gflag[cg_best - c0] = 1;  // one winner per label
      const int gc = clamp_cls(a.cls[(long)g_lo + cg_best], nc);
      atomicAdd(&a.cm[(long)clamp_cls(dcls, nc) * N1 + gc], 1);
    }
    __syncthreads();
    for (int i = tid; i < gn; i += VAL_THREADS)
      if (!gflag[i]) atomicAdd(&a.cm[(long)nc * N1 + clamp_cls(a.cls[(long)g_lo + c0 + i], nc)], 1);
    __syncthreads();
  }
}

}  // namespace adr

using namespace adr;

extern "C" int adr_val_match(const float* det, const int* counts, int B, int rows, const float* cls,
                             const float* bboxes, const int* gt_off, const int* gt_off_host, int N,
                             const float* table, int H, int W, const float* thr, int T, float cm_conf, float cm_iou,
                             int nc, float* gt_xyxy, unsigned char* correct, int* cm, int* nt_per_class,
                             int* nt_per_image, void* stream) {
  ADR_REQUIRE(B >= 1 && B <= 65535 && rows >= 0 && rows <= VAL_PMAX && T >= 1 && T <= VAL_TMAX && nc >= 1 &&
                  nc <= VAL_NCMAX && N >= 0 && H > 0 && W > 0,
              "val_match: B=%d rows=%d T=%d nc=%d N=%d H=%d W=%d unsupported (rows <= %d, T <= %d, nc <= %d)", B, rows,
              T, nc, N, H, W, VAL_PMAX, VAL_TMAX, VAL_NCMAX);
  ADR_REQUIRE(counts && gt_off && gt_off_host && table && thr && nt_per_class && nt_per_image &&
                  (rows == 0 || (det && correct)) && (N == 0 || (cls && bboxes && gt_xyxy)),
              "val_match: null argument");
  ADR_REQUIRE(gt_off_host[0] == 0 && gt_off_host[B] == N, "val_match: gt_off must start at 0 and end at N=%d (%d, %d)",
              N, gt_off_host[0], gt_off_host[B]);
  for (int b = 0; b < B; ++b)
    ADR_REQUIRE(gt_off_host[b + 1] >= gt_off_host[b], "val_match: gt_off not monotone at image %d (%d > %d)", b,
                gt_off_host[b], gt_off_host[b + 1]);
  ValArgs a;
  a.det = det;
  a.counts = counts;
  a.cls = cls;
  a.bboxes = bboxes;
  a.gt_off = gt_off;
  a.tab = (const ValRow*)table;
  a.thr = thr;
  a.gt_xyxy = gt_xyxy;
  a.correct = correct;
  a.cm = cm;
  a.nt_class = nt_per_class;
  a.nt_image = nt_per_image;
  a.B = B;
  a.rows = rows;
  a.N = N;
  a.T = T;
  a.nc = nc;
  a.W = (float)W;
  a.H = (float)H;
  a.cm_conf = cm_conf;
  a.cm_iou = cm_iou;
  hipLaunchKernelGGL(val_match_kernel, dim3(B), dim3(VAL_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("adr_val_match");
}
