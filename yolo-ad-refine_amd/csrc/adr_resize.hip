// BaseDataset.load_image's resize (reference data/base.py:168-172) in one launch for B images of different sizes:
//
//   cv2.resize(im, (nw, nh), interpolation=cv2.INTER_LINEAR)      HWC BGR uint8 -> HWC BGR uint8
//
// from a staging buffer (the decoded images, packed at byte offsets of any alignment) into the resident image pool
// (adrefine/data/pool.py), where adr_augment_u8 / adr_letterbox_u8 read them as their sources. The arithmetic is
// adr_resize_sample.h's, the same two device functions adr_letterbox_u8 samples with (OpenCV's 8-bit fixed point,
// tables from the host, integer only; PARITY UNPINNED against real OpenCV, see adr_letterbox.hip).
//
// Work mapping. A destination image is a compact byte array of nh * nw * 3 bytes whose offset in the pool is a
// multiple of 4 (the pool hands out multiples of 256), so it is also an array of aligned dwords: one thread per
// destination dword. Its 4 bytes are up to two pixels' channels; (y, x, c) of the first byte come from two divisions
// and the rest by stepping. The thread packs the 4 samples and writes one 32-bit store (a wave writes 256 contiguous
// bytes); the last 1-3 bytes of an image are written as bytes. The grid is flattened over the images: image b owns
// the blocks [prefix[b], prefix[b + 1]) with prefix[b + 1] - prefix[b] = ceil(dwords(b) / 256), and a block finds its
// image by a binary search of the prefix table (block-uniform: scalar loads), so a launch of a 10 x 10 and a
// 640 x 640 image has no idle blocks. Whatever the device tables say, a thread writes only inside its own
// descriptor's destination range.
#include "adr_common.h"
#include "adr_resize_sample.h"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace adr {

struct RsDesc {
  long long src_off;  // byte offset of the source image (HWC BGR uint8, pitch sw * 3) in the staging buffer
  long long dst_off;  // byte offset of the destination image (HWC BGR uint8, pitch nw * 3) in the pool, % 4 == 0
  int sw, sh;         // source size
  int nw, nh;         // destination size
  int mode;           // ResizeMode
  int tab_off;        // RS_LINEAR: sx[nw], a0[nw], a1[nw], sy[nh], b0[nh], b1[nh] (ints) at tables + tab_off
};

static inline long rs_dwords(const RsDesc& d) { return ((long)d.nh * d.nw * 3 + 3) / 4; }

__global__ void __launch_bounds__(256) resize_u8_kernel(const uint8_t* src, const RsDesc* descs, const int* prefix,
                                                         int B, const int* tabs, uint8_t* dst) {
  // the image of this block: the last b with prefix[b] <= blockIdx.x
  const int blk = blockIdx.x;
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= blk) lo = mid;
    else hi = mid - 1;
  }
  const RsDesc d = descs[lo];
  const int total = d.nh * d.nw * 3;  // < 2^31 (validated)
  const long first = (long)(blk - prefix[lo]) * 256 + threadIdx.x;  // dword of the image
  if (first < 0 || first * 4 >= total) return;
  const int byte0 = (int)(first * 4);
  int pix = byte0 / 3, c = byte0 - pix * 3;
  int y = pix / d.nw, x = pix - y * d.nw;
  const uint8_t* S = src + d.src_off;
  const int* t = tabs + d.tab_off;
  ResizeTaps taps = resize_taps(S, d.sw, d.sh, d.nw, d.nh, d.mode, t, x, y);
  const int n = min(4, total - byte0);
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < n) {
      w |= (uint32_t)resize_sample(taps, d.mode, c) << (8 * i);
      if (++c == 3 && i + 1 < n) {
        c = 0;
        if (++x == d.nw) {
          x = 0;
          ++y;
        }
        taps = resize_taps(S, d.sw, d.sh, d.nw, d.nh, d.mode, t, x, y);
      }
    }
  }
  uint8_t* o = dst + d.dst_off + byte0;
  if (n == 4) {
    *reinterpret_cast<uint32_t*>(o) = w;
  } else {
    for (int i = 0; i < n; ++i) o[i] = (uint8_t)(w >> (8 * i));
  }
}

}  // namespace adr

using namespace adr;

extern "C" int adr_resize_desc_size(void) { return (int)sizeof(RsDesc); }

extern "C" int adr_resize_u8(const void* src, size_t src_bytes, const void* descs, const void* descs_host,
                             const int* prefix, int B, const int* tables, int ntab, void* dst, size_t dst_bytes,
                             void* stream) {
  ADR_REQUIRE(B > 0 && B <= (1 << 20), "resize: B=%d", B);
  ADR_REQUIRE(src && descs && descs_host && prefix && tables && dst && ntab >= 0, "resize: null argument");
  ADR_REQUIRE(((uintptr_t)dst & 3) == 0, "resize: the pool is not 4-byte aligned");
  const RsDesc* hd = (const RsDesc*)descs_host;
  std::vector<std::pair<long long, long long>> ranges((size_t)B);
  long blocks = 0;
  for (int b = 0; b < B; ++b) {
    const RsDesc& d = hd[b];
    ADR_REQUIRE(d.sw > 0 && d.sh > 0 && d.nw > 0 && d.nh > 0 && (long)d.sw * d.sh < (1l << 29) &&
                    (long)d.nw * d.nh < (1l << 29),
                "resize: image %d sizes sw=%d sh=%d nw=%d nh=%d", b, d.sw, d.sh, d.nw, d.nh);
    const size_t sbytes = (size_t)d.sw * d.sh * 3, dbytes = (size_t)d.nw * d.nh * 3;
    ADR_REQUIRE(d.src_off >= 0 && (size_t)d.src_off <= src_bytes && sbytes <= src_bytes - (size_t)d.src_off,
                "resize: image %d source outside the staging buffer", b);
    ADR_REQUIRE(d.dst_off >= 0 && (size_t)d.dst_off <= dst_bytes && dbytes <= dst_bytes - (size_t)d.dst_off,
                "resize: image %d destination outside the pool", b);
    ADR_REQUIRE((d.dst_off & 3) == 0, "resize: image %d destination not 4-byte aligned", b);
    if (d.mode == RS_LINEAR)
      ADR_REQUIRE(d.tab_off >= 0 && (long)d.tab_off + 3l * ((long)d.nw + d.nh) <= ntab, "resize: image %d tables", b);
    else if (d.mode == RS_AREA2)
      ADR_REQUIRE(d.sw == 2 * d.nw && d.sh == 2 * d.nh, "resize: image %d area path needs an exact 2x", b);
    else
      ADR_REQUIRE(d.mode == RS_COPY && d.sw == d.nw && d.sh == d.nh, "resize: image %d copy mode / size", b);
    ranges[(size_t)b] = {d.dst_off, d.dst_off + (long long)dbytes};
    blocks += cdiv(rs_dwords(d), 256);
  }
  ADR_REQUIRE(blocks < (1l << 31), "resize: %ld blocks", blocks);
  std::sort(ranges.begin(), ranges.end());
  for (int b = 1; b < B; ++b)
    ADR_REQUIRE(ranges[(size_t)b].first >= ranges[(size_t)b - 1].second,
                "resize: destination ranges [%lld, %lld) and [%lld, %lld) overlap", ranges[(size_t)b - 1].first,
                ranges[(size_t)b - 1].second, ranges[(size_t)b].first, ranges[(size_t)b].second);
  hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)src, (const RsDesc*)descs, prefix, B, tables, (uint8_t*)dst);
  return check_launch("adr_resize_u8");
}
