// Linear float input (gz_create_from_device_linear / gz_set_linear_device / gz_compare_device_linear /
// gz_butteraugli_linear): a strided w x h x 3 image of float32, float16 or bfloat16 elements that already lives in
// device memory becomes the context's three linear planes -- the planes ButteraugliInterface (butteraugli.h:44-79)
// takes: raw intensity 0..255 as floats.  k_ingest_rgb (gz_kernels_ingest.h) without the byte image and without the
// table: nothing is rounded to a byte, nothing is gamma-decoded.
//
// The value of an element x:
//   v = ingest_widen(x) * scale      the exact widening to f32, then ONE f32 multiplication (the build has contraction
//                                    off); with scale == 1.0f the identity on every float that is no NaN
//   NaN and everything below 0 become 0 (-inf too); -0.0 is not below 0 and stays -0.0
//   everything above 255 becomes 255 (+inf too)
//     np.where(np.isnan(v) | (v < 0), 0, np.where(v > 255, 255, v))  with  v = x.astype(f32) * f32(scale)
// Inside [0, 255] nothing is altered.  Outside it the reference is undefined by its own documentation
// (butteraugli.h:52-56) and the chain's tables and branches were never pinned there, so the clamp is a
// deliberate difference; every element it alters is COUNTED: one atomicAdd per wavefront that has any, into *altered,
// which the caller has cleared on the stream in front of the kernel.
// float16 and bfloat16 arrive as their 16 bits and are widened with integer operations (ingest_widen), so that the
// emulation build runs the same source without a half type.
#pragma once
#include "gz_common.h"
#include "gz_kernels_ingest.h"

namespace gz {

// one more read path beside gz_kernels_ingest.h's: the image is EXTENDED to the canvas (below)
enum { kIngestExtend = 5 };

// The reference's rule for images under 8 pixels (ButteraugliDiffmap, butteraugli.cc:1825-1855): the w x h canvas
// (8 in every dimension the image is smaller in) reads source pixel
//   (clamp(x - xborder, 0, src_w - 1), clamp(y - yborder, 0, src_h - 1))
// xborder = (8 - src_w) / 2 in integers where src_w < 8, else 0; the same in y.  (Unused by the other read paths.)
struct IngestExtent {
  int src_w, src_h, xborder, yborder;
};

// The rule above for one element; *n counts the elements it altered.
GZ_DEVFN float ingest_linear_value(float x, float scale, unsigned* n) {
  const float v = x * scale;
  float r = v >= 0.0f ? v : 0.0f;     // NaN compares false: 0, as everything negative (-inf too); -0.0 >= 0 stays
  r = r > 255.0f ? 255.0f : r;        // +inf too
  *n += (!(v >= 0.0f) || v > 255.0f) ? 1u : 0u;
  return r;
}

// Element (y, x, c) is data[y * sy + x * sx + c * sc] (strides in elements, >= 0, 64-bit offsets).  Lanes and pixels as
// in k_ingest_rgb: one lane takes P = 16 / sizeof(T) consecutive pixels of one row, consecutive lanes consecutive
// groups, rows follow each other.  WIDE, a template parameter chosen by the CALLER (ingest_wide_mode: it also needs the
// base address and the byte strides the vectors move by to be multiples of 16), says how a full group is read -- one
// read path per instantiation:
//   kIngestPlanarRows       sx == 1: one 16-byte vector per channel (CHW rows, crops of them, grey with sc == 0)
//   kIngestInterleavedRows  sc == 1, sx == 3: the group's 3 P consecutive elements as three vectors (HWC rows, crops)
//   kIngestElementwise      element by element, as the partial group at the end of a row is in every instantiation
//   kIngestExtend           element by element from the pixel IngestExtent's rule names: w x h is the canvas, the
//                           strides are the source's
// No path reads an element other than the (y, x, c) it converts: nothing outside [0, (h-1) sy + (w-1) sx + 2 sc] (of
// the source's w, h) is touched.
// Output: lin[c * pstride + y * pitch + x], a full group as 16-byte stores when the address allows it, float by float
// otherwise; nothing outside the three planes' w x h is written.
// *altered += the number of elements the value rule altered (under kIngestExtend: of the canvas pixels that ARE source
// pixels, so that a replicated border does not count its source again).  Every thread of the block reaches the
// wavefront's vote: lanes behind the last group take part with nothing.
template <class T, int WIDE>
__global__ __launch_bounds__(256) void k_ingest_linear(const T* __restrict__ data, long long sy, long long sx, long long sc,
                                                       int w, int h, float scale, IngestExtent ext, float* __restrict__ lin,
                                                       int pitch, size_t pstride, unsigned* __restrict__ altered) {
  static_assert(WIDE == kIngestElementwise || WIDE == kIngestPlanarRows || WIDE == kIngestInterleavedRows || WIDE == kIngestExtend,
                "k_ingest_linear: an unknown read path");
  constexpr int P = 16 / (int)sizeof(T);
  const unsigned gpr = (unsigned)(w + P - 1) / P;                  // groups per row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;              // (gpr * h <= 16384 * 65535)
  unsigned cnt = 0;
  if (g < gpr * (unsigned)h) {
    const int y = (int)(g / gpr), x0 = (int)(g - (unsigned)y * gpr) * P;
    const int n = w - x0 < P ? w - x0 : P;
    float f[3][P];
    if constexpr (WIDE == kIngestExtend) {
      const int ys = y - ext.yborder, yc = ys < 0 ? 0 : (ys >= ext.src_h ? ext.src_h - 1 : ys);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int xs = x0 + i - ext.xborder, xc = xs < 0 ? 0 : (xs >= ext.src_w ? ext.src_w - 1 : xs);
        const bool own = ys == yc && xs == xc;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          unsigned one = 0;
          f[c][i] = i < n ? ingest_linear_value(ingest_widen(data[(long long)yc * sy + (long long)xc * sx + (long long)c * sc]), scale, &one) : 0.0f;
          cnt += i < n && own ? one : 0u;
        }
      }
    } else {
      const T* src = data + ((long long)y * sy + (long long)x0 * sx);
      if (WIDE != kIngestElementwise && n == P) {
        IngestVec<T> v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          v[k] = *reinterpret_cast<const IngestVec<T>*>(src + (WIDE == kIngestPlanarRows ? (long long)k * sc : (long long)k * P));
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int j = 3 * i + c;
            f[c][i] = ingest_linear_value(ingest_widen(WIDE == kIngestPlanarRows ? v[c].e[i] : v[j / P].e[j % P]), scale, &cnt);
          }
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            unsigned one = 0;
            f[c][i] = i < n ? ingest_linear_value(ingest_widen(src[(long long)i * sx + (long long)c * sc]), scale, &one) : 0.0f;
            cnt += one;
          }
      }
    }
    float* out = lin + ((size_t)y * pitch + x0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* pl = out + (size_t)c * pstride;
      if (n == P && ((uintptr_t)pl & 15u) == 0) {
#pragma unroll
        for (int q = 0; q < P / 4; ++q) {
          gz_f4 t;
#pragma unroll
          for (int j = 0; j < 4; ++j) t.v[j] = f[c][4 * q + j];
          GZ_STG4(pl, 4 * q, t);
        }
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i < n) pl[i] = f[c][i];
      }
    }
  }
  // the wavefront's sum of cnt (at most 3 P = 24 per lane: five bits), one vote per bit; wavefronts without an altered
  // element -- every wavefront of an image inside [0, 255] -- leave after the first vote
  if (__ballot(cnt != 0u) == 0ull) return;
  unsigned total = 0;
#pragma unroll
  for (int b = 0; b < 5; ++b) total += (unsigned)GZ_POPC64(__ballot((cnt >> b) & 1u)) << b;
  if ((threadIdx.x & 63u) == 0u) atomicAdd(altered, total);
}

// k_ingest_linear<T> on `stream` in the instantiation whose read path the layout may take (host side); ext == nullptr:
// the image is the canvas.  The vectors sit where k_ingest_rgb's do, so the conditions are ingest_wide_mode's.
template <class T>
static inline void launch_ingest_linear(hipStream_t stream, const T* data, long long sy, long long sx, long long sc, int w, int h,
                                        float scale, const IngestExtent* ext, float* lin, int pitch, size_t pstride, unsigned* altered) {
  constexpr int P = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256)), block(256);
  const IngestExtent none = {w, h, 0, 0};
  if (ext) {
    GZ_LAUNCH((k_ingest_linear<T, kIngestExtend>), grid, block, stream, data, sy, sx, sc, w, h, scale, *ext, lin, pitch, pstride, altered);
    return;
  }
  switch (ingest_wide_mode(data, sizeof(T), sy, sx, sc)) {
    case kIngestPlanarRows:
      GZ_LAUNCH((k_ingest_linear<T, kIngestPlanarRows>), grid, block, stream, data, sy, sx, sc, w, h, scale, none, lin, pitch, pstride, altered);
      break;
    case kIngestInterleavedRows:
      GZ_LAUNCH((k_ingest_linear<T, kIngestInterleavedRows>), grid, block, stream, data, sy, sx, sc, w, h, scale, none, lin, pitch, pstride, altered);
      break;
    default:
      GZ_LAUNCH((k_ingest_linear<T, kIngestElementwise>), grid, block, stream, data, sy, sx, sc, w, h, scale, none, lin, pitch, pstride, altered);
      break;
  }
}

}  // namespace gz
