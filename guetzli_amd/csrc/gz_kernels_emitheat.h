// Device-resident heat map (gz_heatmap_device / gz_compare_device_pixels_heat / gz_heatmap_from_map_device): a
// pitch-strided float plane of butteraugli distances becomes butteraugli's colour picture of them, CreateHeatMapImage
// (butteraugli.cc:1979-1992), a strided w x h x 3 image of uint8, uint16, float32, float16 or bfloat16 elements in the
// caller's device memory.  k_emit_rgb (gz_kernels_emit.h) with ScoreToRgb (butteraugli.cc:1938-1975) in front of it.
//
// ScoreToRgb per pixel, in FP64 and in the reference's order of operations (the build keeps products and sums apart):
//   d = (double)map[px]
//   d < good:  s = (d / good) * 0.3          d < bad:  s = 0.3 + (d - good) / (bad - good) * 0.15
//   otherwise: s = 0.45 + (d - bad) / (bad * 12) * 0.5
//   s = min(max(s * 11, 0.0), 10.0);  ix = (int)s;  mix = s - ix
//   v[c] = mix * colour[ix + 1][c] + (1 - mix) * colour[ix][c]
//   byte[c] = (uint8_t)(255 * pow(v[c], 0.5) + 0.5)
// The last line is NOT evaluated here: the device has no pow that is the host's, and 255 * sqrt(v) + 0.5
// is another byte for some v.  The byte of v is the number of k in 1 .. 255 with thr[k] <= v, where thr[k] is the least
// double for which the HOST's expression gives a byte >= k (heat_thresholds() below, built once per process): eight
// fixed steps of a binary search over a table staged in LDS.
// The element of a byte is k_emit_rgb's (emit_value).  Defined inputs: every finite float, both zeros, negatives
// (black), +inf (white).  For NaN the reference's (int)s is undefined; here ix is 0 and the result unspecified.
#pragma once
#include <math.h>

#include <mutex>
#include <string>

#include "gz_common.h"
#include "gz_kernels_emit.h"

namespace gz {

// good and bad, and what the reference forms of them alone: bad - good and bad * 12 are the same operations on the host
struct HeatScale {
  double good, bad, bad_minus_good, bad_times_12;
};
static inline HeatScale heat_scale(double good, double bad) { return HeatScale{good, bad, bad - good, bad * 12}; }

// The 12 x 3 colour table of ScoreToRgb, entries 0, 0.5 and 1 as the codes 0, 1 and 2, two bits each, row ix at bits
// 2 ix: colour[ix][c] = code * 0.5 (exact).
//   rows 0 .. 11:  r  0 0 0 0 1 1 1 .5 1 1 1 1    g  0 0 1 1 1 0 0 .5 .5 1 1 1    b  0 1 1 0 0 0 1 1 .5 .5 1 1
GZ_DEVFN double heat_colour(int ix, int c) {
  const unsigned code = c == 0 ? 0xaa6a00u : c == 1 ? 0xa942a0u : 0xa5a028u;
  return (double)(int)((code >> (2 * ix)) & 3u) * 0.5;
}

// The byte of v: the number of the 255 thresholds (s_thr[k - 1] = thr[k], non-decreasing) that are <= v.  The steps
// 128, 64 .. 1 sum to 255, so no index leaves the table.  (NaN compares false: 0.)
GZ_DEVFN uint8_t heat_byte(double v, const double* s_thr) {
  int n = 0;
#pragma unroll
  for (int step = 128; step > 0; step >>= 1)
    if (s_thr[n + step - 1] <= v) n += step;
  return (uint8_t)n;
}

// ScoreToRgb of one distance.
GZ_DEVFN void heat_rgb(float dist, const HeatScale& hs, const double* s_thr, uint8_t* rgb) {
  const double d = (double)dist;
  // the three branches share their shape, (numerator / denominator) * factor behind a constant: one division
  const bool first = d < hs.good, second = d < hs.bad;
  const double num = first ? d : second ? d - hs.good : d - hs.bad;
  const double den = first ? hs.good : second ? hs.bad_minus_good : hs.bad_times_12;
  const double scaled = (num / den) * (first ? 0.3 : second ? 0.15 : 0.5);
  double s = first ? scaled : (second ? 0.3 : 0.45) + scaled;
  s = s * 11;
  s = s < 0.0 ? 0.0 : s;      // std::max<double>(s, 0.0)
  s = 10.0 < s ? 10.0 : s;    // std::min<double>(s, 10)
  int ix = s >= 0.0 ? (int)s : 0;   // (NaN: 0)
  ix = ix > 10 ? 10 : ix;
  const double mix = s - ix;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = mix * heat_colour(ix + 1, c) + (1 - mix) * heat_colour(ix, c);
    rgb[c] = heat_byte(v, s_thr);
  }
}

// Element (y, x, c) is data[y * sy + x * sx + c * sc]: lanes, groups, the three store paths and their conditions are
// k_emit_rgb's, the source plane's reads k_emit_map's (16-byte loads where a full group's first float is 16-byte
// aligned).  thr: the 255 thresholds, lut: emit_lut(), both in device memory, both staged in LDS.
// No path writes an element other than the (y, x, c) it converts.
template <class T, int WIDE>
__global__ __launch_bounds__(256) void k_emit_heat(const float* __restrict__ map, int w, int h, int pitch, T* __restrict__ data,
                                                   long long sy, long long sx, long long sc, const float* __restrict__ lut,
                                                   const double* __restrict__ thr, HeatScale hs) {
  static_assert(WIDE == kIngestElementwise || WIDE == kIngestPlanarRows || WIDE == kIngestInterleavedRows, "k_emit_heat: an unknown store path");
  constexpr int P = 16 / (int)sizeof(T);
  __shared__ float s_lut[256];
  __shared__ double s_thr[255];
  if (threadIdx.x < 255) s_thr[threadIdx.x] = thr[threadIdx.x];
  if constexpr (emit_reads_lut<T>::value) s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();   // (every thread of the block gets here)
  const unsigned gpr = (unsigned)(w + P - 1) / P;                  // groups per row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;              // (gpr * h <= 16384 * 65535)
  if (g >= gpr * (unsigned)h) return;
  const int y = (int)(g / gpr), x0 = (int)(g - (unsigned)y * gpr) * P;
  const int n = w - x0 < P ? w - x0 : P;
  const float* src = map + ((size_t)y * pitch + x0);
  float f[P];
  if (n == P && ((uintptr_t)src & 15u) == 0) {
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
      const gz_f4 v = GZ_LDG4(src, 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * q + j] = v.v[j];
    }
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i) f[i] = i < n ? src[i] : 0.0f;
  }
  uint8_t b[3 * P];
#pragma unroll
  for (int i = 0; i < P; ++i) heat_rgb(f[i], hs, s_thr, &b[3 * i]);
  T* dst = data + ((long long)y * sy + (long long)x0 * sx);
  if (WIDE != kIngestElementwise && n == P) {
    IngestVec<T> v[3];
    if constexpr (WIDE == kIngestPlanarRows) {
#pragma unroll
      for (int i = 0; i < P; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) emit_value(b[3 * i + c], s_lut, &v[c].e[i]);
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<IngestVec<T>*>(dst + (long long)c * sc) = v[c];
    } else {
#pragma unroll
      for (int j = 0; j < 3 * P; ++j) emit_value(b[j], s_lut, &v[j / P].e[j % P]);
#pragma unroll
      for (int k = 0; k < 3; ++k) *reinterpret_cast<IngestVec<T>*>(dst + k * P) = v[k];
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (i < n) emit_value(b[3 * i + c], s_lut, &dst[(long long)i * sx + (long long)c * sc]);
}

// The thresholds, by the host's own libm (host side).  thr[k - 1], k = 1 .. 255: the least double v for which
// (uint8_t)(255 * pow(v, 0.5) + 0.5) >= k.  It is looked for among the 129 doubles from -64 to +64 ulps around
// ((k - 0.5) / 255)^2, where the exact expression crosses k: over them the bytes must not decrease, must start at k - 1,
// end at k and change once.  Outside the windows the table rests on the error bound of glibc's pow, below 1 ulp: a
// result that far from a byte's boundary cannot be rounded across it.  ok == false (with the reason) where a window
// fails: heat maps are then refused, nothing else is affected.
struct HeatThresholds {
  double thr[255];
  bool ok = false;
  std::string why;
};
static inline uint8_t heat_host_byte(double v) {
  volatile double half = 0.5;   // (the exponent is no compile-time constant: the call stays libm's pow)
  return (uint8_t)(255 * pow(v, half) + 0.5);
}
static inline const HeatThresholds& heat_thresholds() {
  static HeatThresholds t;
  static std::once_flag once;
  std::call_once(once, [] {
    for (int k = 1; k <= 255; ++k) {
      const double root = (k - 0.5) / 255;
      double v = root * root;
      for (int i = 0; i < 64; ++i) v = nextafter(v, 0.0);
      int changes = 0, prev = heat_host_byte(v);
      bool fine = prev == k - 1;
      for (int i = 1; i <= 128 && fine; ++i) {
        v = nextafter(v, 2.0);
        const int b = heat_host_byte(v);
        if (b < prev) fine = false;
        if (b != prev && ++changes == 1) t.thr[k - 1] = v;
        prev = b;
      }
      if (!fine || changes != 1 || prev != k) {
        t.why = "heat map: the host's 255 * pow(v, 0.5) + 0.5 does not step from " + std::to_string(k - 1) + " to " + std::to_string(k) +
                " exactly once within 64 ulps of ((k - 0.5) / 255)^2";
        return;
      }
    }
    t.ok = true;
  });
  return t;
}

// k_emit_heat<T> in the instantiation whose store path the layout may take (host side): ingest_wide_mode's conditions.
template <class T>
static inline void launch_emit_heat(hipStream_t stream, const float* map, int w, int h, int pitch, T* data, long long sy, long long sx,
                                    long long sc, const float* lut, const double* thr, const HeatScale& hs) {
  constexpr int P = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256)), block(256);
  switch (ingest_wide_mode(data, sizeof(T), sy, sx, sc)) {
    case kIngestPlanarRows:
      GZ_LAUNCH((k_emit_heat<T, kIngestPlanarRows>), grid, block, stream, map, w, h, pitch, data, sy, sx, sc, lut, thr, hs);
      break;
    case kIngestInterleavedRows:
      GZ_LAUNCH((k_emit_heat<T, kIngestInterleavedRows>), grid, block, stream, map, w, h, pitch, data, sy, sx, sc, lut, thr, hs);
      break;
    default:
      GZ_LAUNCH((k_emit_heat<T, kIngestElementwise>), grid, block, stream, map, w, h, pitch, data, sy, sx, sc, lut, thr, hs);
      break;
  }
}

}  // namespace gz
