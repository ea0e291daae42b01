// Device-resident input (gz_create_from_device / gz_set_rgb_device / gz_pack_rgb_device): a strided
// w x h x 3 image of uint8, float32, float16 or bfloat16 elements that already lives in device memory
// becomes the context's packed 8-bit d_rgb and, in the same pass, its three linear planes (what
// k_linear_from_rgb8 makes of d_rgb behind the host upload).
//
// The byte of an element: integers pass through.  A float x is widened exactly to f32, multiplied by
// 255.0f (one f32 rounding; the build has contraction off), NaN and everything below 0 become 0,
// everything above 255 becomes 255, and the rest is rounded to nearest, ties to even:
//   np.rint(np.clip(np.where(np.isnan(v), 0, v), 0, 255))  with  v = x.astype(f32) * f32(255)
// float16 and bfloat16 arrive as their 16 bits and are widened with integer operations, so that the
// emulation build runs the same source without a half type.
//
// gz_device_pixels adds what a PNG can hold beyond that (host/png_reader.cc, the reference's ReadPNG): uint16
// elements, whose byte is the HIGH byte v >> 8 (libpng's STRIP_16, no rounding), and an alpha sample per pixel, of
// the colours' element type and under their byte rule, with which k_ingest_rgba blends the colour bytes over a
// background:  out = (v * a + bg * (255 - a) + 128) / 255  in integers -- BlendOnBlack (guetzli.cc:42-44) at bg = 0.
#pragma once
#include "gz_common.h"

namespace gz {

// the element types of gz_device_image::dtype (GZ_DT_*); the 16-bit floats are their bit patterns
struct ingest_f16 { uint16_t bits; };
struct ingest_bf16 { uint16_t bits; };

GZ_DEVFN float ingest_widen(float x) { return x; }
GZ_DEVFN float ingest_widen(ingest_bf16 x) { return __uint_as_float((unsigned)x.bits << 16); }
GZ_DEVFN float ingest_widen(ingest_f16 x) {
  const unsigned h = x.bits, sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return __uint_as_float(sign | 0x7f800000u | (m << 13));            // inf, NaN
  if (e != 0u) return __uint_as_float(sign | ((e + 112u) << 23) | (m << 13));      // normal: bias 15 -> 127
  if (m == 0u) return __uint_as_float(sign);                                       // +-0
  // subnormal m * 2^-24: the leading one moves to bit 10, the exponent follows it (a normal f32)
  const int s = __clz((int)m) - 21;                                                // m << s has bit 10 set
  return __uint_as_float(sign | ((unsigned)(113 - s) << 23) | (((m << s) & 0x3ffu) << 13));
}

GZ_DEVFN uint8_t ingest_byte(uint8_t x) { return x; }
GZ_DEVFN uint8_t ingest_byte(float x) {
  float v = x * 255.0f;
  v = v >= 0.0f ? v : 0.0f;       // NaN compares false: 0, as everything negative (-inf too)
  v = v > 255.0f ? 255.0f : v;    // +inf too
  return (uint8_t)(int)rintf(v);  // ties to even
}
GZ_DEVFN uint8_t ingest_byte(uint16_t x) { return (uint8_t)(x >> 8); }   // the high byte, not a rounding
GZ_DEVFN uint8_t ingest_byte(ingest_f16 x) { return ingest_byte(ingest_widen(x)); }
GZ_DEVFN uint8_t ingest_byte(ingest_bf16 x) { return ingest_byte(ingest_widen(x)); }

// 16 bytes of elements moved as one access (global_load_dwordx4)
template <class T>
struct alignas(16) IngestVec {
  T e[16 / sizeof(T)];
};

enum { kIngestElementwise = 0, kIngestPlanarRows = 1, kIngestInterleavedRows = 2, kIngestRgbaRows = 3, kIngestGreyAlphaRows = 4 };

// Element (y, x, c) is data[y * sy + x * sx + c * sc] (strides in elements, >= 0, 64-bit offsets).  One lane takes
// P = 16 / sizeof(T) consecutive pixels of one row -- consecutive lanes sit on consecutive groups of a row, rows
// follow each other -- so that a full group is read as three 16-byte vectors where the layout allows it:
//   wide == kIngestPlanarRows       sx == 1: one vector per channel (CHW rows, crops of them, grey with sc == 0)
//   wide == kIngestInterleavedRows  sc == 1, sx == 3: the group's 3 P elements are consecutive (HWC rows, crops)
// The CALLER says which (ingest_wide_mode below: it also needs the base address and the byte strides the vectors
// move by to be multiples of 16); kIngestElementwise, and the partial group at the end of every row, read element
// by element.  No path reads an element other than the (y, x, c) it converts: nothing outside
// [0, (h-1) sy + (w-1) sx + 2 sc] is touched.
// Output: rgb[(y * w + x) * 3 + c], a full group as 3 P / 4 dwords when its first byte is dword-aligned (every group
// when w is a multiple of 4) and byte by byte otherwise; and, if lin != nullptr, lin[c * pstride + y * pitch + x] =
// lut[byte], a full group as 16-byte stores when the address allows it.  The 1 KB table is staged in LDS.
// B... (empty, or one BatchTensor: gz_common.h): the batched form, gridDim.y = N images of the caller's tensor into N
// arenas' linear planes.  It writes no packed bytes (rgb is not used: a comparison reads the planes alone), and `wide`
// is the CALLER's word for every image of the batch (stride_n must keep the vectors' alignment too).
template <class T, class... B>
__global__ __launch_bounds__(256) void k_ingest_rgb(const T* __restrict__ data, long long sy, long long sx,
                                                    long long sc, int w, int h, int wide,
                                                    uint8_t* __restrict__ rgb, const float* __restrict__ lut,
                                                    float* __restrict__ lin, int pitch, size_t pstride, B... batch) {
  constexpr int P = 16 / (int)sizeof(T);
  if constexpr (sizeof...(B) > 0) {
    const BatchTensor bt = (batch, ...);
    data += (long long)blockIdx.y * bt.stride_n;
    lin += (size_t)blockIdx.y * bt.plane_stride;
  }
  __shared__ float s_lut[256];
  if (lin != nullptr) {   // (uniform: every thread of the block gets here)
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  const unsigned gpr = (unsigned)(w + P - 1) / P;                  // groups per row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;              // (gpr * h <= 16384 * 65535)
  if (g >= gpr * (unsigned)h) return;
  const int y = (int)(g / gpr), x0 = (int)(g - (unsigned)y * gpr) * P;
  const int n = w - x0 < P ? w - x0 : P;
  const T* src = data + ((long long)y * sy + (long long)x0 * sx);
  uint8_t b[3 * P];
  if (wide != kIngestElementwise && n == P) {
    IngestVec<T> v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      v[k] = *reinterpret_cast<const IngestVec<T>*>(src + (wide == kIngestPlanarRows ? (long long)k * sc : (long long)k * P));
    if (wide == kIngestPlanarRows) {
#pragma unroll
      for (int i = 0; i < P; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * i + c] = ingest_byte(v[c].e[i]);
    } else {
#pragma unroll
      for (int j = 0; j < 3 * P; ++j) b[j] = ingest_byte(v[j / P].e[j % P]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        b[3 * i + c] = i < n ? ingest_byte(src[(long long)i * sx + (long long)c * sc]) : (uint8_t)0;
  }
  if constexpr (sizeof...(B) == 0) {
  uint8_t* dst = rgb + ((size_t)y * w + x0) * 3;
  if (n == P && ((uintptr_t)dst & 3u) == 0) {
    uint32_t* dst4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int j = 0; j < 3 * P / 4; ++j)
      dst4[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 3 * P; ++j)
      if (j < 3 * n) dst[j] = b[j];
  }
  }
  if (lin == nullptr) return;
  float* out = lin + ((size_t)y * pitch + x0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* pl = out + (size_t)c * pstride;
    if (n == P && ((uintptr_t)pl & 15u) == 0) {
#pragma unroll
      for (int q = 0; q < P / 4; ++q) {
        gz_f4 f;
#pragma unroll
        for (int j = 0; j < 4; ++j) f.v[j] = s_lut[b[3 * (4 * q + j) + c]];
        GZ_STG4(pl, 4 * q, f);
      }
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i < n) pl[i] = s_lut[b[3 * i + c]];
    }
  }
}

// The floor of (v a + bg (255 - a) + 128) / 255 for bytes v, a, bg: the numerator is at most 255 * 255 + 128, the
// division an integer one (the shortcuts (t + (t >> 8)) >> 8 and a multiplication by 1 / 255 ROUND: they differ from
// it on 128 of the 65536 (v, a) pairs at bg = 0).
GZ_DEVFN uint8_t ingest_blend(unsigned v, unsigned a, unsigned bg) { return (uint8_t)((v * a + bg * (255u - a) + 128u) / 255u); }

// What k_ingest_rgb does with the bytes of a lane's group (the same stores, in the same forms): b[3 i + c] of the n
// pixels from (y, x0) on -> rgb and, if lin != nullptr, the linear planes through the staged table.
template <int P>
GZ_DEVFN void ingest_emit(const uint8_t (&b)[3 * P], int n, int y, int x0, int w, uint8_t* __restrict__ rgb,
                          const float* s_lut, float* __restrict__ lin, int pitch, size_t pstride) {
  uint8_t* dst = rgb + ((size_t)y * w + x0) * 3;
  if (n == P && ((uintptr_t)dst & 3u) == 0) {
    uint32_t* dst4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int j = 0; j < 3 * P / 4; ++j)
      dst4[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 3 * P; ++j)
      if (j < 3 * n) dst[j] = b[j];
  }
  if (lin == nullptr) return;
  float* out = lin + ((size_t)y * pitch + x0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* pl = out + (size_t)c * pstride;
    if (n == P && ((uintptr_t)pl & 15u) == 0) {
#pragma unroll
      for (int q = 0; q < P / 4; ++q) {
        gz_f4 f;
#pragma unroll
        for (int j = 0; j < 4; ++j) f.v[j] = s_lut[b[3 * (4 * q + j) + c]];
        GZ_STG4(pl, 4 * q, f);
      }
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i < n) pl[i] = s_lut[b[3 * i + c]];
    }
  }
}

// k_ingest_rgb for pixels with an alpha sample: colours as there, the alpha of pixel (y, x) is alpha[y * sy + x * sx]
// -- a pointer of its own under the colours' two strides: data + 3 of HWC RGBA, the fourth plane of CHW, data + 1 of
// interleaved grey + alpha (sc == 0, sx == 2), a mask in another allocation.  The byte that comes out is
// ingest_blend(colour byte, alpha byte, bg byte), bg = r | g << 8 | b << 16.  Same lane-to-pixel mapping (P consecutive
// pixels of a row per lane: the stores stay k_ingest_rgb's), same grid.  WIDE, a template parameter chosen by the
// CALLER (ingest_alpha_wide_mode below), says how a full group is read -- one read path per instantiation, nothing
// to choose at run time:
//   kIngestPlanarRows     sx == 1: one 16-byte vector per colour plane and one of alpha
//   kIngestRgbaRows       sc == 1, sx == 4, alpha == data + 3: the group's 4 P consecutive elements as four vectors
//   kIngestGreyAlphaRows  sc == 0, sx == 2, alpha == data + 1: its 2 P consecutive elements as two
//   kIngestElementwise    element by element, as the partial group at the end of a row is read in every instantiation
// (A lane's vectors are 64 or 32 consecutive bytes, so a wave's k-th load takes every fourth or second 16-byte piece of
// a 4 KB or 2 KB run and the k loads together take all of it once: the lines come from memory once and the later loads
// hit them in the cache, as k_ingest_rgb's three 48-byte-strided loads do at 3.4 TB/s.  Lane i on piece i would need
// the bytes of a pixel to change lanes before the blend; the stores, two thirds of the traffic, want this mapping.)
// No path reads an element other than the (y, x, c) or the (y, x) alpha it converts.
template <class T, int WIDE>
__global__ __launch_bounds__(256) void k_ingest_rgba(const T* data, const T* alpha, long long sy, long long sx, long long sc,
                                                     int w, int h, unsigned bg, uint8_t* __restrict__ rgb,
                                                     const float* __restrict__ lut, float* __restrict__ lin, int pitch,
                                                     size_t pstride) {
  constexpr int P = 16 / (int)sizeof(T);
  __shared__ float s_lut[256];
  if (lin != nullptr) {   // (uniform: every thread of the block gets here)
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  const unsigned gpr = (unsigned)(w + P - 1) / P;                  // groups per row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;              // (gpr * h <= 16384 * 65535)
  if (g >= gpr * (unsigned)h) return;
  const int y = (int)(g / gpr), x0 = (int)(g - (unsigned)y * gpr) * P;
  const int n = w - x0 < P ? w - x0 : P;
  const long long first = (long long)y * sy + (long long)x0 * sx;
  const T* src = data + first;
  const T* asrc = alpha + first;
  uint8_t v[3 * P], a[P];
  if (WIDE != kIngestElementwise && n == P) {
    if constexpr (WIDE == kIngestPlanarRows) {
      IngestVec<T> q[4];
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = *reinterpret_cast<const IngestVec<T>*>(src + (long long)k * sc);
      q[3] = *reinterpret_cast<const IngestVec<T>*>(asrc);
#pragma unroll
      for (int i = 0; i < P; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * i + c] = ingest_byte(q[c].e[i]);
        a[i] = ingest_byte(q[3].e[i]);
      }
    } else if constexpr (WIDE == kIngestRgbaRows) {
      IngestVec<T> q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const IngestVec<T>*>(src + k * P);
#pragma unroll
      for (int i = 0; i < P; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * i + c] = ingest_byte(q[(4 * i + c) / P].e[(4 * i + c) % P]);
        a[i] = ingest_byte(q[(4 * i + 3) / P].e[(4 * i + 3) % P]);
      }
    } else {
      static_assert(WIDE == kIngestElementwise || WIDE == kIngestGreyAlphaRows, "k_ingest_rgba: an unknown read path");
      IngestVec<T> q[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) q[k] = *reinterpret_cast<const IngestVec<T>*>(src + k * P);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        v[3 * i] = v[3 * i + 1] = v[3 * i + 2] = ingest_byte(q[(2 * i) / P].e[(2 * i) % P]);
        a[i] = ingest_byte(q[(2 * i + 1) / P].e[(2 * i + 1) % P]);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[3 * i + c] = i < n ? ingest_byte(src[(long long)i * sx + (long long)c * sc]) : (uint8_t)0;
      a[i] = i < n ? ingest_byte(asrc[(long long)i * sx]) : (uint8_t)0;
    }
  }
  uint8_t b[3 * P];
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) b[3 * i + c] = ingest_blend(v[3 * i + c], a[i], (bg >> (8 * c)) & 255u);
  ingest_emit<P>(b, n, y, x0, w, rgb, s_lut, lin, pitch, pstride);
}

// Which of the kernel's read paths a layout may take (host side).  The vectors of the planar form sit at
// base + (y sy + x0 + k sc) elements, those of the interleaved form at base + (y sy + 3 x0 + k P) elements, x0 a
// multiple of P = 16 / elem: both are 16-byte aligned if the base is and sy (and, planar, sc) are multiples of P.
static inline int ingest_wide_mode(const void* data, size_t elem, long long sy, long long sx, long long sc) {
  const long long p = (long long)(16 / elem);
  if (((uintptr_t)data & 15u) != 0 || sy % p != 0) return kIngestElementwise;
  if (sx == 1 && sc % p == 0) return kIngestPlanarRows;
  if (sc == 1 && sx == 3) return kIngestInterleavedRows;
  return kIngestElementwise;
}
// The same for k_ingest_rgba.  Alpha's vector of the planar form sits at alpha + (y sy + x0) elements, the vectors of
// the two interleaved forms at base + (y sy + x0 sx + k P) elements, sx = 4 or 2, and hold the alpha samples too.
static inline int ingest_alpha_wide_mode(const void* data, const void* alpha, size_t elem, long long sy, long long sx, long long sc) {
  const long long p = (long long)(16 / elem);
  const char* next = (const char*)data;   // (alpha == data + k elements: compared as addresses, never dereferenced here)
  if (((uintptr_t)data & 15u) != 0 || sy % p != 0) return kIngestElementwise;
  if (sx == 1 && sc % p == 0 && ((uintptr_t)alpha & 15u) == 0) return kIngestPlanarRows;
  if (sc == 1 && sx == 4 && (const char*)alpha == next + 3 * elem) return kIngestRgbaRows;
  if (sc == 0 && sx == 2 && (const char*)alpha == next + elem) return kIngestGreyAlphaRows;
  return kIngestElementwise;
}
// k_ingest_rgba<T> in the instantiation whose read path the layout may take (host side).
template <class T>
static inline void launch_ingest_rgba(hipStream_t stream, dim3 grid, dim3 block, const T* data, const T* alpha, long long sy,
                                      long long sx, long long sc, int w, int h, unsigned bg, uint8_t* rgb, const float* lut,
                                      float* lin, int pitch, size_t pstride) {
  switch (ingest_alpha_wide_mode(data, alpha, sizeof(T), sy, sx, sc)) {
    case kIngestPlanarRows:
      GZ_LAUNCH((k_ingest_rgba<T, kIngestPlanarRows>), grid, block, stream, data, alpha, sy, sx, sc, w, h, bg, rgb, lut, lin, pitch, pstride);
      break;
    case kIngestRgbaRows:
      GZ_LAUNCH((k_ingest_rgba<T, kIngestRgbaRows>), grid, block, stream, data, alpha, sy, sx, sc, w, h, bg, rgb, lut, lin, pitch, pstride);
      break;
    case kIngestGreyAlphaRows:
      GZ_LAUNCH((k_ingest_rgba<T, kIngestGreyAlphaRows>), grid, block, stream, data, alpha, sy, sx, sc, w, h, bg, rgb, lut, lin, pitch, pstride);
      break;
    default:
      GZ_LAUNCH((k_ingest_rgba<T, kIngestElementwise>), grid, block, stream, data, alpha, sy, sx, sc, w, h, bg, rgb, lut, lin, pitch, pstride);
      break;
  }
}

}  // namespace gz
