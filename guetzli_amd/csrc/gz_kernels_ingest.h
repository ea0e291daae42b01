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
GZ_DEVFN uint8_t ingest_byte(ingest_f16 x) { return ingest_byte(ingest_widen(x)); }
GZ_DEVFN uint8_t ingest_byte(ingest_bf16 x) { return ingest_byte(ingest_widen(x)); }

// 16 bytes of elements moved as one access (global_load_dwordx4)
template <class T>
struct alignas(16) IngestVec {
  T e[16 / sizeof(T)];
};

enum { kIngestElementwise = 0, kIngestPlanarRows = 1, kIngestInterleavedRows = 2 };

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
template <class T>
__global__ __launch_bounds__(256) void k_ingest_rgb(const T* __restrict__ data, long long sy, long long sx,
                                                    long long sc, int w, int h, int wide,
                                                    uint8_t* __restrict__ rgb, const float* __restrict__ lut,
                                                    float* __restrict__ lin, int pitch, size_t pstride) {
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

}  // namespace gz
