// Device-resident distance map (gz_compare_device_pixels / gz_compare_rgb / gz_distmap_device): the context's
// pitch-strided float plane c->distmap -- DiffmapPsychoImage's result, what gz_compare downloads -- becomes a strided
// w x h image of float32, float16 or bfloat16 elements in the caller's device memory: out[y * sy + x * sx].
// k_emit_rgb (gz_kernels_emit.h) for one float plane instead of packed bytes.
//
// The element of a distance d:
//   float32   d, bit for bit
//   float16, bfloat16   d rounded to nearest, ties to even, over the WHOLE float32 domain, with integer operations on
//             its bits (the emulation build runs the same source without a half type): results that are subnormals of
//             the format (a distance of 1e-6 is a float16 subnormal), overflow to infinity, infinities, and NaN, which
//             stays a (quiet) NaN of its sign.  numpy's astype(float16); for bfloat16 the rounding of emit_bf16_bits.
// (emit_f16_bits of gz_kernels_emit.h is NOT this: it knows 0 and the normal numbers [1 / 255, 1] only.)
#pragma once
#include "gz_common.h"
#include "gz_kernels_ingest.h"

namespace gz {

GZ_DEVFN uint16_t emit_map_f16_bits(float f) {
  const unsigned u = __float_as_uint(f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                          // NaN
  if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                         // >= 65536, inf: infinity
  if (a >= 0x38800000u)   // >= 2^-14, a normal float16 -- or, by the rounding's carry into the exponent, the infinity 0x7c00
    return (uint16_t)(sign | (((a + 0xfffu + ((a >> 13) & 1u)) >> 13) - (112u << 10)));   // bias 127 -> 15
  const unsigned e = a >> 23;
  if (e < 102u) return (uint16_t)sign;                                             // < 2^-25: below half of the least subnormal
  // a subnormal of the format, m * 2^(e - 150) in units of 2^-24: the 24-bit significand shifted down by 126 - e
  // (14 .. 24) bits, the bits shifted out rounded to nearest even; a carry out of bit 9 gives the least normal number
  const unsigned m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;
  unsigned hb = m >> shift;
  const unsigned rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  if (rest > half || (rest == half && (hb & 1u))) ++hb;
  return (uint16_t)(sign | hb);
}
GZ_DEVFN uint16_t emit_map_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x7fc0u);    // NaN (the carry below would leave NaN)
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                       // (overflow carries into the infinity)
}

GZ_DEVFN void emit_map_value(float f, float* out) { *out = f; }
GZ_DEVFN void emit_map_value(float f, ingest_f16* out) { out->bits = emit_map_f16_bits(f); }
GZ_DEVFN void emit_map_value(float f, ingest_bf16* out) { out->bits = emit_map_bf16_bits(f); }

// Element (y, x) is out[y * sy + x * sx] (strides in elements, > 0 wherever they count, 64-bit offsets; the CALLER has
// checked that no two of the w * h elements share an address).  Lanes and pixels as in k_emit_rgb: one lane takes
// P = 16 / sizeof(T) consecutive pixels of one row -- 4 of float32, 8 of the 16-bit types -- consecutive lanes
// consecutive groups, rows follow each other.  A full group is read as 16-byte loads where its first float is 16-byte
// aligned (the plane's rows have a pitch of w floats: every group when w is a multiple of 4 and the plane is aligned),
// float by float otherwise.  WIDE, a template parameter chosen by the CALLER (emit_map_wide: sx == 1, the base address
// and the byte pitch multiples of 16): a full group leaves as ONE 16-byte store; every other layout, and the partial
// group at the end of a row in either instantiation, goes element by element.
// No path writes an element other than the (y, x) it converts: the destination may be a crop inside a larger tensor,
// and its neighbours stay as they are.
// B... (empty, or one BatchTensor: gz_common.h): the batched form, gridDim.y = N arenas' planes into N images of the
// caller's tensor; WIDE is the caller's word for every one of them.
template <class T, bool WIDE, class... B>
__global__ __launch_bounds__(256) void k_emit_map(const float* __restrict__ map, int w, int h, int pitch, T* __restrict__ out,
                                                  long long sy, long long sx, B... batch) {
  constexpr int P = 16 / (int)sizeof(T);
  if constexpr (sizeof...(B) > 0) {
    const BatchTensor bt = (batch, ...);
    map += (size_t)blockIdx.y * bt.plane_stride;
    out += (long long)blockIdx.y * bt.stride_n;
  }
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
  T* dst = out + ((long long)y * sy + (long long)x0 * sx);
  if (WIDE && n == P) {
    if constexpr (sizeof(T) == 4) {   // float32: the four floats as they are, through the vector store of the planes' kernels
      gz_f4 v;                        // (as a struct copy the compiler splits it into 12 + 4 bytes and shares the tail's code)
#pragma unroll
      for (int i = 0; i < 4; ++i) v.v[i] = f[i];
      GZ_STG4(reinterpret_cast<float*>(dst), 0, v);
    } else {
      IngestVec<T> v;
#pragma unroll
      for (int i = 0; i < P; ++i) emit_map_value(f[i], &v.e[i]);
      *reinterpret_cast<IngestVec<T>*>(dst) = v;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < P; ++i)
    if (i < n) emit_map_value(f[i], &dst[(long long)i * sx]);
}

// The maximum of the w x h window at (x0, y0) of a plane, into *max_bits as the chain's image maximum is formed: float
// bits compared as unsigned -- the map is non-negative -- through atomicMax, one per wavefront at the most; the CALLER
// has cleared *max_bits on the stream in front of the kernel.  ButteraugliScoreFromDiffmap (butteraugli.cc:1857-1867)
// of an image under 8 pixels is the maximum over the CROPPED map (:1846-1854), not over the 8-pixel canvas the chain's
// own maximum covers.  One lane per pixel, rows follow each other; every thread of the block reaches the wavefront's
// exchange, lanes behind the last pixel with a 0.  Nothing outside the window is read.
__global__ __launch_bounds__(256) void k_region_max(const float* __restrict__ plane, int pitch, int x0, int y0, int w, int h,
                                                    unsigned* __restrict__ max_bits) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;              // (w * h < 8 * 65536)
  unsigned m = 0;
  if (i < (unsigned)w * (unsigned)h) {
    const unsigned y = i / (unsigned)w, x = i - y * (unsigned)w;
    m = __float_as_uint(plane[(size_t)(y0 + (int)y) * pitch + (x0 + (int)x)]);
  }
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned o = (unsigned)__shfl((int)m, lane ^ d);
    m = o > m ? o : m;
  }
  if (lane == 0 && m > *(volatile unsigned*)max_bits) atomicMax(max_bits, m);
}
static inline void launch_region_max(hipStream_t stream, const float* plane, int pitch, int x0, int y0, int w, int h, unsigned* max_bits) {
  GZ_LAUNCH(k_region_max, dim3((unsigned)(((size_t)w * h + 255) / 256)), dim3(256), stream, plane, pitch, x0, y0, w, h, max_bits);
}

// May a layout take the 16-byte stores (host side)?  The vector of a full group sits at base + (y sy + x0) elements,
// x0 a multiple of P = 16 / elem: 16-byte aligned if the base is and sy is a multiple of P.
static inline bool emit_map_wide(const void* data, size_t elem, long long sy, long long sx) {
  return sx == 1 && ((uintptr_t)data & 15u) == 0 && sy % (long long)(16 / elem) == 0;
}
// k_emit_map<T> in the instantiation whose store path the layout may take (host side).
template <class T>
static inline void launch_emit_map(hipStream_t stream, const float* map, int w, int h, int pitch, T* out, long long sy, long long sx) {
  constexpr int P = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256)), block(256);
  if (emit_map_wide(out, sizeof(T), sy, sx)) {
    GZ_LAUNCH((k_emit_map<T, true>), grid, block, stream, map, w, h, pitch, out, sy, sx);
  } else {
    GZ_LAUNCH((k_emit_map<T, false>), grid, block, stream, map, w, h, pitch, out, sy, sx);
  }
}

}  // namespace gz
