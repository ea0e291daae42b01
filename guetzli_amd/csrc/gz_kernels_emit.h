// Device-resident output (gz_decode_coeffs_device / gz_reconstruct_device): the packed 8-bit image k_reconstruct* write
// (srgb, rgb[(y * w + x) * 3 + c]) becomes a strided w x h x 3 image of uint8, uint16, float32, float16 or bfloat16
// elements in the caller's device memory -- k_ingest_rgb (gz_kernels_ingest.h) with the directions swapped.
//
// The element of a byte b:
//   uint8     b
//   uint16    b * 257: the high byte is b (and so is the low one), ingest's v >> 8 gives b back
//   float32   (float)b / 255.0f, the IEEE division -- NOT b * (1 / 255.f), which is another float for 126 of the 256
//             bytes.  The 256 quotients come from the HOST (emit_lut below) and are staged in LDS, as s_lut is.
//   float16, bfloat16   that float32 rounded to nearest, ties to even, with integer operations on its bits: the
//             emulation build runs the same source without a half type.
// Every rule satisfies ingest_byte(emit(b)) == b for all 256 bytes.
#pragma once
#include "gz_common.h"
#include "gz_kernels_ingest.h"

namespace gz {

// float32 -> the 16-bit floats, round to nearest even.  The domain is the table's: 0 and [1 / 255, 1] -- normal numbers
// of both formats (1 / 255 > 2^-14), no overflow, no NaN; the carry of a rounding runs into the exponent by itself.
GZ_DEVFN uint16_t emit_f16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if (u == 0u) return (uint16_t)0;
  return (uint16_t)(((u + 0xfffu + ((u >> 13) & 1u)) >> 13) - (112u << 10));   // bias 127 -> 15
}
GZ_DEVFN uint16_t emit_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// s_lut: the staged table (only the three float types read it)
GZ_DEVFN void emit_value(uint8_t b, const float*, uint8_t* out) { *out = b; }
GZ_DEVFN void emit_value(uint8_t b, const float*, uint16_t* out) { *out = (uint16_t)(b * 257u); }
GZ_DEVFN void emit_value(uint8_t b, const float* s_lut, float* out) { *out = s_lut[b]; }
GZ_DEVFN void emit_value(uint8_t b, const float* s_lut, ingest_f16* out) { out->bits = emit_f16_bits(s_lut[b]); }
GZ_DEVFN void emit_value(uint8_t b, const float* s_lut, ingest_bf16* out) { out->bits = emit_bf16_bits(s_lut[b]); }

template <class T> struct emit_reads_lut { static constexpr bool value = true; };
template <> struct emit_reads_lut<uint8_t> { static constexpr bool value = false; };
template <> struct emit_reads_lut<uint16_t> { static constexpr bool value = false; };

// Element (y, x, c) is data[y * sy + x * sx + c * sc] (strides in elements, > 0 wherever they count, 64-bit offsets;
// the CALLER has checked that no two of the w * h * 3 elements share an address).  Lanes and pixels as in k_ingest_rgb:
// one lane takes P = 16 / sizeof(T) consecutive pixels of one row, consecutive lanes consecutive groups, rows follow
// each other.  The lane's 3 P bytes are read as dwords when their first byte is dword-aligned (every group when w is a
// multiple of 4), byte by byte otherwise.  A full group is stored as 16-byte vectors (global_store_dwordx4) where the
// layout allows it -- WIDE, a template parameter chosen by the CALLER (ingest_wide_mode: it also needs the base address
// and the byte strides the vectors move by to be multiples of 16), one store path per instantiation:
//   kIngestPlanarRows       sx == 1: one vector per channel (CHW rows, crops of them)
//   kIngestInterleavedRows  sc == 1, sx == 3: the group's 3 P consecutive elements as three vectors (HWC rows, crops)
//   kIngestElementwise      element by element, as the partial group at the end of a row is in every instantiation
// No path writes an element other than the (y, x, c) it converts: the destination may be a crop inside a larger
// tensor, and its neighbours stay as they are.
// B... (empty, or one EmitBatch): the batched form, gridDim.y = the images of the launch -- image j is packed image
// arena[j] of the scratch (rgb_stride bytes apart) and image slot[j] of the caller's tensor (stride_n elements apart);
// WIDE is the caller's word for every one of them.
struct EmitBatch {
  const int* arena;
  const int* slot;
  size_t rgb_stride;
  long long stride_n;
};
template <class T, int WIDE, class... B>
__global__ __launch_bounds__(256) void k_emit_rgb(const uint8_t* __restrict__ rgb, int w, int h, T* __restrict__ data,
                                                  long long sy, long long sx, long long sc,
                                                  const float* __restrict__ lut, B... batch) {
  static_assert(WIDE == kIngestElementwise || WIDE == kIngestPlanarRows || WIDE == kIngestInterleavedRows, "k_emit_rgb: an unknown store path");
  constexpr int P = 16 / (int)sizeof(T);
  if constexpr (sizeof...(B) > 0) {
    const EmitBatch eb = (batch, ...);
    rgb += (size_t)eb.arena[blockIdx.y] * eb.rgb_stride;
    data += (long long)eb.slot[blockIdx.y] * eb.stride_n;
  }
  __shared__ float s_lut[256];
  if constexpr (emit_reads_lut<T>::value) {   // (every thread of the block gets here)
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  const unsigned gpr = (unsigned)(w + P - 1) / P;                  // groups per row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;              // (gpr * h <= 16384 * 65535)
  if (g >= gpr * (unsigned)h) return;
  const int y = (int)(g / gpr), x0 = (int)(g - (unsigned)y * gpr) * P;
  const int n = w - x0 < P ? w - x0 : P;
  const uint8_t* src = rgb + ((size_t)y * w + x0) * 3;
  uint8_t b[3 * P];
  if (n == P && ((uintptr_t)src & 3u) == 0) {
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
#pragma unroll
    for (int j = 0; j < 3 * P / 4; ++j) {
      const uint32_t v = src4[j];
      b[4 * j] = (uint8_t)v; b[4 * j + 1] = (uint8_t)(v >> 8); b[4 * j + 2] = (uint8_t)(v >> 16); b[4 * j + 3] = (uint8_t)(v >> 24);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3 * P; ++j) b[j] = j < 3 * n ? src[j] : (uint8_t)0;
  }
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

// The float32 elements of the 256 bytes, by the host's IEEE division.
static inline const float* emit_lut() {
  static const struct Table {
    float v[256];
    Table() { for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f; }
  } t;
  return t.v;
}

// k_emit_rgb<T> in the instantiation whose store path the layout may take (host side).  The vectors sit where
// k_ingest_rgb's do, so the conditions are ingest_wide_mode's.
template <class T>
static inline void launch_emit_rgb(hipStream_t stream, const uint8_t* rgb, int w, int h, T* data, long long sy, long long sx,
                                   long long sc, const float* lut) {
  constexpr int P = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256)), block(256);
  switch (ingest_wide_mode(data, sizeof(T), sy, sx, sc)) {
    case kIngestPlanarRows:
      GZ_LAUNCH((k_emit_rgb<T, kIngestPlanarRows>), grid, block, stream, rgb, w, h, data, sy, sx, sc, lut);
      break;
    case kIngestInterleavedRows:
      GZ_LAUNCH((k_emit_rgb<T, kIngestInterleavedRows>), grid, block, stream, rgb, w, h, data, sy, sx, sc, lut);
      break;
    default:
      GZ_LAUNCH((k_emit_rgb<T, kIngestElementwise>), grid, block, stream, rgb, w, h, data, sy, sx, sc, lut);
      break;
  }
}
// The batched form: `count` images, image j from packed image arena[j] into image slot[j] of the tensor.  The 16-byte
// stores need every image's base aligned: the first one's, and stride_n a multiple of the vector's elements.
template <class T>
static inline void launch_emit_rgb_batch(hipStream_t stream, const uint8_t* rgb, int w, int h, T* data, long long sn, long long sy,
                                         long long sx, long long sc, const float* lut, const int* arena, const int* slot, int count,
                                         size_t rgb_stride) {
  constexpr int P = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256), (unsigned)count), block(256);
  const EmitBatch eb = {arena, slot, rgb_stride, sn};
  switch (sn % P == 0 ? ingest_wide_mode(data, sizeof(T), sy, sx, sc) : (int)kIngestElementwise) {
    case kIngestPlanarRows:
      GZ_LAUNCH((k_emit_rgb<T, kIngestPlanarRows, EmitBatch>), grid, block, stream, rgb, w, h, data, sy, sx, sc, lut, eb);
      break;
    case kIngestInterleavedRows:
      GZ_LAUNCH((k_emit_rgb<T, kIngestInterleavedRows, EmitBatch>), grid, block, stream, rgb, w, h, data, sy, sx, sc, lut, eb);
      break;
    default:
      GZ_LAUNCH((k_emit_rgb<T, kIngestElementwise, EmitBatch>), grid, block, stream, rgb, w, h, data, sy, sx, sc, lut, eb);
      break;
  }
}

}  // namespace gz
