// Device-resident masking images (gz_mask_device, gz_adaptive_quantization): the second half of Mask()
// (butteraugli.cc:1780-1816) per pixel -- mask_p0p1 and the four interp_lut512 look-ups of combine_px
// (gz_kernels_diff.h), in its casts and order -- fused with the conversion and the strided store of k_emit_map
// (gz_kernels_emitmap.h).  It reads the three blurred planes of the first half (mask_x_blur, mask_y_blur1,
// mask_y_blur2, `pitch` floats per row) and writes up to six elements per pixel straight into the caller's tensors:
// no mask plane exists in between.
//
// What a launch writes (MODE):
//   kEmitMask      mask[0..2]                      kEmitMaskDc   mask_dc[0..2]
//   kEmitMaskBoth  all six                         kEmitMaskY    mask[1] alone, into a 2-D image: the quantisation field
// kEmitMaskY reads the two Y blurs alone: plane 1 of the mask does not depend on the X blur (p1 of mask_p0p1).
// Element rule: emit_map_value's -- float32 bit for bit, float16 / bfloat16 rounded to nearest even over the whole
// float32 domain.
#pragma once
#include "gz_common.h"
#include "gz_kernels_diff.h"
#include "gz_kernels_emitmap.h"

namespace gz {

enum { kEmitMask = 1, kEmitMaskDc = 2, kEmitMaskBoth = 3, kEmitMaskY = 4 };

// A destination: element (y, x, c) is data[y * sy + x * sx + c * sc], strides in elements (the CALLER has checked that no
// two elements share an address).  kEmitMaskY: `mask` is the 2-D image, its sc is not read.
template <class T>
struct EmitMaskDst {
  T* data;
  long long sy, sx, sc;
};
template <class T>
struct EmitMaskArgs {
  const float* mask_x_blur;    // blur(diffX, 9.24); not read by kEmitMaskY
  const float* mask_y_blur1;   // blur(diffY, 2.377)
  const float* mask_y_blur2;   // blur(diffY, 9.04)
  const double* luts;          // [4][512]: MaskX, MaskY, MaskDcX, MaskDcY
  EmitMaskDst<T> mask, dc;
  unsigned wide;               // bit c: plane c of mask, bit 3 + c: plane c of dc may take 16-byte stores (emit_mask_wide_bits)
};

// One group of a plane, k_emit_map's store: ONE 16-byte store for a full group where the plane's layout allows it,
// element by element otherwise and for the partial group at the end of a row.
template <class T>
GZ_DEVFN void emit_mask_store(const float* f, int n, T* dst, long long sx, bool wide) {
  constexpr int P = 16 / (int)sizeof(T);
  if (wide && n == P) {
    if constexpr (sizeof(T) == 4) {
      gz_f4 v;
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

// P consecutive floats of a plane row: 16-byte loads where `vec` (a full group whose first float is 16-byte aligned).
template <int P>
GZ_DEVFN void emit_mask_load(const float* src, int n, bool vec, float* f) {
  if (vec) {
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
}

// Lanes and pixels as in k_emit_map: one lane takes P = 16 / sizeof(T) consecutive pixels of one row, consecutive lanes
// consecutive groups, rows follow each other.  No path writes an element other than the (y, x, c) it converts.
template <class T, int MODE>
__global__ __launch_bounds__(256) void k_emit_mask(EmitMaskArgs<T> a, int w, int h, int pitch) {
  constexpr int P = 16 / (int)sizeof(T);
  constexpr bool kX = MODE != kEmitMaskY;
  constexpr bool kM = (MODE & kEmitMask) != 0, kDc = (MODE & kEmitMaskDc) != 0;
  const unsigned gpr = (unsigned)(w + P - 1) / P;                  // groups per row
  const unsigned g = blockIdx.x * 256u + threadIdx.x;              // (gpr * h <= 16384 * 65535)
  if (g >= gpr * (unsigned)h) return;
  const int y = (int)(g / gpr), x0 = (int)(g - (unsigned)y * gpr) * P;
  const int n = w - x0 < P ? w - x0 : P;
  const size_t at = (size_t)y * pitch + x0;
  const float *s1 = a.mask_y_blur1 + at, *s2 = a.mask_y_blur2 + at;
  const float* s0 = kX ? a.mask_x_blur + at : s1;   // (the Y-only mode does not look at the X blur)
  const bool vec = n == P && ((((uintptr_t)s0 | (uintptr_t)s1) | (uintptr_t)s2) & 15u) == 0;
  float bx[P], by1[P], by2[P];
  if (kX) emit_mask_load<P>(s0, n, vec, bx);
  emit_mask_load<P>(s1, n, vec, by1);
  emit_mask_load<P>(s2, n, vec, by2);
  const double w_ytob_hf = 0.086624184478, w_ytob_lf = 21.6804277046;   // (combine_px)
  if (MODE == kEmitMaskY) {
    float m1[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      double p0, p1;
      mask_p0p1(0.0f, by1[i], by2[i], &p0, &p1);   // (p1 does not depend on the X blur)
      m1[i] = (float)interp_lut512(a.luts + 512, p1);
    }
    emit_mask_store(m1, n, a.mask.data + ((long long)y * a.mask.sy + (long long)x0 * a.mask.sx), a.mask.sx, (a.wide & 1u) != 0);
    return;
  }
  float m[3][P], d[3][P];   // (the half a MODE does not write is never computed: the loop is unrolled, the arrays are registers)
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double p0, p1;
    mask_p0p1(bx[i], by1[i], by2[i], &p0, &p1);
    if (kM) {
      m[0][i] = (float)interp_lut512(a.luts, p0);
      const double my = interp_lut512(a.luts + 512, p1);
      m[1][i] = (float)my;
      m[2][i] = (float)(w_ytob_hf * my);
    }
    if (kDc) {
      d[0][i] = (float)interp_lut512(a.luts + 1024, p0);
      const double mdcy = interp_lut512(a.luts + 1536, p1);
      d[1][i] = (float)mdcy;
      d[2][i] = (float)(w_ytob_lf * mdcy);
    }
  }
  if (kM) {
    T* dst = a.mask.data + ((long long)y * a.mask.sy + (long long)x0 * a.mask.sx);
#pragma unroll
    for (int c = 0; c < 3; ++c) emit_mask_store(m[c], n, dst + (long long)c * a.mask.sc, a.mask.sx, ((a.wide >> c) & 1u) != 0);
  }
  if (kDc) {
    T* dst = a.dc.data + ((long long)y * a.dc.sy + (long long)x0 * a.dc.sx);
#pragma unroll
    for (int c = 0; c < 3; ++c) emit_mask_store(d[c], n, dst + (long long)c * a.dc.sc, a.dc.sx, ((a.wide >> (3 + c)) & 1u) != 0);
  }
}

// Which of a destination's `planes` planes may take the 16-byte stores (host side): emit_map_wide's condition at each
// plane's own base, data + c * sc.
static inline unsigned emit_mask_wide_bits(const void* data, size_t elem, long long sy, long long sx, long long sc, int planes) {
  unsigned bits = 0;
  for (int c = 0; c < planes; ++c)
    if (emit_map_wide((const char*)data + (size_t)c * (size_t)sc * elem, elem, sy, sx)) bits |= 1u << c;
  return bits;
}

// k_emit_mask<T, MODE> on `stream` (host side); a.wide is filled in here.
template <class T, int MODE>
static inline void launch_emit_mask(hipStream_t stream, EmitMaskArgs<T> a, int w, int h, int pitch) {
  constexpr int P = 16 / (int)sizeof(T);
  a.wide = 0;
  if (MODE == kEmitMaskY) a.wide = emit_mask_wide_bits(a.mask.data, sizeof(T), a.mask.sy, a.mask.sx, 0, 1);
  if (MODE & kEmitMask) a.wide |= emit_mask_wide_bits(a.mask.data, sizeof(T), a.mask.sy, a.mask.sx, a.mask.sc, 3);
  if (MODE & kEmitMaskDc) a.wide |= emit_mask_wide_bits(a.dc.data, sizeof(T), a.dc.sy, a.dc.sx, a.dc.sc, 3) << 3;
  const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256)), block(256);
  GZ_LAUNCH((k_emit_mask<T, MODE>), grid, block, stream, a, w, h, pitch);
}

}  // namespace gz
