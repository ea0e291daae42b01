// A caller's strided device tensor as the entries see it: ONE internal view of the seven ABI structs (gz_device_image,
// gz_device_pixels, gz_device_output, gz_device_map, gz_device_batch, gz_device_map_batch, gz_device_output_batch), the arithmetic on it -- the
// extent rule, the distinct-addresses rule, the last offset -- and one adapter per struct.
// Host code without a device call and without a gz_ctx: tests/cpp/tensor_args.cc compiles this file alone.
// (in gz_api.hip: included behind context.h)
#pragma once

// ---------------------------------------------------------------- the arithmetic ----
// (nothing but these three headers)
#include <stdint.h>

#include <algorithm>
#include <utility>

namespace {

// Element (i0, i1, ...) is data[i0 * dim[0].stride + i1 * dim[1].stride + ...], strides in ELEMENTS; the dimensions
// outermost first: (n,) y, x (, c).
struct TensorDim {
  int64_t stride, count;
};
struct TensorView {
  void* data = nullptr;
  int dtype = 0;
  int nd = 0;
  TensorDim dim[4] = {{0, 1}, {0, 1}, {0, 1}, {0, 1}};
  void* alpha = nullptr;   // a second base (gz_device_pixels' alpha; NULL: none) over the first alpha_nd dimensions:
  int alpha_nd = 0;        // data's extent without the channel term
  void* stream = nullptr;  // the producer's (inputs) or the consumer's (outputs) hipStream_t; NULL: none
};

constexpr uint64_t kTensorLimit = ((uint64_t)1 << 62) - 1;

// The offset of the last element of the first nd dimensions (nd = v.nd: data's; nd = v.alpha_nd: alpha's).  Of a view
// that has passed tensor_extent_ok: below 2^62.
inline uint64_t tensor_last(const TensorView& v, int nd) {
  uint64_t last = 0;
  for (int i = 0; i < nd; ++i) last += (uint64_t)v.dim[i].stride * (uint64_t)(v.dim[i].count - 1);
  return last;
}

// The last element's offset in 62 bits: every term is bounded before it is formed, and so is their sum.  A negative
// stride and a dimension without an element fail too (nothing below could be formed from them).
inline bool tensor_extent_ok(const TensorView& v) {
  uint64_t last = 0;
  for (int i = 0; i < v.nd; ++i) {
    if (v.dim[i].stride < 0 || v.dim[i].count < 1) return false;
    const uint64_t s = (uint64_t)v.dim[i].stride, steps = (uint64_t)v.dim[i].count - 1;
    if (steps > 0 && s > kTensorLimit / steps) return false;
    last += s * steps;   // (both <= the limit < 2^62)
    if (last > kTensorLimit) return false;
  }
  return true;
}

// No two elements at one address.  Sufficient, not necessary: the dimensions ordered by stride, each stride at least the
// extent stride * count of the one before -- and at least 1: a stride of 0, a convenience of the input side, would make
// a kernel's lanes write one element in turns.  A dimension of one element addresses nothing: its stride does not
// count.  (of a view that has passed tensor_extent_ok: stride * count <= 2^63, no overflow)
inline bool tensor_distinct(const TensorView& v) {
  std::pair<uint64_t, uint64_t> dim[4];
  for (int i = 0; i < v.nd; ++i) dim[i] = {(uint64_t)v.dim[i].stride, (uint64_t)v.dim[i].count};
  std::sort(dim, dim + v.nd);
  uint64_t least = 1;
  for (int i = 0; i < v.nd; ++i) {
    if (dim[i].second == 1) continue;
    if (dim[i].first < least) return false;
    least = dim[i].first * dim[i].second;
  }
  return true;
}

}  // namespace

// ---------------------------------------------------------------- the ABI structs ----
#include <string.h>

#include "../../../include/guetzli_amd.h"

namespace {

inline size_t tensor_elem_size(int dtype) { return dtype == GZ_DT_U8 ? 1 : dtype == GZ_DT_F32 ? 4 : 2; }
inline bool tensor_float_dtype(int dtype) { return dtype == GZ_DT_F32 || dtype == GZ_DT_F16 || dtype == GZ_DT_BF16; }

// Element `index` of dimension `d`: the base (and alpha's, where alpha has that dimension) moves, the dimension goes.
inline TensorView tensor_select(TensorView v, int d, int64_t index) {
  const size_t bytes = (size_t)index * (size_t)v.dim[d].stride * tensor_elem_size(v.dtype);
  v.data = (char*)v.data + bytes;
  if (v.alpha && d < v.alpha_nd) v.alpha = (char*)v.alpha + bytes;
  if (d < v.alpha_nd) --v.alpha_nd;
  for (int i = d; i + 1 < v.nd; ++i) v.dim[i] = v.dim[i + 1];
  v.dim[--v.nd] = {0, 1};
  return v;
}

// The views.  (the struct is not NULL; what it says is not checked yet)
inline TensorView tensor_view(const gz_device_pixels* p, int w, int h) {
  TensorView v;
  v.data = const_cast<void*>(p->data); v.dtype = p->dtype; v.nd = 3;
  v.dim[0] = {p->stride_y, h}; v.dim[1] = {p->stride_x, w}; v.dim[2] = {p->stride_c, 3};
  v.alpha = const_cast<void*>(p->alpha); v.alpha_nd = 2;
  v.stream = p->producer_stream;
  return v;
}
inline TensorView tensor_view(const gz_device_output* p, int w, int h) {
  TensorView v;
  v.data = p->data; v.dtype = p->dtype; v.nd = 3;
  v.dim[0] = {p->stride_y, h}; v.dim[1] = {p->stride_x, w}; v.dim[2] = {p->stride_c, 3};
  v.stream = p->consumer_stream;
  return v;
}
inline TensorView tensor_view(const gz_device_map* p, int w, int h) {
  TensorView v;
  v.data = p->data; v.dtype = p->dtype; v.nd = 2;
  v.dim[0] = {p->stride_y, h}; v.dim[1] = {p->stride_x, w};
  v.stream = p->consumer_stream;
  return v;
}
inline TensorView tensor_view(const gz_device_batch* p, int w, int h, int n) {
  TensorView v;
  v.data = const_cast<void*>(p->data); v.dtype = p->dtype; v.nd = 4;
  v.dim[0] = {p->stride_n, n}; v.dim[1] = {p->stride_y, h}; v.dim[2] = {p->stride_x, w}; v.dim[3] = {p->stride_c, 3};
  v.stream = p->producer_stream;
  return v;
}
inline TensorView tensor_view(const gz_device_output_batch* p, int w, int h) {
  TensorView v;
  v.data = p->data; v.dtype = p->dtype; v.nd = 4;
  v.dim[0] = {p->stride_n, p->n}; v.dim[1] = {p->stride_y, h}; v.dim[2] = {p->stride_x, w}; v.dim[3] = {p->stride_c, 3};
  v.stream = p->consumer_stream;
  return v;
}
inline TensorView tensor_view(const gz_device_map_batch* p, int w, int h, int n) {
  TensorView v;
  v.data = p->data; v.dtype = p->dtype; v.nd = 3;
  v.dim[0] = {p->stride_n, n}; v.dim[1] = {p->stride_y, h}; v.dim[2] = {p->stride_x, w};
  v.stream = p->consumer_stream;
  return v;
}

// The arguments alone: no device call (the library answers these without a GPU).  What is specific to a struct -- its
// size, the element types it takes, whether it is written (then no two elements may share an address; an input may
// repeat one with a stride of 0) -- is the adapter's; the rules are the view's.
inline int tensor_check(const TensorView& v, int dtype_first, int dtype_last, bool written) {
  if (!v.data || v.dtype < dtype_first || v.dtype > dtype_last) return GZ_E_ARG;
  if (!tensor_extent_ok(v) || (written && !tensor_distinct(v))) return GZ_E_ARG;
  return GZ_OK;
}
inline bool tensor_plane_size(int w, int h) { return w > 0 && h > 0 && w < (1 << 16) && h < (1 << 16); }

inline int check_device_pixels(const gz_device_pixels* img, int w, int h) {
  if (!img || img->struct_size != (int)sizeof(gz_device_pixels) || !tensor_plane_size(w, h)) return GZ_E_ARG;
  return tensor_check(tensor_view(img, w, h), GZ_DT_U8, GZ_DT_U16, false);
}
inline int check_device_output(const gz_device_output* out, int w, int h) {
  if (!out || out->struct_size != (int)sizeof(gz_device_output) || !tensor_plane_size(w, h)) return GZ_E_ARG;
  return tensor_check(tensor_view(out, w, h), GZ_DT_U8, GZ_DT_U16, true);
}
inline int check_device_map(const gz_device_map* map, int w, int h) {
  if (!map || map->struct_size != (int)sizeof(gz_device_map) || !tensor_plane_size(w, h)) return GZ_E_ARG;
  return tensor_check(tensor_view(map, w, h), GZ_DT_F32, GZ_DT_BF16, true);
}
// The images of a batch are n gz_device_pixels without alpha and without GZ_DT_U16.
inline int check_device_batch(const gz_device_batch* b, int w, int h, int n) {
  if (!b || b->struct_size != (int)sizeof(gz_device_batch) || !tensor_plane_size(w, h)) return GZ_E_ARG;
  return tensor_check(tensor_view(b, w, h, n), GZ_DT_U8, GZ_DT_BF16, false);
}
// (w and h are the entry's to bound: gz_butteraugli_batch does, before it comes here)
inline int check_device_map_batch(const gz_device_map_batch* m, int w, int h, int n) {
  if (!m || m->struct_size != (int)sizeof(gz_device_map_batch)) return GZ_E_ARG;
  return tensor_check(tensor_view(m, w, h, n), GZ_DT_F32, GZ_DT_BF16, true);
}
// The images of an output batch are its n gz_device_outputs: every dtype of those, and no address twice among them all.
inline int check_device_output_batch(const gz_device_output_batch* b, int w, int h) {
  if (!b || b->struct_size != (int)sizeof(gz_device_output_batch) || !tensor_plane_size(w, h) || b->n < 1) return GZ_E_ARG;
  return tensor_check(tensor_view(b, w, h), GZ_DT_U8, GZ_DT_U16, true);
}
// gz_device_image is gz_device_pixels without alpha: what the three older entries accept stays what it was (their
// struct_size, no GZ_DT_U16), the rest is the code behind the newer ones.
inline int pixels_of_image(const gz_device_image* img, gz_device_pixels* px) {
  if (!img || img->struct_size != (int)sizeof(gz_device_image) || img->dtype > GZ_DT_BF16) return GZ_E_ARG;
  memset(px, 0, sizeof(*px));
  px->struct_size = (int)sizeof(*px);
  px->dtype = img->dtype;
  px->data = img->data;
  px->stride_y = img->stride_y; px->stride_x = img->stride_x; px->stride_c = img->stride_c;
  px->producer_stream = img->producer_stream;
  return GZ_OK;
}

}  // namespace
