// C ABI: butteraugli of LINEAR float images -- ButteraugliInterface (butteraugli.h:44-79, butteraugli.cc:1819-1878) on
// the device.  A strided image of float32 / float16 / bfloat16 elements in device memory goes into the context's three
// linear planes through k_ingest_linear (gz_kernels_ingestlin.h) -- no byte image, no table -- as a context's original
// (gz_create_from_device_linear, gz_set_linear_device) or as the other image of a pair (gz_compare_device_linear);
// gz_butteraugli_linear is the whole function on a context that lives for the call, from 1 x 1 up.
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

// A linear image and how it reaches the planes: w x h is the image's own size; with `extended` the planes are the
// canvas of ButteraugliDiffmap's rule for images under 8 pixels (ext; gz_kernels_ingestlin.h).
struct LinearSource {
  const gz_device_pixels* img;
  float scale;
  int w, h;
  bool extended;
  IngestExtent ext;
};

extern "C" {

// The arguments alone: no device call (the library answers these without a GPU).
static int check_linear_pixels(const gz_device_pixels* img, int w, int h, float scale) {
  if (check_device_pixels(img, w, h) != GZ_OK) return GZ_E_ARG;
  if (!tensor_float_dtype(img->dtype) || img->alpha) return GZ_E_ARG;
  if (!(scale > 0.0f && scale < INFINITY)) return GZ_E_ARG;   // (NaN fails every comparison)
  return GZ_OK;
}

// ButteraugliDiffmap's border (butteraugli.cc:1830-1833): (8 - size) / 2 in integers under 8 pixels, else 0.
static LinearSource linear_source(const gz_device_pixels* img, float scale, int w, int h) {
  LinearSource s;
  s.img = img; s.scale = scale; s.w = w; s.h = h;
  s.extended = w < 8 || h < 8;
  s.ext.src_w = w; s.ext.src_h = h;
  s.ext.xborder = w < 8 ? (8 - w) / 2 : 0;
  s.ext.yborder = h < 8 ? (8 - h) / 2 : 0;
  return s;
}

// (the image's own extent: the extension reads no element outside it)
static int check_linear_pointer(int device, const LinearSource* src, std::string* why) {
  return check_tensor_memory(device, tensor_view(src->img, src->w, src->h), "data", why);
}

// k_ingest_linear on `stream`: src -> the three planes of a cw x ch canvas (the image's own size unless extended),
// counting into *altered, which a fill on `stream` clears first.
static hipError_t ingest_linear(hipStream_t stream, const LinearSource* src, int cw, int ch, float* lin, int pitch, size_t pstride,
                                unsigned* altered) {
  const hipError_t e = hipMemsetAsync(altered, 0, sizeof(unsigned), stream);
  if (e != hipSuccess) return e;
  const gz_device_pixels* img = src->img;
  const long long sy = img->stride_y, sx = img->stride_x, sc = img->stride_c;
  const IngestExtent* ext = src->extended ? &src->ext : nullptr;
  with_float_type(img->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    launch_ingest_linear(stream, (const T*)img->data, sy, sx, sc, cw, ch, src->scale, ext, lin, pitch, pstride, altered);
  });
  return hipSuccess;
}

// (the context's device is current, src has passed check_linear_pixels and check_linear_pointer)
// set_rgb_device's drops; and the context is a linear one from the first write on: d_rgb stays the OLD original's, which
// pi0 no longer is, so the entries that read it must refuse whether this call succeeds or not.
static int set_linear_device(gz_ctx* c, const LinearSource* src) {
  c->lin_is_cand = c->xyb_is_cand = false;
  c->have_block_mask = c->have_distmap = false;
  c->orig_linear = true;
  c->orig_clamped = 0;
  TRY(wait_for_producer(c, src->img->producer_stream));
  void* res = nullptr;
  TRY(result_buffer(c, sizeof(unsigned), &res));
  unsigned* altered = c->d_max_bits + gz_ctx::kWordClamped;
  HIPCHK(c, ingest_linear(c->stream, src, c->w, c->h, c->lin[0], c->pitch, c->plane, altered));
  KCHK(c);
  HIPCHK(c, hipMemcpyAsync(res, altered, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  TRY(original_from_lin(c));   // (its synchronise: the source is read, and the count has landed, when the call returns)
  c->orig_clamped = *(const unsigned*)res;
  return GZ_OK;
}

gz_ctx* gz_create_from_device_linear(int device, int w, int h, const gz_device_pixels* img, float scale, int* err) {
  if (check_linear_pixels(img, w, h, scale) != GZ_OK || w < 8 || h < 8) {   // (before any device call)
    if (err) *err = GZ_E_ARG;
    return nullptr;
  }
  const LinearSource src = linear_source(img, scale, w, h);
  CallerDevice keep(device);
  return create_context(device, w, h, nullptr, nullptr, 1.0f, err, &src);
}

int gz_set_linear_device(gz_ctx* c, const gz_device_pixels* img, float scale) {
  if (!c) return GZ_E_ARG;
  if (check_linear_pixels(img, c->w, c->h, scale) != GZ_OK) return GZ_E_ARG;   // (before any device call)
  const LinearSource src = linear_source(img, scale, c->w, c->h);
  DeviceScope ds_(c);
  if (const int rc = check_linear_pointer(c->device, &src, &c->err)) return rc;
  if (c->pending.busy() || c->scan_pending) { c->err = "gz_set_linear_device while work of the context is in flight"; return GZ_E_STATE; }
  return set_linear_device(c, &src);
}

// compare_device_pixels (entry_pair.h) with k_ingest_linear in place of launch_ingest.  src: the other image, of the
// context's size or -- extended -- of the size the context's canvas was made for; win: that image's window of the planes.
static int compare_device_linear(gz_ctx* c, const LinearSource* src, float* distance, const gz_device_map* map, const HeatRequest* heat,
                                 uint64_t* clamped, const char* who) {
  const MapWindow window = {src->ext.xborder, src->ext.yborder, src->w, src->h};
  const MapWindow* win = src->extended ? &window : nullptr;
  if (const int rc = check_linear_pointer(c->device, src, &c->err)) return rc;
  if (map)
    if (const int rc = check_tensor_memory(c->device, tensor_view(map, src->w, src->h), "map", &c->err)) return rc;
  if (heat)
    if (const int rc = check_tensor_memory(c->device, tensor_view(heat->out, src->w, src->h), "heat", &c->err)) return rc;
  TRY(pair_compare_state(c, who));
  pair_compare_drops(c);
  TRY(wait_for_producer(c, src->img->producer_stream));
  HIPCHK(c, ingest_linear(c->stream, src, c->w, c->h, c->lin[0], c->pitch, c->plane, c->d_max_bits + gz_ctx::kWordClamped));
  KCHK(c);
  const LinearTail tail = {win, clamped};
  return pair_compare_tail(c, distance, map, nullptr, heat, &tail);   // (its synchronise: `other` is read when the call returns)
}

int gz_compare_device_linear(gz_ctx* c, const gz_device_pixels* other, float scale, float* distance, const gz_device_map* map,
                             const gz_device_output* heat, double good, double bad, uint64_t* clamped) {
  if (!c || !distance) return GZ_E_ARG;
  if (check_linear_pixels(other, c->w, c->h, scale) != GZ_OK) return GZ_E_ARG;   // (before any device call)
  if (map && check_device_map(map, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  const HeatRequest req{heat, good, bad};
  if (heat && check_heat_request(req, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  const LinearSource src = linear_source(other, scale, c->w, c->h);   // (a context is 8 x 8 at the least: never extended)
  DeviceScope ds_(c);
  return compare_device_linear(c, &src, distance, map, heat ? &req : nullptr, clamped, "gz_compare_device_linear");
}

int gz_butteraugli_linear(int device, int w, int h, const gz_device_pixels* ref, const gz_device_pixels* other, float scale,
                          float* distance, const gz_device_map* map, const gz_device_output* heat, double good, double bad,
                          uint64_t* clamped) {
  if (!distance) return GZ_E_ARG;   // (all of these before any device call)
  if (check_linear_pixels(ref, w, h, scale) != GZ_OK || check_linear_pixels(other, w, h, scale) != GZ_OK) return GZ_E_ARG;
  if (map && check_device_map(map, w, h) != GZ_OK) return GZ_E_ARG;
  const HeatRequest req{heat, good, bad};
  if (heat && check_heat_request(req, w, h) != GZ_OK) return GZ_E_ARG;
  const LinearSource src0 = linear_source(ref, scale, w, h), src1 = linear_source(other, scale, w, h);
  CallerDevice keep(device);
  int rc = GZ_OK;
  const CallContext ctx(create_context(device, w < 8 ? 8 : w, h < 8 ? 8 : h, nullptr, nullptr, 1.0f, &rc, &src0));
  if (!ctx.c) return rc;
  uint64_t altered = 0;
  rc = compare_device_linear(ctx.c, &src1, distance, map, heat ? &req : nullptr, &altered, "gz_butteraugli_linear");
  if (rc == GZ_OK && clamped) *clamped = ctx.c->orig_clamped + altered;   // (of both images)
  return rc;
}

#ifndef GZ_NO_PROBES
int gz_probe_linear_planes(gz_ctx* c, float* planes3) {
  DeviceScope ds_(c);
  if (!c || !planes3) return GZ_E_ARG;
  if (c->pending.busy()) { c->err = "gz_probe_linear_planes while a Compare or phase-B work of the context is in flight"; return GZ_E_STATE; }
  for (int i = 0; i < 3; ++i) TRY(download_plane(c, c->lin[i], planes3 + (size_t)i * c->w * c->h));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}
#endif  // GZ_NO_PROBES

}  // extern "C"
