// C ABI: butteraugli's masking on the device -- OpsinDynamicsImage (gz_opsin_device), Mask (gz_mask_device;
// butteraugli.cc:1741-1817) and ButteraugliAdaptiveQuantization (gz_adaptive_quantization, :1880-1901) of device-resident
// images, written into the caller's strided device tensors.  Context-free: a context lives for the call (create_context
// with the first image as its original, which also computes that image's psycho image -- nothing here reads it), the
// work runs on its main stream, the results leave through k_emit_map (the opsin planes) and k_emit_mask
// (gz_kernels_emitmask.h: the second half of Mask fused with the store -- no mask plane, no probe arena).
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

namespace {

// The arguments alone: no device call (the library answers these without a GPU).
static int check_float_output(const gz_device_output* out, int w, int h) {
  if (check_device_output(out, w, h) != GZ_OK) return GZ_E_ARG;
  return tensor_float_dtype(out->dtype) ? GZ_OK : GZ_E_ARG;
}
static int check_sampled_pixels(const gz_device_pixels* img, int w, int h, int samples, float scale) {
  if (samples == GZ_SAMPLES_SRGB8) return check_device_pixels(img, w, h);
  if (samples == GZ_SAMPLES_LINEAR) return check_linear_pixels(img, w, h, scale);
  return GZ_E_ARG;
}

// A context whose original is `img` read as `samples` say: lin[] holds its linear planes, xyb[] their opsin image.
// *clamped: the elements the linear reader altered (0 for 8-bit samples).
static gz_ctx* sampled_context(int device, int w, int h, const gz_device_pixels* img, int samples, float scale, int* rc,
                               unsigned long long* clamped) {
  gz_ctx* c;
  if (samples == GZ_SAMPLES_LINEAR) {
    const LinearSource src = linear_source(img, scale, w, h);
    c = create_context(device, w, h, nullptr, nullptr, 1.0f, rc, &src);
  } else {
    c = create_context(device, w, h, nullptr, img, 1.0f, rc);
  }
  *clamped = c ? c->orig_clamped : 0;
  return c;
}

// k_emit_mask<T, MODE> for the element type of the destinations (one type for both: gz_mask_device converts a second
// type in a second launch).
template <int MODE, class T>
static void launch_mask_of_type(gz_ctx* c, const gz_device_output* mask, const gz_device_output* dc, const gz_device_map* y) {
  EmitMaskArgs<T> a;
  memset(&a, 0, sizeof(a));
  a.mask_x_blur = c->mxb; a.mask_y_blur1 = c->myb1; a.mask_y_blur2 = c->myb2;
  a.luts = c->d_mask_luts;
  if (mask) a.mask = {(T*)mask->data, mask->stride_y, mask->stride_x, mask->stride_c};
  if (dc) a.dc = {(T*)dc->data, dc->stride_y, dc->stride_x, dc->stride_c};
  if (y) a.mask = {(T*)y->data, y->stride_y, y->stride_x, 0};
  launch_emit_mask<T, MODE>(c->stream, a, c->w, c->h, c->pitch);
}
template <int MODE>
static void launch_mask(gz_ctx* c, int dtype, const gz_device_output* mask, const gz_device_output* dc, const gz_device_map* y) {
  with_float_type(dtype, [&](auto tag) { launch_mask_of_type<MODE, typename decltype(tag)::type>(c, mask, dc, y); });
}

// Two scratch planes for image 0's half of DiffPrecompute: Malta's outputs, which nothing here computes.
static float* const* mask_sup_planes(gz_ctx* c) { return c->ac; }

// xyb[] holds the opsin image of image 0; img1 (may be NULL: image 0 again) is read behind its half of DiffPrecompute.
static int mask_on_context(gz_ctx* c, const gz_device_pixels* img1, int samples, float scale, const gz_device_output* mask,
                           const gz_device_output* dc, unsigned long long* clamped) {
  const hipStream_t stream = c->stream;
  for (const gz_device_output* o : {mask, dc})
    if (o)
      if (const int rc = check_tensor_memory(c->device, tensor_view(o, c->w, c->h), "data", &c->err)) return rc;
  if (img1)
    if (const int rc = check_tensor_memory(c->device, tensor_view(img1, c->w, c->h), "data", &c->err)) return rc;
  MaskPrePack pk;
  {
    MaskIn in0[2];
    for (int i = 0; i < 2; ++i) {
      in0[i] = {nullptr, c->xyb[i], 0.0, 1.0, 1};
      pk.in1[i] = {nullptr, c->xyb[i], 0.0, 1.0, 1};   // (read behind the second image's opsin kernel, when there is one)
      pk.sup0[i] = mask_sup_planes(c)[i];
    }
    pk.out[0] = c->diffx; pk.out[1] = c->diffy;
    TRY(stage_mask_sup(c, stream, in0, mask_sup_planes(c)));
  }
  const unsigned* altered = nullptr;
  if (img1) {
    TRY(wait_for_producer(c, img1->producer_stream));
    if (samples == GZ_SAMPLES_LINEAR) {
      const LinearSource src = linear_source(img1, scale, c->w, c->h);
      void* res = nullptr;
      TRY(result_buffer(c, sizeof(unsigned), &res));
      HIPCHK(c, ingest_linear(stream, &src, c->w, c->h, c->lin[0], c->pitch, c->plane, c->d_max_bits + gz_ctx::kWordClamped));
      KCHK(c);
      HIPCHK(c, hipMemcpyAsync(res, c->d_max_bits + gz_ctx::kWordClamped, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
      altered = (const unsigned*)res;
    } else {
      launch_ingest(stream, tensor_view(img1, c->w, c->h), img1->background, c->w, c->h, c->d_srgb_out, c->d_srgb_lut, c->lin[0], c->pitch, c->plane);
      KCHK(c);
    }
    TRY(stage_opsin(c, stream));
  }
  TRY(stage_mask_blurs(c, stream, stream, pk));
  TRY(outputs_after_consumers(c, stream, &c->ev_emit, {mask ? mask->consumer_stream : nullptr, dc ? dc->consumer_stream : nullptr}));
  if (mask && dc && mask->dtype == dc->dtype) {
    launch_mask<kEmitMaskBoth>(c, mask->dtype, mask, dc, nullptr);
  } else {
    if (mask) launch_mask<kEmitMask>(c, mask->dtype, mask, nullptr, nullptr);
    if (dc) launch_mask<kEmitMaskDc>(c, dc->dtype, nullptr, dc, nullptr);
  }
  KCHK(c);
  TRY(consumers_after_outputs(c, stream, c->ev_emit, {mask ? mask->consumer_stream : nullptr, dc ? dc->consumer_stream : nullptr}));
  HIPCHK(c, hipStreamSynchronize(stream));   // (the context's memory goes back to the pool behind this)
  if (altered) *clamped += *altered;
  return GZ_OK;
}

// lin[] holds the image's linear planes: Mask(rgb, rgb)'s plane 1 (ButteraugliAdaptiveQuantization passes the linear
// planes as xyb0 and xyb1) -- the Y half of DiffPrecompute in slot 0 of one-plane launches, its radius-5 blur and ONE
// radius-20 pass pair, then the Y-only emit.  Nothing of the X plane runs.
static int quant_on_context(gz_ctx* c, const gz_device_map* quant) {
  const hipStream_t stream = c->stream;
  if (const int rc = check_tensor_memory(c->device, tensor_view(quant, c->w, c->h), "map", &c->err)) return rc;
  const MaskIn y = {nullptr, c->lin[1], 0.0, 1.0, 1};
  const dim3 grid(gz_div_up(c->w, 1024), c->h, 1);
  {
    MaskSupPack pk;
    pk.in[0] = pk.in[1] = y;
    pk.out[0] = pk.out[1] = mask_sup_planes(c)[1];
    GZ_LAUNCH(k_mask_sup, grid, dim3(256), stream, pk, c->w, c->h, c->pitch);
    KCHK(c);
  }
  {
    MaskPrePack pk;
    pk.in1[0] = pk.in1[1] = y;
    pk.sup0[0] = pk.sup0[1] = mask_sup_planes(c)[1];
    pk.out[0] = pk.out[1] = c->diffy;
    GZ_LAUNCH(k_mask_pre, grid, dim3(256), stream, pk, c->w, c->h, c->pitch);
    KCHK(c);
  }
  {
    SrcPack<SrcPlain, 1> s; s.s[0].p = c->diffy;
    PostStore<1> post; post.out[0] = c->myb1;
    TRY((blur2d<5, 1, SrcPlain, PostStore<1>>(c, stream, s, post, c->blur[B_MASKY0])));
  }
  {
    SrcPack<SrcPlain, 1> s; PlanePack<1> t; CPlanePack<1> ct;
    s.s[0].p = c->diffy; t.p[0] = c->tmp[2]; ct.p[0] = c->tmp[2];
    TRY((blur_h<20, SrcPlain, 1>(c, stream, s, t, c->blur[B_MASKY1])));
    PostStore<1> post; post.out[0] = c->myb2;
    TRY((blur_v<20, 1, PostStore<1>>(c, stream, ct, post, c->blur[B_MASKY1])));
  }
  TRY(outputs_after_consumers(c, stream, &c->ev_emit, {quant->consumer_stream}));
  launch_mask<kEmitMaskY>(c, quant->dtype, nullptr, nullptr, quant);
  KCHK(c);
  TRY(consumers_after_outputs(c, stream, c->ev_emit, {quant->consumer_stream}));
  HIPCHK(c, hipStreamSynchronize(stream));   // (the context's memory goes back to the pool behind this)
  return GZ_OK;
}

// xyb[] -> the three planes of `out`, each through k_emit_map at its own base.
static int opsin_on_context(gz_ctx* c, const gz_device_output* out) {
  const TensorView v = tensor_view(out, c->w, c->h);
  if (const int rc = check_tensor_memory(c->device, v, "data", &c->err)) return rc;
  TRY(outputs_after_consumers(c, c->stream, &c->ev_emit, {out->consumer_stream}));
  for (int i = 0; i < 3; ++i) {
    launch_map(c->stream, c->xyb[i], c->w, c->h, c->pitch, tensor_select(v, 2, i));
    KCHK(c);
  }
  TRY(consumers_after_outputs(c, c->stream, c->ev_emit, {out->consumer_stream}));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (the context's memory goes back to the pool behind this)
  return GZ_OK;
}

}  // namespace

extern "C" {

int gz_opsin_device(int device, int w, int h, const gz_device_pixels* img, int samples, float scale, const gz_device_output* xyb,
                    uint64_t* clamped) {
  if (w < 8 || h < 8) return GZ_E_ARG;   // (all of these before any device call)
  if (check_sampled_pixels(img, w, h, samples, scale) != GZ_OK || check_float_output(xyb, w, h) != GZ_OK) return GZ_E_ARG;
  CallerDevice keep(device);
  int rc = GZ_OK;
  unsigned long long altered = 0;
  const CallContext ctx(sampled_context(device, w, h, img, samples, scale, &rc, &altered));
  if (ctx.c) rc = opsin_on_context(ctx.c, xyb);
  if (rc == GZ_OK && clamped) *clamped = altered;
  return rc;
}

int gz_mask_device(int device, int w, int h, const gz_device_pixels* img0, const gz_device_pixels* img1, int samples, float scale,
                   const gz_device_output* mask, const gz_device_output* mask_dc, uint64_t* clamped) {
  if (w < 8 || h < 8 || (!mask && !mask_dc)) return GZ_E_ARG;   // (all of these before any device call)
  if (check_sampled_pixels(img0, w, h, samples, scale) != GZ_OK) return GZ_E_ARG;
  if (img1 && check_sampled_pixels(img1, w, h, samples, scale) != GZ_OK) return GZ_E_ARG;
  if (mask && check_float_output(mask, w, h) != GZ_OK) return GZ_E_ARG;
  if (mask_dc && check_float_output(mask_dc, w, h) != GZ_OK) return GZ_E_ARG;
  CallerDevice keep(device);
  int rc = GZ_OK;
  unsigned long long altered = 0;
  const CallContext ctx(sampled_context(device, w, h, img0, samples, scale, &rc, &altered));
  if (ctx.c) rc = mask_on_context(ctx.c, img1, samples, scale, mask, mask_dc, &altered);
  if (rc == GZ_OK && clamped) *clamped = altered;   // (of both images)
  return rc;
}

int gz_adaptive_quantization(int device, int w, int h, const gz_device_pixels* img, float scale, const gz_device_map* quant,
                             uint64_t* clamped) {
  if (w < 16 || h < 16) return GZ_E_ARG;   // (the reference returns false; all of these before any device call)
  if (check_linear_pixels(img, w, h, scale) != GZ_OK || check_device_map(quant, w, h) != GZ_OK) return GZ_E_ARG;
  CallerDevice keep(device);
  int rc = GZ_OK;
  unsigned long long altered = 0;
  const CallContext ctx(sampled_context(device, w, h, img, GZ_SAMPLES_LINEAR, scale, &rc, &altered));
  if (ctx.c) rc = quant_on_context(ctx.c, quant);
  if (rc == GZ_OK && clamped) *clamped = altered;
  return rc;
}

}  // extern "C"
