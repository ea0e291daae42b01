// C ABI: library and context life cycle (gz_create / gz_set_rgb / gz_destroy, pools, streams).
// (part of the one translation unit gz_api.hip, which includes these files in order; split by
// concern in round 5 -- no declaration here is visible outside libguetzli_amd.so but the C ABI)
#pragma once

// The element type of a dtype as a tag: f(TypeTag<T>()) -- for the five sample types of pixels and outputs, and for the
// three float types of maps and linear images (a family that takes floats only instantiates nothing else).
template <class T> struct TypeTag { using type = T; };
template <class F> static void with_sample_type(int dtype, F&& f) {
  switch (dtype) {
    case GZ_DT_U8: f(TypeTag<uint8_t>()); break;
    case GZ_DT_F32: f(TypeTag<float>()); break;
    case GZ_DT_F16: f(TypeTag<ingest_f16>()); break;
    case GZ_DT_BF16: f(TypeTag<ingest_bf16>()); break;
    default: f(TypeTag<uint16_t>()); break;
  }
}
template <class F> static void with_float_type(int dtype, F&& f) {
  switch (dtype) {
    case GZ_DT_F32: f(TypeTag<float>()); break;
    case GZ_DT_F16: f(TypeTag<ingest_f16>()); break;
    default: f(TypeTag<ingest_bf16>()); break;
  }
}

extern "C" {


int gz_abi_version(void) { return 6; }

int gz_config_from_environment(gz_config* out) {
  if (!out) return GZ_E_ARG;
  gz_config c;
  memset(&c, 0, sizeof(c));
  c.struct_size = (int)sizeof(gz_config);
  c.blur_packed = -1;
  c.single_stream = -1;
  if (const char* e = getenv("GZ_BLUR_PK")) c.blur_packed = atoi(e) != 0;
  if (const char* e = getenv("GZ_TILE_ROWS")) { const int v = atoi(e); if (v == 16 || v == 32) c.tile_rows = v; }
  if (const char* e = getenv("GZ_SINGLE_STREAM")) c.single_stream = atoi(e) != 0;
  if (const char* e = getenv("GZ_STORE_DISTMAP")) c.store_distmap = atoi(e) != 0;
  c.patch_reconstruct = 1;
  if (const char* e = getenv("GZ_PATCH_RECON")) { const int v = atoi(e); if (v >= 0 && v <= 2) c.patch_reconstruct = v; }
  c.opsin_ahead = 1;
  if (const char* e = getenv("GZ_OPSIN_AHEAD")) c.opsin_ahead = atoi(e) != 0;
  *out = c;
  return GZ_OK;
}
int gz_get_config(const gz_ctx* c, gz_config* out) {
  if (!c || !out) return GZ_E_ARG;
  *out = c->cfg;
  return GZ_OK;
}
int gz_set_config(gz_ctx* c, const gz_config* in) {
  if (!c || !in || in->struct_size != (int)sizeof(gz_config)) return GZ_E_ARG;
  if (in->blur_packed < -1 || in->blur_packed > 1 || in->single_stream < -1 || in->single_stream > 1 || (in->tile_rows != 0 && in->tile_rows != 16 && in->tile_rows != 32) ||
      in->patch_reconstruct < 0 || in->patch_reconstruct > 2)
    return GZ_E_ARG;
  if (c->pending.busy() || c->scan_pending) {
    c->err = "gz_set_config while work of the context is in flight";
    return GZ_E_STATE;
  }
  c->cfg = *in;
  c->lin_is_cand = c->xyb_is_cand = false;
  return GZ_OK;
}

static std::atomic<int>& images_in_flight_hint() { static std::atomic<int> v{0}; return v; }
void gz_hint_images_in_flight(int n) {
  images_in_flight_hint().store(n, std::memory_order_relaxed);
  if (n > 1) {
    // company is coming: idle stream sets with a priority main stream go (a priority stream is one more hardware
    // queue for the runtime to multiplex, even while nobody uses it)
    StreamSetPool& sp = stream_set_pool();
    std::lock_guard<std::mutex> lk(sp.mu);
    for (auto it = sp.sets.begin(); it != sp.sets.end();) {
      if (it->first & 1) { stream_set_teardown(it->second); it = sp.sets.erase(it); }
      else ++it;
    }
  }
}

int gz_device_pci_bus_id(int device, char* out, int cap) {
  if (!out || cap < 16) return GZ_E_ARG;
#ifdef GZ_EMU
  (void)device;
  snprintf(out, (size_t)cap, "0000:00:00.0");
  return GZ_OK;
#else
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void)hipGetLastError(); return GZ_E_NO_DEVICE; }
  if (hipDeviceGetPCIBusId(out, cap, device) != hipSuccess) { (void)hipGetLastError(); return GZ_E_HIP; }
  return GZ_OK;
#endif
}

int gz_trim_pool(void) {
  {
    MemPool& p = dev_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    pool_release_idle(p, false, -1);
  }
  {
    MemPool& h = host_pool();
    std::lock_guard<std::mutex> lk(h.mu);
    pool_release_idle(h, true, -1);
  }
  {
    StreamSetPool& sp = stream_set_pool();
    std::lock_guard<std::mutex> lk(sp.mu);
    for (auto& kv : sp.sets) stream_set_teardown(kv.second);
    sp.sets.clear();
  }
  HandlePool& hp = handle_pool();
  std::lock_guard<std::mutex> lk(hp.mu);
  for (auto& kv : hp.events) (void)hipEventDestroy(kv.second);
  hp.events.clear();
  return GZ_OK;
}

int gz_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return GZ_E_NO_DEVICE;
  return n;
}

const char* gz_strerror(int code) {
  switch (code) {
    case GZ_OK: return "ok";
    case GZ_E_ARG: return "invalid argument";
    case GZ_E_NO_DEVICE: return "no usable HIP device";
    case GZ_E_HIP: return "HIP runtime error";
    case GZ_E_STATE: return "invalid call sequence";
    case GZ_E_NOMEM: return "out of memory";
    default: return "unknown error";
  }
}

const char* gz_last_error(const gz_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }

// ---- the stream contracts of the callers' tensors ----
// An input's producer_stream: c->stream goes on behind what the producer has enqueued so far, without waiting for it on
// the host.
static int wait_for_producer(gz_ctx* c, void* producer) {
  if (!producer) return GZ_OK;
  if (!c->ev_ingest) TRY(own_event(c, &c->ev_ingest));
  HIPCHK(c, hipEventRecord(c->ev_ingest, (hipStream_t)producer));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ingest, 0));
  return GZ_OK;
}
// An output's consumer_stream, around the emit kernels on `stream`, with the event `ev`:
// before: `stream` waits for what the consumer's stream has been given so far (a caching allocator may have handed the
// memory out while earlier work of that stream still uses it); behind: the consumer's stream waits for the kernels.
static hipError_t emit_after_consumer(hipStream_t stream, hipEvent_t ev, void* consumer) {
  const hipError_t e = hipEventRecord(ev, (hipStream_t)consumer);
  return e != hipSuccess ? e : hipStreamWaitEvent(stream, ev, 0);
}
static hipError_t consumer_after_emit(hipStream_t stream, hipEvent_t ev, void* consumer) {
  const hipError_t e = hipEventRecord(ev, stream);
  return e != hipSuccess ? e : hipStreamWaitEvent((hipStream_t)consumer, ev, 0);
}
// ... for every consumer of `consumers` that is one (NULL: none).  *ev: the holder's slot for the event -- a context's
// ev_emit, a DecodeScratch's ev -- entered into c's record when the first consumer needs it, unless it is there already
// (a caller that emits in several rounds makes it in front of them).
static int outputs_after_consumers(gz_ctx* c, hipStream_t stream, hipEvent_t* ev, std::initializer_list<void*> consumers) {
  for (void* s : consumers) {
    if (!s) continue;
    if (!*ev) TRY(own_event(c, ev));
    HIPCHK(c, emit_after_consumer(stream, *ev, s));
  }
  return GZ_OK;
}
static int consumers_after_outputs(gz_ctx* c, hipStream_t stream, hipEvent_t ev, std::initializer_list<void*> consumers) {
  for (void* s : consumers)
    if (s) HIPCHK(c, consumer_after_emit(stream, ev, s));
  return GZ_OK;
}

// ---- device-resident input (gz_kernels_ingest.h) ----
// (the arguments alone -- check_device_pixels and its siblings, pixels_of_image: tensor.h)
// Where the memory lives: it must be readable by `device` (the current one).  An ordinary host pointer, memory of
// another GPU or an extent that leaves its allocation is an argument error here, not a fault in the kernel.
// `last` = the offset of the last element read from p, `what` = "data" or "alpha".
static int check_device_range(int device, const void* p, uint64_t last, size_t elem, const char* what, std::string* why) {
#ifndef GZ_EMU
  const std::string name = std::string("device image: ") + what;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    if (why) *why = name + " is not memory the HIP runtime knows (a host pointer?)";
    return GZ_E_ARG;
  }
  const bool readable = (at.type == hipMemoryTypeDevice && at.device == device) || at.type == hipMemoryTypeManaged ||
                        (at.type == hipMemoryTypeHost && at.devicePointer == p);
  if (!readable) {
    if (why) *why = at.type == hipMemoryTypeDevice ? name + " lives on device " + std::to_string(at.device) + ", the context on " + std::to_string(device)
                                                   : name + " is not device-readable memory (a host pointer?)";
    return GZ_E_ARG;
  }
  if (at.type == hipMemoryTypeDevice) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) {
      const uint64_t room = (uint64_t)((const char*)base + size - (const char*)p) / elem;
      if (last >= room) {
        if (why) *why = name + ": the strides lead outside the allocation that holds it";
        return GZ_E_ARG;
      }
    } else {
      (void)hipGetLastError();
    }
  }
#else
  (void)device; (void)p; (void)last; (void)elem; (void)what; (void)why;
#endif
  return GZ_OK;
}
// ... for a view: its data and, where it has one, its alpha.  `what` names the data in gz_last_error.
static int check_tensor_memory(int device, const TensorView& v, const char* what, std::string* why) {
  const size_t elem = tensor_elem_size(v.dtype);
  if (const int rc = check_device_range(device, v.data, tensor_last(v, v.nd), elem, what, why)) return rc;
  return v.alpha ? check_device_range(device, v.alpha, tensor_last(v, v.alpha_nd), elem, "alpha", why) : GZ_OK;
}

// The ingest kernel on `stream`: img (y, x, c: w x h x 3, checked by the caller) -> rgb [h][w][3] and, with lin != nullptr,
// the three linear planes.  Opaque pixels take k_ingest_rgb, pixels with alpha -- over `background`, gz_device_pixels' --
// k_ingest_rgba: same grid, one launch either way.
static void launch_ingest(hipStream_t stream, const TensorView& img, const uint8_t* background, int w, int h, uint8_t* rgb,
                          const float* lut, float* lin, int pitch, size_t pstride) {
  const size_t elem = tensor_elem_size(img.dtype);
  const long long sy = img.dim[0].stride, sx = img.dim[1].stride, sc = img.dim[2].stride;
  const int per_lane = (int)(16 / elem);
  const dim3 grid((unsigned)(((size_t)gz_div_up(w, per_lane) * h + 255) / 256)), block(256);
  with_sample_type(img.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (img.alpha) {
      const unsigned bg = (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16);
      launch_ingest_rgba(stream, grid, block, (const T*)img.data, (const T*)img.alpha, sy, sx, sc, w, h, bg, rgb, lut, lin, pitch, pstride);
    } else {
      const int wide = ingest_wide_mode(img.data, elem, sy, sx, sc);
      GZ_LAUNCH((k_ingest_rgb<T>), grid, block, stream, (const T*)img.data, sy, sx, sc, w, h, wide, rgb, lut, lin, pitch, pstride);
    }
  });
}

static int set_rgb_device(gz_ctx* c, const gz_device_pixels* img);
// (entry_linear.h: a linear float image as the original -- what it is, where its memory must live, its arrival)
struct LinearSource;
static int check_linear_pointer(int device, const LinearSource* src, std::string* why);
static int set_linear_device(gz_ctx* c, const LinearSource* src);
static gz_ctx* create_context(int device, int w, int h, const uint8_t* rgb, const gz_device_pixels* img, float target, int* err,
                              const LinearSource* linear = nullptr, int batch_arenas = 0);
gz_ctx* gz_create(int device, int w, int h, const uint8_t* rgb, float target, int* err) {
  CallerDevice keep(device);
  return create_context(device, w, h, rgb, nullptr, target, err);
}
gz_ctx* gz_create_from_device_pixels(int device, int w, int h, const gz_device_pixels* img, float target, int* err) {
  if (check_device_pixels(img, w, h) != GZ_OK) {   // (before any device call)
    if (err) *err = GZ_E_ARG;
    return nullptr;
  }
  CallerDevice keep(device);
  return create_context(device, w, h, nullptr, img, target, err);
}
gz_ctx* gz_create_from_device(int device, int w, int h, const gz_device_image* img, float target, int* err) {
  gz_device_pixels px;
  if (pixels_of_image(img, &px) != GZ_OK) {
    if (err) *err = GZ_E_ARG;
    return nullptr;
  }
  return gz_create_from_device_pixels(device, w, h, &px, target, err);
}
// The original from host pixels (rgb), from a device-resident image (img, checked by the caller) or from a linear float
// image (linear, checked by the caller; w x h is then the canvas it is extended to): one of the three.
// Or none of them, with batch_arenas > 0 (entry_batch.h): a context without an original, whose arena is that many images'
// arenas back to back (batch_arena_stride() apart) and, behind them, one result word per image -- one allocation.  Its
// plane pointers are the first arena's; the coefficient buffers, which nothing of a pixel comparison touches, stay empty.
static gz_ctx* create_context(int device, int w, int h, const uint8_t* rgb, const gz_device_pixels* img, float target, int* err,
                              const LinearSource* linear, int batch_arenas) {
  int dummy;
  if (!err) err = &dummy;
  *err = GZ_OK;
  if ((!rgb && !img && !linear && batch_arenas <= 0) || w < 8 || h < 8 || w >= (1 << 16) || h >= (1 << 16)) { *err = GZ_E_ARG; return nullptr; }
  // coefficient positions (3 x blocks x 64) and candidate offsets (blocks x 189) are 32-bit
  // on both sides of the ABI: 11.18 M blocks = 715 MPix is the largest image (tested: 268 MPix)
  if ((uint64_t)((w + 7) / 8) * (uint64_t)((h + 7) / 8) * 192u > 0x7fffffffull) { *err = GZ_E_ARG; return nullptr; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev ||
      hipSetDevice(device) != hipSuccess) {
    *err = GZ_E_NO_DEVICE;
    return nullptr;
  }
  if (img && check_tensor_memory(device, tensor_view(img, w, h), "data", nullptr) != GZ_OK) { *err = GZ_E_ARG; return nullptr; }
  if (linear && check_linear_pointer(device, linear, nullptr) != GZ_OK) { *err = GZ_E_ARG; return nullptr; }
  gz_ctx* c = new gz_ctx;
  c->device = device;
  c->w = w; c->h = h;
  c->bw = (w + 7) / 8; c->bh = (h + 7) / 8; c->nb = c->bw * c->bh;
  c->pitch = w;
  c->plane = (size_t)c->pitch * h;
  c->target = target;
  (void)gz_config_from_environment(&c->cfg);
  set_frame(c, 1);
  auto fail = [&](int code) { *err = code; gz_destroy(c); return (gz_ctx*)nullptr; };
#define CHK0(call) do { const hipError_t e0_ = (call); if (e0_ != hipSuccess) { (void)hipGetLastError(); return fail(e0_ == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP); } } while (0)
  // The chain's main stream takes the device's highest priority, so that the dispatcher serves
  // its workgroups before those of the entropy coder that runs beside it (1080p encode 0.144 ->
  // 0.140 s) -- but only for a context that has the device to itself when it is created, and no
  // stream ever goes BELOW the default: with several images in flight priorities invert (an
  // image's low-priority entropy coder starves behind the other images' chains while its host
  // thread waits for it: 16 x 1080p, 8 in flight, 21.8 -> 7.5-13.5 MPix/s with main = highest and
  // entropy = lowest on every context; profiles/r03_stream_priorities.log).
  int taken_before = 0;
  c->slot = slot_take(device, &taken_before);
  c->prio_streams = taken_before == 0 && images_in_flight_hint().load(std::memory_order_relaxed) <= 1;
  {
    StreamSet ss;
    // The contexts alive on a device take slots (lowest free first) and slot s gets a stream set whose MAIN stream
    // sits on hardware queue s mod 4: four images in flight then have their main streams on four different queues
    // whatever order the images before them finished in (handed out by availability, two mains could share a queue:
    // the "40 or 44-46 MPix/s" of a 4K batch from process to process; 16 x 1080p 35.4 -> 39.7 MPix/s, 12 x 1440p 38.9 ->
    // 40.2, 8 x 4K 42.4 -> 43.6, nothing at 1 MPix and below: r06_chain_experiments.log, section 12).
    const hipError_t se = pool_stream_set_create(&ss, c->prio_streams, c->slot % 4);
    c->own_stream = ss.own; c->side_stream = ss.side; c->side_stream2 = ss.side2; c->entropy_stream = ss.entropy;
    c->stream = c->own_stream;
    CHK0(se);
  }
  for (hipEvent_t* e : {&c->ev_candidate, &c->ev_fork, &c->ev_join, &c->ev_join2, &c->ev_mask_pre, &c->ev_next_cand, &c->ev_xyb, &c->ev_lfy})
    if (const int rc = own_event(c, e)) return fail(rc);
  const size_t ncoef = batch_arenas > 0 ? 1 : (size_t)3 * c->nb * 64;
  const size_t arena_bytes = batch_arenas > 0 ? (sizeof(float) * batch_arena_stride(c->plane) + sizeof(unsigned)) * (size_t)batch_arenas
                                              : sizeof(float) * c->plane * kNumPlanes;
  if (const int rc = regrow(c, nullptr, nullptr, 0,
                            {{(void**)&c->d_rgb, (size_t)3 * w * h}, {(void**)&c->d_orig, ncoef * 2}, {(void**)&c->d_cand, ncoef * 2},
                             {(void**)&c->d_q, sizeof(int) * 192}, {(void**)&c->d_srgb_lut, sizeof(float) * 256},
                             {(void**)&c->d_mask_luts, sizeof(double) * 2048}, {(void**)&c->d_block_max, sizeof(float) * c->nb},
                             {(void**)&c->d_max_bits, sizeof(unsigned) * gz_ctx::kResultWords}, {(void**)&c->d_srgb_out, (size_t)3 * w * h},
                             {(void**)&c->arena, arena_bytes}}))
    return fail(rc);
  for (int i = kNumPlanes - 1; i >= 0; --i) c->free_planes.push_back(c->arena + (size_t)i * c->plane);
  alloc_psycho(c, &c->pi0);
  alloc_psycho(c, &c->pi1);
  for (int i = 0; i < 3; ++i) { c->lin[i] = take_plane(c); }
  for (int i = 0; i < 3; ++i) { c->tmp[i] = take_plane(c); }
  for (int i = 0; i < 3; ++i) { c->xyb[i] = take_plane(c); }
  for (int i = 0; i < 2; ++i) { c->lf_raw[i] = take_plane(c); c->hfp[i] = take_plane(c); }
  c->snb = take_plane(c); c->diffx = take_plane(c); c->diffy = take_plane(c);
  c->mxb = take_plane(c); c->myb1 = take_plane(c); c->myb2 = take_plane(c);
  c->ac[0] = take_plane(c); c->ac[1] = take_plane(c);
  c->dsq = take_plane(c); c->distmap = take_plane(c);
  c->sup0[0] = take_plane(c); c->sup0[1] = take_plane(c);
  // lin planes must be contiguous for k_reconstruct / k_linear_from_rgb8 (plane stride)
  if (c->lin[1] != c->lin[0] + c->plane || c->lin[2] != c->lin[0] + 2 * c->plane) return fail(GZ_E_STATE);

  // tables
  {
    // Srgb8ToLinearTable (gamma_correct.cc:23-38), then float() as LinearRgb /
    // ToLinearRGB store it (butteraugli_comparator.cc:42, output_image.cc:434).
    float lut[256];
    int i = 0;
    for (; i < 11; ++i) lut[i] = (float)(i / 12.92);
    for (; i < 256; ++i) lut[i] = (float)(255.0 * pow(((i / 255.0) + 0.055) / 1.055, 2.4));
    CHK0(hipMemcpy(c->d_srgb_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
    std::vector<double> ml(2048);
    make_mask_lut(2.59885507073, 3.08805636789, 5.62939030582, 0.315424196682, 16.2770141832, &ml[0]);
    make_mask_lut(0.9613705131, -0.581933100068, 6.64307621174, 1.00846207765, 2.2342321176, &ml[512]);
    make_mask_lut(10.0470705878, 3.18472654033, 0.373092999662, 0.0551512255218, 70.0, &ml[1024]);
    make_mask_lut(0.0115640939227, 45.9483175519, 2.52611324247, 0.0142290066313, 5.0, &ml[1536]);
    CHK0(hipMemcpy(c->d_mask_luts, ml.data(), sizeof(double) * 2048, hipMemcpyHostToDevice));
  }
  for (int b = 0; b < B_COUNT; ++b) {
    // Blur(in, float sigma, float border_ratio): both narrowed to float at the call.
    int rc = setup_blur_cfg(c, &c->blur[b], (float)kBlurSpecs[b].sigma, (float)kBlurSpecs[b].border, true);
    if (rc != GZ_OK) return fail(rc);
    if (c->blur[b].r != kBlurSpecs[b].r) return fail(GZ_E_STATE);
  }
  if (linear || img || rgb) {
    const int rc = linear ? set_linear_device(c, linear) : img ? set_rgb_device(c, img) : gz_set_rgb(c, rgb);
    if (rc != GZ_OK) return fail(rc);
  }
#undef CHK0
  return c;
}

// What follows the original's arrival in d_rgb and lin[], from the host or from the device:
// pi0_ = SeparateFrequencies(OpsinDynamicsImage(LinearRgb(rgb))), the original's half of every Compare's DiffPrecompute,
// and the wait for all of it.
static int original_from_lin(gz_ctx* c) {
  TRY(stage_opsin(c, c->stream));
  TRY(stage_separate(c, chain_streams(c, false), &c->pi0));
  {
    MaskIn in0[2];
    mask_in_psycho(c->pi0, in0);
    TRY(stage_mask_sup(c, c->stream, in0, c->sup0));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

int gz_set_rgb(gz_ctx* c, const uint8_t* rgb) {
  DeviceScope ds_(c);
  if (!c || !rgb) return GZ_E_ARG;
  c->lin_is_cand = c->xyb_is_cand = false;   // (lin[] takes the original)
  c->have_block_mask = c->have_distmap = false;   // (StartBlockComparisons' mask and the map belong to the old one)
  HIPCHK(c, hipMemcpyAsync(c->d_rgb, rgb, (size_t)3 * c->w * c->h, hipMemcpyHostToDevice, c->stream));
  dim3 grid(gz_div_up(c->w, 256), c->h);
  GZ_LAUNCH(k_linear_from_rgb8, grid, dim3(256), c->stream, c->d_rgb, c->w, c->h, c->pitch,
            c->plane, c->d_srgb_lut, c->lin[0]);
  KCHK(c);
  TRY(original_from_lin(c));
  c->orig_linear = false;   // (d_rgb is the original's again)
  return GZ_OK;
}

// (the context's device is current, img has passed check_device_pixels and check_tensor_memory)
static int set_rgb_device(gz_ctx* c, const gz_device_pixels* img) {
  c->lin_is_cand = c->xyb_is_cand = false;
  c->have_block_mask = c->have_distmap = false;
  TRY(wait_for_producer(c, img->producer_stream));
  launch_ingest(c->stream, tensor_view(img, c->w, c->h), img->background, c->w, c->h, c->d_rgb, c->d_srgb_lut, c->lin[0], c->pitch, c->plane);
  KCHK(c);
  TRY(original_from_lin(c));   // (its synchronise: the source is read when the call returns)
  c->orig_linear = false;      // (d_rgb is the original's again)
  return GZ_OK;
}

int gz_set_rgb_device_pixels(gz_ctx* c, const gz_device_pixels* img) {
  if (!c) return GZ_E_ARG;
  if (check_device_pixels(img, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  DeviceScope ds_(c);
  if (const int rc = check_tensor_memory(c->device, tensor_view(img, c->w, c->h), "data", &c->err)) return rc;
  return set_rgb_device(c, img);
}
int gz_set_rgb_device(gz_ctx* c, const gz_device_image* img) {
  gz_device_pixels px;
  if (!c || pixels_of_image(img, &px) != GZ_OK) return GZ_E_ARG;
  return gz_set_rgb_device_pixels(c, &px);
}

void gz_destroy(gz_ctx* c) {
  if (!c) return;
  DeviceScope ds_(c);   // the pools file what comes back under the current device
  // everything must be idle before the memory goes back to the pool (another context may get
  // it at once; hipFree would have waited, the pool does not)
  if (c->stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->stream);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
  if (c->side_stream2) (void)hipStreamSynchronize(c->side_stream2);
  if (c->entropy_stream) (void)hipStreamSynchronize(c->entropy_stream);
  release_owned(c);
  // (the side and entropy streams a second time: nothing was enqueued since the first, so it waits for nothing -- it stays
  // because the recorded enqueue order of a context's life, tests/golden/enqueue_order/create_and_set_rgb.txt, holds it)
  for (hipStream_t s : {c->side_stream, c->side_stream2, c->entropy_stream}) if (s) (void)hipStreamSynchronize(s);
  {   // the four streams go back as the set they were made as (own_stream: synchronised at the top of gz_destroy)
    StreamSet ss;
    ss.own = c->own_stream; ss.side = c->side_stream; ss.side2 = c->side_stream2; ss.entropy = c->entropy_stream;
    pool_stream_set_destroy(ss, c->prio_streams, c->slot % 4);
  }
  if (c->slot >= 0) slot_release(c->device, c->slot);
  delete c;
}

int gz_synchronize(gz_ctx* c) {
  DeviceScope ds_(c);
  if (!c) return GZ_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

int gz_set_stream(gz_ctx* c, void* s) {
  DeviceScope ds_(c);
  if (!c) return GZ_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return GZ_OK;
}


}  // extern "C"
