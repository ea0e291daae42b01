// C ABI: context-free block transforms (gz_encode_rgb_only, double-precision DCT and its two users), the frame layout switch, OutputImage::Downsample (4:2:0; use_silver_screen on the device: silver_run, gz_downsample_silver).
// (part of the one translation unit gz_api.hip, which includes these files in order; split by
// concern in round 5 -- no declaration here is visible outside libguetzli_amd.so but the C ABI)
#pragma once

extern "C" {

static int probe_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev ||
      hipSetDevice(device) != hipSuccess)
    return GZ_E_NO_DEVICE;
  return GZ_OK;
}


// ----------------------------------------------------------- double-precision DCT ----
namespace {
struct DevBuf {   // scoped device allocation for the context-free entry points
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess; }
};
}  // namespace

int gz_encode_rgb_only(int device, const uint8_t* rgb, int w, int h, int16_t* coeffs_out) {
  if (!rgb || !coeffs_out || w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16)) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const int bw = (w + 7) / 8, bh = (h + 7) / 8, nb = bw * bh;
  DevBuf drgb, dco;
  if (!drgb.alloc((size_t)3 * w * h) || !dco.alloc((size_t)3 * nb * 128)) return GZ_E_NOMEM;
  if (hipMemcpy(drgb.p, rgb, (size_t)3 * w * h, hipMemcpyHostToDevice) != hipSuccess) return GZ_E_HIP;
  const uint8_t* d_rgb = (const uint8_t*)drgb.p;
  int16_t* d_co = (int16_t*)dco.p;
  GZ_LAUNCH(k_encode_rgb, dim3(gz_div_up(nb, kBlocksPerWG)), dim3(256), (hipStream_t)0, d_rgb, w, h,
            bw, nb, d_co);
  if (hipGetLastError() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(coeffs_out, dco.p, (size_t)3 * nb * 128, hipMemcpyDeviceToHost) != hipSuccess)
    return GZ_E_HIP;
  return GZ_OK;
}

int gz_pack_rgb_device_pixels(int device, const gz_device_pixels* img, int w, int h, uint8_t* host_rgb_out) {
  if (!host_rgb_out || check_device_pixels(img, w, h) != GZ_OK) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (check_tensor_memory(device, tensor_view(img, w, h), "data", nullptr) != GZ_OK) return GZ_E_ARG;
  DevBuf drgb;
  if (!drgb.alloc((size_t)3 * w * h)) return GZ_E_NOMEM;
  hipEvent_t ev = nullptr;
  if (img->producer_stream) {   // the null stream below waits for the producer on the device
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return GZ_E_HIP;
    const bool ok = hipEventRecord(ev, (hipStream_t)img->producer_stream) == hipSuccess &&
                    hipStreamWaitEvent((hipStream_t)0, ev, 0) == hipSuccess;
    if (!ok) { (void)hipEventDestroy(ev); return GZ_E_HIP; }
  }
  launch_ingest((hipStream_t)0, tensor_view(img, w, h), img->background, w, h, (uint8_t*)drgb.p, nullptr, nullptr, w, 0);
  const bool launched = hipGetLastError() == hipSuccess;
  // (a blocking copy on the null stream: behind the kernel, and complete when it returns)
  const bool copied = launched && hipMemcpy(host_rgb_out, drgb.p, (size_t)3 * w * h, hipMemcpyDeviceToHost) == hipSuccess;
  if (ev) (void)hipEventDestroy(ev);
  return copied ? GZ_OK : GZ_E_HIP;
}
int gz_pack_rgb_device(int device, const gz_device_image* img, int w, int h, uint8_t* host_rgb_out) {
  gz_device_pixels px;
  if (pixels_of_image(img, &px) != GZ_OK) return GZ_E_ARG;
  return gz_pack_rgb_device_pixels(device, &px, w, h, host_rgb_out);
}

int gz_dct_double_blocks(int device, double* blocks, int n, int inverse) {
  if (!blocks || n <= 0) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  DevBuf d;
  const size_t bytes = (size_t)n * 64 * sizeof(double);
  if (!d.alloc(bytes)) return GZ_E_NOMEM;
  if (hipMemcpy(d.p, blocks, bytes, hipMemcpyHostToDevice) != hipSuccess) return GZ_E_HIP;
  double* dblk = (double*)d.p;
  if (inverse) {
    GZ_LAUNCH((k_dctd_blocks<true>), dim3(gz_div_up(n, kBlocksPerWG)), dim3(256), (hipStream_t)0,
              dblk, n);
  } else {
    GZ_LAUNCH((k_dctd_blocks<false>), dim3(gz_div_up(n, kBlocksPerWG)), dim3(256), (hipStream_t)0,
              dblk, n);
  }
  if (hipGetLastError() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(blocks, d.p, bytes, hipMemcpyDeviceToHost) != hipSuccess) return GZ_E_HIP;
  return GZ_OK;
}

int gz_component_to_float_pixels(int device, const int16_t* coeffs, int w, int h, float* out) {
  if (!coeffs || !out || w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16)) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const int bw = (w + 7) / 8, bh = (h + 7) / 8, nb = bw * bh;
  DevBuf dc, dp;
  if (!dc.alloc((size_t)nb * 128) || !dp.alloc((size_t)w * h * sizeof(float))) return GZ_E_NOMEM;
  if (hipMemcpy(dc.p, coeffs, (size_t)nb * 128, hipMemcpyHostToDevice) != hipSuccess) return GZ_E_HIP;
  const int16_t* dcoef = (const int16_t*)dc.p;
  float* dpix = (float*)dp.p;
  GZ_LAUNCH(k_to_float_pixels, dim3(gz_div_up(nb, kBlocksPerWG)), dim3(256), (hipStream_t)0,
            dcoef, w, h, bw, nb, dpix);
  if (hipGetLastError() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(out, dp.p, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    return GZ_E_HIP;
  return GZ_OK;
}

int gz_component_set_downsampled(int device, const float* pixels, int w, int h, int fx, int fy,
                                 int16_t* coeffs_out) {
  if (!pixels || !coeffs_out || w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16) ||
      fx < 1 || fy < 1 || fx > 4 || fy > 4)
    return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const int bw = (w + 8 * fx - 1) / (8 * fx), bh = (h + 8 * fy - 1) / (8 * fy), nb = bw * bh;
  DevBuf dc, dp;
  if (!dc.alloc((size_t)nb * 128) || !dp.alloc((size_t)w * h * sizeof(float))) return GZ_E_NOMEM;
  if (hipMemcpy(dp.p, pixels, (size_t)w * h * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    return GZ_E_HIP;
  const float* dpix = (const float*)dp.p;
  int16_t* dcoef = (int16_t*)dc.p;
  GZ_LAUNCH(k_set_downsampled_coeffs, dim3(gz_div_up(nb, kBlocksPerWG)), dim3(256), (hipStream_t)0,
            dpix, w, h, fx, fy, bw, nb, dcoef);
  if (hipGetLastError() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(coeffs_out, dc.p, (size_t)nb * 128, hipMemcpyDeviceToHost) != hipSuccess)
    return GZ_E_HIP;
  return GZ_OK;
}


int gz_set_frame(gz_ctx* c, int chroma_factor) {
  DeviceScope ds_(c);
  if (!c || (chroma_factor != 1 && chroma_factor != 2)) return GZ_E_ARG;
  if (c->cfac == chroma_factor) return GZ_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  set_frame(c, chroma_factor);
  c->have_orig = false;   // the original coefficients on the device belonged to the other frame
  return GZ_OK;
}


// OutputImage::Downsample (output_image.cc:304-340), cfg defaults of Processor::DownsampleImage
// (processor.cc:97-104) without the silver-screen option, on the ORIGINAL coefficients of a
// 4:4:4 frame: ToFloatPixels of the three components, PreProcessChannel on V then on U
// (preprocess_downsample.cc:157-279), SetDownsampledCoefficients of U and V by 2 x 2.
static void normal_taps(double sigma, float k[5], float* mul) {   // Normal(), :85-88; Sharpen / Blur :92-100,138-146
  double kernel[5], sum = 0;
  for (size_t i = 0; i < 5; ++i) {
    const double x = 1.0 * i - 5 / 2;
    static const double kInvSqrt2Pi = 0.3989422804014327;
    kernel[i] = exp(-x * x / (2 * sigma * sigma)) * kInvSqrt2Pi / sigma;
  }
  for (size_t i = 0; i < 5; ++i) sum += kernel[i];
  for (size_t i = 0; i < 5; ++i) k[i] = static_cast<float>(kernel[i]);
  *mul = static_cast<float>(1.0 / sum);
}

int gz_downsample(gz_ctx* c, int16_t* coeffs_out) {
  DeviceScope ds_(c);
  if (!c) return GZ_E_ARG;
  TRY(byte_original(c, "gz_downsample"));
  if (!c->have_orig || c->cfac != 1) { c->err = "gz_downsample needs the original coefficients of a 4:4:4 frame"; return GZ_E_STATE; }
  c->have_orig = false;     // (d_orig's chroma is rewritten)
  c->xyb_is_cand = false;   // scratch: planes of the candidate's evaluation (nothing of it is in flight here)
  const int w = c->w, h = c->h;
  const size_t n = (size_t)w * h;
  float* yuv[3] = {c->xyb[0], c->xyb[1], c->xyb[2]};
  float* tmp_s = c->tmp[0];
  float* tmp_b = c->tmp[1];
  // byte planes: four per float plane
  uint8_t* bp0 = reinterpret_cast<uint8_t*>(c->tmp[2]);
  uint8_t* bp1 = reinterpret_cast<uint8_t*>(c->lf_raw[0]);
  uint8_t* dark_a = bp0; uint8_t* dark_b = bp0 + n; uint8_t* red_a = bp0 + 2 * n; uint8_t* red_b = bp0 + 3 * n;
  uint8_t* sharpen = bp1; uint8_t* blurm = bp1 + n; uint8_t* blur_t = bp1 + 2 * n;
  for (int i = 0; i < 3; ++i) {
    GZ_LAUNCH(k_to_float_pixels, dim3(gz_div_up(c->nb, kBlocksPerWG)), dim3(256), c->stream,
              (const int16_t*)(c->d_orig + (size_t)c->coff[i] * 64), w, h, c->bw, c->nb, yuv[i]);
    KCHK(c);
  }
  PPTaps taps;
  normal_taps((double)1.3f, taps.ks, &taps.mul_s);   // Sharpen(sigma = 1.3f)
  normal_taps(1.3, taps.kb, &taps.mul_b);            // Blur: kSigma = 1.3
  const dim3 g1(gz_div_up((int)std::min<size_t>(n, 0x7fffffff), 256)), g2(gz_div_up(w, 256), h);
  const int channels[2] = {2, 1};   // :326-329
  for (int pass = 0; pass < 2; ++pass) {
    const int channel = channels[pass];
    GZ_LAUNCH(k_pp_normalize, g1, dim3(256), c->stream, yuv[0], yuv[1], yuv[2], n);
    KCHK(c);
    GZ_LAUNCH(k_pp_maps, g1, dim3(256), c->stream, (const float*)yuv[0], (const float*)yuv[1],
              (const float*)yuv[2], n, channel, dark_a, red_a);
    KCHK(c);
    // Erode x3 (darkmap, :194-196): a -> b -> a -> b; Dilate x3 (redmap, :217-219) likewise
    for (int i = 0; i < 3; ++i) {
      GZ_LAUNCH(k_pp_morph, g2, dim3(256), c->stream, (const uint8_t*)(i & 1 ? dark_b : dark_a),
                i & 1 ? dark_a : dark_b, w, h, 1);
      KCHK(c);
      GZ_LAUNCH(k_pp_morph, g2, dim3(256), c->stream, (const uint8_t*)(i & 1 ? red_b : red_a),
                i & 1 ? red_a : red_b, w, h, 0);
      KCHK(c);
    }
    const double threshold = (channel == 2 ? 0.02 : 1.0) * 127.5;
    GZ_LAUNCH(k_pp_edge_maps, g2, dim3(256), c->stream, (const float*)yuv[channel], (const float*)yuv[1],
              (const float*)yuv[2], (const uint8_t*)dark_b, (const uint8_t*)red_b, w, h,
              threshold, sharpen, blurm);
    KCHK(c);
    // Erode x2 (blurmap, :254-255)
    GZ_LAUNCH(k_pp_morph, g2, dim3(256), c->stream, (const uint8_t*)blurm, blur_t, w, h, 1);
    KCHK(c);
    GZ_LAUNCH(k_pp_morph, g2, dim3(256), c->stream, (const uint8_t*)blur_t, blurm, w, h, 1);
    KCHK(c);
    GZ_LAUNCH(k_pp_conv_h, g2, dim3(256), c->stream, (const float*)yuv[channel], w, h, taps, tmp_s, tmp_b);
    KCHK(c);
    GZ_LAUNCH(k_pp_conv_v_select, g2, dim3(256), c->stream, yuv[channel], (const float*)tmp_s,
              (const float*)tmp_b, (const uint8_t*)sharpen, (const uint8_t*)blurm, w, h, taps, 0.5f, 1, 1);
    KCHK(c);
    GZ_LAUNCH(k_pp_denormalize, g1, dim3(256), c->stream, yuv[0], yuv[1], yuv[2], n);
    KCHK(c);
  }
  // the two chroma components, 2 x 2 subsampled, replace the 4:4:4 ones (luma is kept as it is)
  const int cbw = (w + 15) / 16, cbh = (h + 15) / 16, nbc = cbw * cbh;
  for (int i = 1; i < 3; ++i) {
    int16_t* dst = c->d_orig + ((size_t)c->nb + (size_t)(i - 1) * nbc) * 64;
    GZ_LAUNCH(k_set_downsampled_coeffs, dim3(gz_div_up(nbc, kBlocksPerWG)), dim3(256), c->stream,
              (const float*)yuv[i], w, h, 2, 2, cbw, nbc, dst);
    KCHK(c);
  }
  set_frame(c, 2);
  if (coeffs_out)
    HIPCHK(c, hipMemcpyAsync(coeffs_out, c->d_orig, (size_t)c->nblk * 128, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_orig = true;
  return GZ_OK;
}

int gz_downsample_planes(gz_ctx* c, const float* y, const float* u, const float* v, int16_t* coeffs_out) {
  DeviceScope ds_(c);
  if (!c || !y || !u || !v) return GZ_E_ARG;
  TRY(byte_original(c, "gz_downsample_planes"));
  if (!c->have_orig || c->cfac != 1) { c->err = "gz_downsample_planes needs the original coefficients of a 4:4:4 frame"; return GZ_E_STATE; }
  c->have_orig = false;
  c->xyb_is_cand = false;   // (xyb[] as scratch)
  const int w = c->w, h = c->h;
  const size_t n = (size_t)w * h;
  const float* src[3] = {y, u, v};
  for (int i = 0; i < 3; ++i)
    HIPCHK(c, hipMemcpyAsync(c->xyb[i], src[i], n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  // output_image.cc:314-316: every component from its plane, luma included (factor 1), the
  // chroma blocks packed behind the nb luma blocks
  const int cbw = (w + 15) / 16, cbh = (h + 15) / 16, nbc = cbw * cbh;
  GZ_LAUNCH(k_set_downsampled_coeffs, dim3(gz_div_up(c->nb, kBlocksPerWG)), dim3(256), c->stream,
            (const float*)c->xyb[0], w, h, 1, 1, c->bw, c->nb, c->d_orig);
  KCHK(c);
  for (int i = 1; i < 3; ++i) {
    int16_t* dst = c->d_orig + ((size_t)c->nb + (size_t)(i - 1) * nbc) * 64;
    GZ_LAUNCH(k_set_downsampled_coeffs, dim3(gz_div_up(nbc, kBlocksPerWG)), dim3(256), c->stream,
              (const float*)c->xyb[i], w, h, 2, 2, cbw, nbc, dst);
    KCHK(c);
  }
  set_frame(c, 2);
  if (coeffs_out)
    HIPCHK(c, hipMemcpyAsync(coeffs_out, c->d_orig, (size_t)c->nblk * 128, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_orig = true;
  return GZ_OK;
}


// ------------------------------------------------ use_silver_screen on the device ----
// RGBToYUV420 (preprocess_downsample.cc:452-476) by the kernels of gz_kernels_silver.h: the init pass and twenty
// rounds, one launch each.  A cell whose device power could not be proven to round like libm's pow wrote nothing
// and is on the device's list; behind every launch the listed cells are gathered into the pinned staging, a chunk
// at a time, redone here with libm (gz_silver_ref.h: the same CellEval the kernels run) and scattered back before
// the next launch is enqueued.  One wait per launch reads the list's length and its first chunk together.
namespace {
// GammaToLinear of a byte, by the host's libm: exact by construction
const float* silver_lut() {
  static const std::vector<float> lut = [] {
    std::vector<float> v(256);
    for (int i = 0; i < 256; ++i) v[i] = gz_silver::GammaToLinear(static_cast<float>(i));
    return v;
  }();
  return lut.data();
}
// One gathered cell (kSilverIn floats, k_silver_gather's layout) -> kSilverOut floats for k_silver_patch.
void silver_host_cell(bool init, const float* in, float* out) {
  float rec[4][3], yrec[4], yuv[3];
  memcpy(rec, in, sizeof(rec));
  gz_silver::LibmPow pw;
  gz_silver::CellEval(rec, (int)in[24], (int)in[25], pw, yrec, yuv);
  if (init) {
    for (int s = 0; s < 4; ++s) out[s] = yrec[s];
    out[4] = yuv[0]; out[5] = yuv[1]; out[6] = yuv[2]; out[7] = 0.0f;
  } else {
    for (int s = 0; s < 4; ++s) out[s] = gz_silver::Update(in[12 + s], yrec[s], in[16 + s]);
    out[4] = gz_silver::Update(in[20], yuv[1], in[22]);
    out[5] = gz_silver::Update(in[21], yuv[2], in[23]);
    out[6] = out[7] = 0.0f;
  }
}
constexpr size_t kSilverStageBytes = sizeof(float) * (kSilverHeader + (size_t)kSilverChunk * (kSilverIn + kSilverOut));
struct SilverRun {
  hipStream_t stream;
  SilverArgs a;
  float* stage;            // pinned and mapped, kSilverStageBytes
  float *out_u, *out_v;    // the chroma guesses box-upsampled to w x h (the luma plane is a.guess_y)
};
// counters (may be null): cell-passes evaluated (the init pass and the rounds), cell-passes redone on the host
int silver_run(const SilverRun& r, uint64_t* counters, std::string* err) {
#define SILVER_HIP(call)                                                             \
  do {                                                                               \
    const hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                          \
      *err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
      return e_ == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP;                      \
    }                                                                                \
  } while (0)
#define SILVER_KCHK()                                                                \
  do {                                                                               \
    const hipError_t e_ = hipGetLastError();                                         \
    if (e_ != hipSuccess) {                                                          \
      *err = std::string("kernel launch: ") + hipGetErrorString(e_);                 \
      return GZ_E_HIP;                                                               \
    }                                                                                \
  } while (0)
  const SilverArgs& a = r.a;
  const unsigned cells = (unsigned)a.w2 * (unsigned)a.h2;
  const dim3 grid(gz_div_up((int)cells, 256)), gather_grid(kSilverChunk / 256);
  float* in = r.stage + kSilverHeader;
  float* out = in + (size_t)kSilverChunk * kSilverIn;
  uint64_t redone = 0;
  for (int round = -1; round < kSilverRounds; ++round) {
    const int from = round < 0 ? -1 : (round & 1);
    SILVER_HIP(hipMemsetAsync(a.list, 0, sizeof(unsigned), r.stream));
    if (round < 0) {
      GZ_LAUNCH(k_silver_init, grid, dim3(256), r.stream, a);
    } else {
      GZ_LAUNCH(k_silver_iter, grid, dim3(256), r.stream, a, from);
    }
    SILVER_KCHK();
    unsigned n = 0;
    for (unsigned first = 0; first == 0 || first < n; first += kSilverChunk) {
      GZ_LAUNCH(k_silver_gather, gather_grid, dim3(256), r.stream, a, from, first, r.stage);
      SILVER_KCHK();
      SILVER_HIP(hipStreamSynchronize(r.stream));   // (also: the patch of the chunk before has read `out`)
      n = reinterpret_cast<const unsigned*>(r.stage)[0];
      if (n > cells) { *err = "silver screen: more listed cells than cells"; return GZ_E_HIP; }
      if (n == 0) break;
      const unsigned m = std::min<unsigned>(kSilverChunk, n - first);
      for (unsigned t = 0; t < m; ++t) silver_host_cell(round < 0, in + (size_t)t * kSilverIn, out + (size_t)t * kSilverOut);
      GZ_LAUNCH(k_silver_patch, dim3(gz_div_up((int)m, 256)), dim3(256), r.stream, a, from, first, m, (const float*)out);
      SILVER_KCHK();
    }
    redone += n;
  }
  const int last = kSilverRounds & 1;   // the half the last round wrote
  GZ_LAUNCH(k_silver_upsample, dim3(gz_div_up(a.w, 256), a.h), dim3(256), r.stream, (const float*)a.guess_u[last],
            (const float*)a.guess_v[last], a.w, a.h, a.w2, r.out_u, r.out_v);
  SILVER_KCHK();
  if (counters) {
    counters[0] = (uint64_t)cells * (kSilverRounds + 1);
    counters[1] = redone;
  }
  return GZ_OK;
#undef SILVER_HIP
#undef SILVER_KCHK
}
}  // namespace

int gz_downsample_silver(gz_ctx* c, int16_t* coeffs_out, uint64_t counters[2]) {
  DeviceScope ds_(c);
  if (!c) return GZ_E_ARG;
  TRY(byte_original(c, "gz_downsample_silver"));
  if (!c->have_orig || c->cfac != 1) { c->err = "gz_downsample_silver needs the original coefficients of a 4:4:4 frame"; return GZ_E_STATE; }
  const int w = c->w, h = c->h, w2 = (w + 1) / 2, h2 = (h + 1) / 2;
  const size_t cells = (size_t)w2 * h2;
  if (!c->made.silver) {
    TRY(regrow(c, c->stream, nullptr, 0, {{(void**)&c->d_silver_list, sizeof(unsigned) * (cells + 1)},
                                          {(void**)&c->d_silver_lut, sizeof(float) * 256},
                                          {(void**)&c->h_silver, kSilverStageBytes, true}}));
    HIPCHK(c, hipMemcpyAsync(c->d_silver_lut, silver_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, c->stream));
    c->made.silver = true;
  }
  c->have_orig = false;     // (d_orig is rewritten)
  c->xyb_is_cand = false;   // (xyb[] takes the three planes; tmp[] and lf_raw[0] are scratch no claim covers)
  // OutputImage::ToSRGB() of the unquantised image (output_image.cc:310): quantising by all ones is the identity, so the
  // pixels come from d_orig as they are -- the candidate and its planes are not touched
  TRY(stage_reconstruct(c, c->stream, c->d_orig, nullptr, c->d_srgb_out));
  SilverRun r;
  r.stream = c->stream;
  r.a.w = w; r.a.h = h; r.a.w2 = w2; r.a.h2 = h2;
  r.a.rgb = c->d_srgb_out;
  r.a.lut = c->d_silver_lut;
  r.a.guess_y = c->xyb[0];
  r.out_u = c->xyb[1];
  r.out_v = c->xyb[2];
  r.a.y_target = c->tmp[0];
  // (2 * cells <= w * h for every w, h >= 3: two quarter planes per scratch plane)
  r.a.target_u = c->tmp[1]; r.a.target_v = c->tmp[1] + cells;
  r.a.guess_u[0] = c->tmp[2]; r.a.guess_v[0] = c->tmp[2] + cells;
  r.a.guess_u[1] = c->lf_raw[0]; r.a.guess_v[1] = c->lf_raw[0] + cells;
  r.a.list = c->d_silver_list;
  r.a.guard = kPowGuard;
  r.a.list_all = 0;
  r.stage = c->h_silver;
  uint64_t cnt[2] = {0, 0};
  if (const int rc = silver_run(r, cnt, &c->err)) return rc;
  // output_image.cc:314-316: every component from its plane, as gz_downsample_planes
  const int cbw = (w + 15) / 16, cbh = (h + 15) / 16, nbc = cbw * cbh;
  GZ_LAUNCH(k_set_downsampled_coeffs, dim3(gz_div_up(c->nb, kBlocksPerWG)), dim3(256), c->stream,
            (const float*)c->xyb[0], w, h, 1, 1, c->bw, c->nb, c->d_orig);
  KCHK(c);
  for (int i = 1; i < 3; ++i) {
    int16_t* dst = c->d_orig + ((size_t)c->nb + (size_t)(i - 1) * nbc) * 64;
    GZ_LAUNCH(k_set_downsampled_coeffs, dim3(gz_div_up(nbc, kBlocksPerWG)), dim3(256), c->stream,
              (const float*)c->xyb[i], w, h, 2, 2, cbw, nbc, dst);
    KCHK(c);
  }
  set_frame(c, 2);
  if (coeffs_out)
    HIPCHK(c, hipMemcpyAsync(coeffs_out, c->d_orig, (size_t)c->nblk * 128, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (counters) { counters[0] = cnt[0]; counters[1] = cnt[1]; }
  c->have_orig = true;
  return GZ_OK;
}


}  // extern "C"
