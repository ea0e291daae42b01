#include <math.h>
#include <stdarg.h>
#include <string.h>

#include <atomic>

#include "encoder.h"
#include "jpeg_reader.h"
#include "parallel.h"

// A weak reference: the driver is also linked against stand-ins for the device library that implement the C ABI as
// it was when they were written (the recorded-session replay of the tests).  Such a library still loads; asking it
// for use_silver_screen fails below, loudly -- there is no host path behind this call.
extern "C" int gz_downsample_silver(gz_ctx* ctx, int16_t* coeffs_out, uint64_t counters[2]) __attribute__((weak));
// ... and so do the device-input entries: a stand-in without them refuses a DeviceImage, it has nowhere to read one from.
extern "C" gz_ctx* gz_create_from_device_pixels(int device, int w, int h, const gz_device_pixels* img, float target, int* err) __attribute__((weak));
extern "C" int gz_pack_rgb_device_pixels(int device, const gz_device_pixels* img, int w, int h, uint8_t* host_rgb_out) __attribute__((weak));

// ... and the device-output entries: a stand-in without them refuses DecodeJpegToRGB.
extern "C" int gz_decode_coeffs_device(int device, const int16_t* coeffs, int w, int h, int chroma_factor, const gz_device_output* out) __attribute__((weak));
extern "C" int gz_decode_coeffs(int device, const int16_t* coeffs, int w, int h, int chroma_factor, uint8_t* host_rgb_out) __attribute__((weak));
// ... and the device's scan decoder: without it every scan is read by the host.
extern "C" int gz_decode_scan(int device, const gz_scan* scan, int16_t* host_coeffs, gz_scan_result* result) __attribute__((weak));
extern "C" int gz_decode_scan_device(int device, const gz_scan* scan, const gz_device_output* out, gz_scan_result* result) __attribute__((weak));
extern "C" int gz_decode_scan_input(int device, const gz_scan* scan, int16_t* host_coeffs, int* large_coeff, gz_scan_result* result) __attribute__((weak));
extern "C" int gz_decode_scan_batch_device(int device, int n, const gz_scan* scans, const int* slots, const gz_device_output_batch* out,
                                           gz_scan_result* results, size_t scratch_cap_bytes) __attribute__((weak));

namespace guetzli_amd {

// ------------------------------------------------------------- quality / score tables --
namespace {
const int kLowestQuality = 70;
const int kHighestQuality = 110;
// Median butteraugli scores of libjpeg-turbo output per quality level 70..111
// (kScoreForQuality, quality.cc:31-74) -- data.
const double kQualityScore[] = {
  2.810761, 2.729300, 2.689687, 2.636811, 2.547863, 2.525400, 2.473416, 2.366133, 2.338078,
  2.318654, 2.201674, 2.145517, 2.087322, 2.009328, 1.945456, 1.900112, 1.805701, 1.750194,
  1.644175, 1.562165, 1.473608, 1.382021, 1.294298, 1.185402, 1.066781, 0.971769, 0.852901,
  0.724544, 0.611302, 0.443185, 0.211578, 0.209462, 0.207346, 0.205230, 0.203114, 0.200999,
  0.198883, 0.196767, 0.194651, 0.192535, 0.190420, 0.190420,
};
}  // namespace

double ButteraugliScoreForQuality(double quality) {
  if (quality < kLowestQuality) quality = kLowestQuality;
  if (quality > kHighestQuality) quality = kHighestQuality;
  const int index = static_cast<int>(quality);
  const double mix = quality - index;
  return kQualityScore[index - kLowestQuality] * (1 - mix) +
         kQualityScore[index - kLowestQuality + 1] * mix;
}

double ScoreJPEG(double butteraugli_distance, int size, double butteraugli_target) {
  const double kScale = 50, kMaxExponent = 10, kLargeSize = 1e30;
  const double diff = butteraugli_distance - butteraugli_target;
  if (diff <= 0.0) return size;
  const double exponent = kScale * diff;
  if (exponent > kMaxExponent) return kLargeSize * std::exp(kMaxExponent) * diff + size;
  return std::exp(exponent) * size;
}

// ------------------------------------------------------------------- the encoder ------
static HostScratch& ThreadScratch() {   // (HostScratch: encoder.h)
  static thread_local HostScratch s;
  return s;
}

static std::atomic<int> g_live_encoders{0};

Encoder::Encoder(const Params& p, ProcessStats* s) : params_(p), stats_(s), knobs_(HostKnobs::FromEnvironment()) {
  ++g_live_encoders;
  std::swap(sc_, ThreadScratch());
}

Encoder::~Encoder() {
  refreshers_.reset();
  --g_live_encoders;
  if (ctx_) gz_destroy(ctx_);
  std::swap(sc_, ThreadScratch());
}

// Helper threads for the size model's code refreshes (code_refresh.h) of ONE encode: GZ_CODE_THREADS,
// else by the cores the process may run on per encode in flight (batch mode: one Encoder per image in
// flight): 3 from eight cores on (4K: 0.271 s with none, 0.267 with 1, 0.258 with 2, 0.254 with 3;
// profiles/r05_chain_experiments.log, section 12), else one per core beyond the encode's own, at most 2.
// (evaluated at every search: in batch mode the first encoder of a batch is alone for a moment)
int Encoder::CodeRefreshThreads() const {
  if (knobs_.code_threads >= 0) return knobs_.code_threads;
  const int per_encode = WorkerPool::AllowedCpus() / std::max(1, g_live_encoders.load());
  if (per_encode >= 8) return 3;
  return std::max(0, std::min(2, per_encode - 1));
}

void Encoder::Log(const char* fmt, ...) {   // GUETZLI_LOG / PrintDebug, debug_print.h
  if (!stats_->debug_output && !stats_->debug_output_file) return;
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (stats_->debug_output) stats_->debug_output->append(buf);
  if (stats_->debug_output_file) fputs(buf, stats_->debug_output_file);
}

void Encoder::LogMatrix(const QuantMatrix q) {   // GUETZLI_LOG_QUANT
  for (int y = 0; y < 8; ++y) {
    for (int c = 0; c < 3; ++c) {
      for (int x = 0; x < 8; ++x) Log(" %2d", q[c][8 * y + x]);
      Log("   ");
    }
    Log("\n");
  }
}

bool Encoder::Fail(const char* what, int rc) {
  fprintf(stderr, "guetzli_amd: %s failed: %s (%s)\n", what, gz_strerror(rc),
          ctx_ ? gz_last_error(ctx_) : "");
  return false;
}

bool Encoder::TargetRefused() const {   // ProcessJpegData, processor.cc:800-806
  if (params_.butteraugli_target <= 2.0f) return false;
  fprintf(stderr,
          "Guetzli should be called with quality >= 84, otherwise the\n"
          "output will have noticeable artifacts. If you want to\n"
          "proceed anyway, please edit the source code.\n");
  return true;
}

void Encoder::SetGeometry(int w, int h, int factor) {
  w_ = w; h_ = h;
  bw_ = (w + 7) / 8; bh_ = (h + 7) / 8; nb_ = bw_ * bh_;
  SetFrame(factor);
}

void Encoder::SetFrame(int factor) {
  fac_ = factor;
  cbw_ = (w_ + 8 * factor - 1) / (8 * factor);
  cbh_ = (h_ + 8 * factor - 1) / (8 * factor);
  nbc_ = cbw_ * cbh_;
  coff_[0] = 0;
  coff_[1] = nb_;
  coff_[2] = nb_ + nbc_;
  nblk_ = nb_ + 2 * nbc_;
}

// "image too small for Butteraugli" (processor.cc:832-838, :940): the input is written as it is.
bool Encoder::WriteTooSmall(const Frame& f, std::string* out) {
  if (!WriteJpeg(f, out)) return Fail("WriteJpeg", GZ_E_STATE);
  Log("Original Out[%7zd]", out->size());
  Log(" <image too small for Butteraugli>\n");
  return true;
}

static void AllOnes(QuantMatrix q) {
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) q[c][k] = 1;
}

// start: the stopwatch of the whole call (what came before the search is "create+encode")
bool Encoder::Search(const QuantMatrix first_q, const Stopwatch& start, std::string* out) {
  stats_->timers["create+encode"] = start.read();
  Stopwatch sw;
  int rc = GZ_OK;
  // the original as the fallback output (processor.cc:826-846)
  best_score_ = -1;
  QuantMatrix ones;
  AllOnes(ones);
  if (!SetImageFromQuantization(ones, false)) return false;
  if (jpeg_input_ && fac_ == 2) {
    // OutputJpeg(jpg_in) of a 4:2:0 input: the file is written from the input's own blocks,
    // MCU padding included (the device frame leaves the padding out): on the host, once
    if (!WriteJpeg(in_frame_, &best_full_)) return Fail("WriteJpeg", GZ_E_STATE);
    const size_t size = best_full_.size();
    Log("Original Out[%7zd]", size);
    if (!CompareBegin() || !CompareCurrent()) return false;
    const double score = ScoreJPEG(distance_, (int)size, params_.butteraugli_target);
    Log(" Score[%.4f]", score);
    best_score_ = score;   // final_output_->score < 0: always taken (:142)
    best_size_ = size;
    best_on_host_ = true;
    Log(" (*)\n");
  } else {
    // symbols of the original: coefficient / its quantiser (1 for RGB input, the input's own
    // tables for a JPEG input, whose coefficients are held dequantised)
    SymbolHistogram dc[3], ac[3];
    size_t size = 0;
    if (!DeviceHistograms(jpeg_input_ ? q_in_ : ones, dc, ac) || !CompareBegin() ||
        !Serialize(nullptr, dc, ac, &size))
      return false;
    Log("Original Out[%7zd]", size);
    if (!CompareCurrent()) return false;
    if (!MaybeOutput(size)) return false;
  }

  // ProcessJpegData's loop over the sampling modes (:847-878)
  bool grey = true;   // IsGrayscale(jpg_in), :782-790
  for (size_t i = (size_t)coff_[1] * 64; i < (size_t)nblk_ * 64 && grey; ++i) grey = sc_.orig[i] == 0;
  const bool input_is_420 = fac_ == 2;
  const int try_420 = (input_is_420 || params_.force_420 || (params_.try_420 && !grey)) ? 1 : 0;
  const int force_420 = (input_is_420 || params_.force_420) ? 1 : 0;
  for (int downsample = force_420; downsample <= try_420; ++downsample) {
    // SaveToJpegData writes ONE component when both chroma components are all zero
    // (output_image.cc:357) -- whatever the frame: an RGB / 4:4:4 input whose chroma is zero
    // (Downsample does nothing, :305-308) and a 4:2:0 JPEG input with zero chroma alike.  The
    // round then runs with ymul = 1.0, without the chroma search and with one AC histogram.
    jpg_ncomp_ = (downsample && grey) ? 1 : 3;
    mirror_valid_ = false;   // sc_.img follows the device image from SetImageFromQuantization(best_q) on
    if (downsample && fac_ == 1) {   // DownsampleImage (:97-104) + SaveToJpegData
      if (!grey) {
        Stopwatch dw;
        if (params_.use_silver_screen) {
          // output_image.cc:309-318: ToSRGB() of the unquantised image -> RGBToYUV420 -> all three components
          // from the planes it returns, on the device (bit-identical to silver_screen.cc's host form: the cells
          // whose power the device cannot prove to round like libm's are redone by the library's host code)
          uint64_t cell_passes[2] = {0, 0};
          if (!gz_downsample_silver) return Fail("gz_downsample_silver (not in this device library)", GZ_E_STATE);
          rc = gz_downsample_silver(ctx_, sc_.orig.data(), cell_passes);
          if (rc != GZ_OK) return Fail("gz_downsample_silver", rc);
          stats_->counters["silver screen cell rounds"] = (int)std::min<uint64_t>(cell_passes[0], 0x7fffffff);
          stats_->counters["silver screen cell rounds on host"] = (int)std::min<uint64_t>(cell_passes[1], 0x7fffffff);
        } else {
          rc = gz_downsample(ctx_, sc_.orig.data());
          if (rc != GZ_OK) return Fail("gz_downsample", rc);
        }
        SetFrame(2);
        stats_->timers["downsample"] = dw.lap();
      }
    }
    QuantMatrix best_q;
    memcpy(best_q, first_q, sizeof(best_q));
    bool dist_ok = false;
    if (!SelectMatrix(best_q, downsample != 0, &dist_ok)) return false;
    if (!dist_ok) AllOnes(best_q);
    stats_->timers["select_quant_matrix"] += sw.lap();
    if (!SetImageFromQuantization(best_q, true)) return false;
    mirror_valid_ = true;
    if (!downsample) {
      if (!SelectFrequencyMasking(7, 1.0, false, true)) return false;
    } else {
      const float ymul = jpg_ncomp_ == 1 ? 1.0f : 0.97f;
      if (!SelectFrequencyMasking(1, ymul, false, false)) return false;
      if (!SelectFrequencyMasking(6, 1.0, true, true)) return false;
    }
    stats_->timers["select_frequency_masking"] += sw.lap();
  }
  // the timers and counters of encoder.h's table under their names
  static const char* const timer_name[kNumTimers] = {
#define GZ_STAT_NAME(id, name, ...) name,
      GZ_HOST_TIMERS(GZ_STAT_NAME)};
  static const struct { const char* name; long max; } counter[kNumCounters] = {
#define GZ_STAT_NAME_MAX(id, name, max) {name, max},
      GZ_HOST_COUNTERS(GZ_STAT_NAME_MAX)};
  for (int i = 0; i < kNumTimers; ++i)
    if (timer_name[i]) stats_->timers[timer_name[i]] = timer_[i];
  double fast_steps = 0;
  for (int i = kTFastCount; i <= kTFastRest; ++i) fast_steps += timer_[i];
  stats_->timers["pb_loop_fast_steps"] = fast_steps;
  for (int i = 0; i < kNumCounters; ++i)
    stats_->counters[counter[i].name] = (int)std::min(count_[i], counter[i].max);
  stats_->counters["phase B code refresh threads"] = refreshers_ ? refreshers_->threads() : 0;
  if (best_on_host_) {
    *out = best_full_;
  } else {  // the winner: its head from the host, its scan from the device
    std::vector<uint8_t>& scan = sc_.scan;
    if (scan.size() < (size_t)6 * w_ * h_ + 4096) scan.resize((size_t)6 * w_ * h_ + 4096);
    size_t n = 0;
    rc = gz_jpeg_scan_bytes(ctx_, 1, scan.data(), scan.size(), &n);
    if (rc != GZ_OK) return Fail("gz_jpeg_scan_bytes", rc);
    *out = best_head_;
    out->append((const char*)scan.data(), n);
    out->push_back((char)0xff);
    out->push_back((char)0xd9);
    if (jpeg_input_ && !meta_.strip) out->append(meta_.tail_data);
  }
  stats_->timers["total"] = start.read();
  return true;
}

// libjpeg's colour-space guess for three-component files (jpeg_data_decoder.cc:23-43): JFIF
// means YCbCr, an Adobe marker decides by its transform byte, else the ids 'R','G','B' mean RGB.
static bool HasYCbCrColorSpace(const JpegInput& jpg) {
  bool adobe = false;
  uint8_t transform = 0;
  for (const std::string& app : jpg.app_data) {
    if ((uint8_t)app[0] == 0xe0) return true;
    if ((uint8_t)app[0] == 0xee && app.size() >= 15) {
      adobe = true;
      transform = (uint8_t)app[14];
    }
  }
  if (adobe) return transform != 0;
  return jpg.components[0].id != 'R' || jpg.components[1].id != 'G' || jpg.components[2].id != 'B';
}

// A ScanRequest as the gz_scan the device's scan decoder takes.
static void ScanFromRequest(const ScanRequest& rq, const EntropyOptions& opt, gz_scan* sc) {
  memset(sc, 0, sizeof(*sc));
  sc->struct_size = (int)sizeof(*sc);
  sc->w = rq.width; sc->h = rq.height; sc->ncomp = rq.ncomp; sc->chroma_factor = rq.chroma_factor;
  sc->data = rq.data;
  sc->len = rq.len;
  for (int c = 0; c < rq.ncomp; ++c) {
    memcpy(sc->dc[c].counts, rq.dc[c].counts, 16);
    memcpy(sc->dc[c].values, rq.dc[c].values, 256);
    memcpy(sc->ac[c].counts, rq.ac[c].counts, 16);
    memcpy(sc->ac[c].values, rq.ac[c].values, 256);
    memcpy(sc->quant[c], rq.quant[c], sizeof(sc->quant[c]));
  }
  sc->subseq_bytes = opt.subseq_bytes;
  sc->max_sync_rounds = opt.max_sync_rounds;
}

namespace {
// What an encode of JPEG input with EntropyOptions::device gives the reader's hook: the scan as the READER leaves it
// (gz_decode_scan_input: quantised values on the grids padded to whole MCUs, and CheckJpegSanity's verdict over them),
// kept until ReadJpeg has returned and the components' `coeffs` can be filled from it.  It takes every scan the reader
// offers -- grey, 4:4:4, 4:2:0: no pixels are made here, so the colour space is not its business.
struct InputScan {
  int device = 0;
  EntropyOptions opt;
  DecodeInfo info;
  bool large_coeff = false;
  std::vector<int16_t>* coeffs = nullptr;   // the components one after the other
  bool operator()(const ScanRequest& rq, size_t* end_offset) {
    if (!gz_decode_scan_input) return false;
    static thread_local gz_scan sc;
    ScanFromRequest(rq, opt, &sc);
    const int f = rq.chroma_factor;
    const size_t mcus = (size_t)((rq.width + 8 * f - 1) / (8 * f)) * ((rq.height + 8 * f - 1) / (8 * f));
    coeffs->resize(mcus * (rq.ncomp == 1 ? 1 : f == 2 ? 6 : 3) * 64);
    gz_scan_result res;
    memset(&res, 0, sizeof(res));
    int large = 0;
    const int rc = gz_decode_scan_input(device, &sc, coeffs->data(), &large, &res);
    info.rc = rc;
    if (rc != GZ_OK) {   // the host reads the scan: the call's failure costs the attempt, not the encode -- and is on record
      fprintf(stderr, "guetzli_amd: the device's scan decoder failed (%s): the host reads the scan\n", gz_strerror(rc));
      return false;
    }
    info.status = res.status;
    info.subsequences = res.subsequences;
    info.sync_rounds = res.sync_rounds;
    info.end_offset = res.end_offset;
    if (res.status != GZ_SCAN_DECODED) return false;
    large_coeff = large != 0;
    *end_offset = (size_t)res.end_offset;
    return true;
  }
};

// The coefficients between the device and the components, kept per thread: a read after the first of a size touches no
// fresh pages (50 MB at 4K).
std::vector<int16_t>& InputScratchCoeffs() {
  static thread_local std::vector<int16_t> v;
  return v;
}
}  // namespace

bool ReadJpegInput(const std::string& data, int device, const EntropyOptions& entropy, JpegInput* jpg, bool* large_coeff,
                   DecodeInfo* info) {
  if (info) *info = DecodeInfo();
  if (large_coeff) *large_coeff = false;
  if (!entropy.device) return ReadJpeg((const uint8_t*)data.data(), data.size(), jpg);
  InputScan scan;
  scan.device = device;
  scan.opt = entropy;
  scan.coeffs = &InputScratchCoeffs();
  const ScanDecoder hook = [&scan](const ScanRequest& rq, size_t* end) { return scan(rq, end); };
  const bool ok = ReadJpeg((const uint8_t*)data.data(), data.size(), jpg, nullptr, &hook);
  if (info) *info = scan.info;
  if (!ok) return false;
  if (!jpg->scan_decoded_elsewhere) return true;   // (the block loop ran: nothing was offered, or the device handed it back)
  // ... as the block loop would have left it: `coeffs` of every component filled, everything else the parser's
  const int16_t* src = scan.coeffs->data();
  size_t at = 0;
  for (JpegComponentIn& c : jpg->components) {
    const size_t n = (size_t)c.width_in_blocks * c.height_in_blocks * 64;
    if (at + n > scan.coeffs->size()) {
      fprintf(stderr, "guetzli_amd: the device's scan holds fewer blocks than the frame\n");
      return false;
    }
    c.coeffs.assign(src + at, src + at + n);
    at += n;
  }
  jpg->scan_decoded_elsewhere = false;
  if (info) info->device_path = true;
  if (large_coeff) *large_coeff = scan.large_coeff;
  return true;
}

// guetzli::Process(params, stats, jpeg_data, &out) (processor.cc:890-924) for YUV 4:4:4 input.
bool Encoder::RunJpeg(const std::string& data, std::string* out, const EntropyOptions& entropy, DecodeInfo* info) {
  const Stopwatch start;
  JpegInput jpg;
  bool large_coeff = false;
  DecodeInfo read_info;
  const bool read = ReadJpegInput(data, params_.device, entropy, &jpg, &large_coeff, &read_info);
  if (info) *info = read_info;
  if (!read) {
    fprintf(stderr, "Can't read jpg data from input file\n");
    return false;
  }
  if (!read_info.device_path) {   // (the device has looked at every coefficient it stored)
    for (const JpegComponentIn& comp : jpg.components) {   // CheckJpegSanity, :117-131
      const int* q = jpg.quant[comp.quant_idx].values;
      for (size_t i = 0; i < comp.coeffs.size() && !large_coeff; ++i)
        large_coeff = std::abs((int64_t)comp.coeffs[i] * q[i % 64]) > (1 << 12);
    }
  }
  if (large_coeff) {
    fprintf(stderr, "Unsupported input JPEG (unexpectedly large coefficient values).\n");
    return false;
  }
  const size_t ncomp = jpg.components.size();
  const bool ycbcr3 = ncomp == 3 && HasYCbCrColorSpace(jpg);
  if (!(ncomp == 1 || (ycbcr3 && (jpg.Is420() || jpg.Is444())))) {   // DecodeJpegToRGB is empty
    fprintf(stderr, "Unsupported input JPEG file (e.g. unsupported downsampling mode).\n"
                    "Please provide the input image as a PNG file.\n");
    return false;
  }
  if (TargetRefused()) return false;
  if (!ycbcr3) {
    fprintf(stderr, "Only YUV color space input jpeg is supported\n");
    return false;
  }
  if (!jpg.Is444() && !jpg.Is420()) {   // ProcessJpegData, :811-824
    fprintf(stderr, "Unsupported sampling factors:");
    for (const JpegComponentIn& comp : jpg.components) fprintf(stderr, " %dx%d", comp.h_samp, comp.v_samp);
    fprintf(stderr, "\n");
    return false;
  }
  const int w = jpg.width, h = jpg.height;
  SetGeometry(w, h, jpg.Is420() ? 2 : 1);
  jpeg_input_ = true;
  meta_.strip = params_.clear_metadata;
  meta_.app_data = jpg.app_data;
  meta_.com_data = jpg.com_data;
  meta_.tail_data = jpg.tail_data;
  in_quant_.clear();
  for (const JpegQuant& t : jpg.quant) {
    QuantTable q;
    memcpy(q.values, t.values, sizeof(q.values));
    q.precision = t.precision;
    q.index = t.index;
    in_quant_.push_back(q);
  }
  // RemoveOriginalQuantization (:84-97): coefficients are held dequantised; of a 4:2:0
  // input's blocks those inside the image (CopyFromJpegComponent, output_image.cc:211-230)
  sc_.orig.resize((size_t)3 * nb_ * 64);
  for (int c = 0; c < 3; ++c) {
    const JpegComponentIn& comp = jpg.components[c];
    in_comp_id_[c] = comp.id;
    in_quant_idx_[c] = comp.quant_idx;
    memcpy(q_in_[c], jpg.quant[comp.quant_idx].values, sizeof(q_in_[c]));
    const int rw = c == 0 ? bw_ : cbw_, rh = c == 0 ? bh_ : cbh_;
    if (comp.width_in_blocks < rw || comp.height_in_blocks < rh) return Fail("block grid", GZ_E_STATE);
    int16_t* dst = &sc_.orig[(size_t)coff_[c] * 64];
    for (int by = 0; by < rh; ++by)
      for (int bx = 0; bx < rw; ++bx, dst += 64) {
        const int16_t* src = &comp.coeffs[((size_t)by * comp.width_in_blocks + bx) * 64];
        for (int k = 0; k < 64; ++k) dst[k] = (int16_t)(src[k] * q_in_[c][k]);
      }
  }
  if (fac_ == 2) {   // the input as read, for OutputJpeg(jpg_in)
    Frame& f = in_frame_;
    f.width = w; f.height = h; f.bw = bw_; f.bh = bh_;
    f.ncomp = 3;
    f.mcu_cols = jpg.mcu_cols; f.mcu_rows = jpg.mcu_rows;
    for (int c = 0; c < 3; ++c) {
      const JpegComponentIn& comp = jpg.components[c];
      f.samp[c] = comp.h_samp;
      f.cw[c] = comp.width_in_blocks;
      f.ch[c] = comp.height_in_blocks;
      f.coeffs[c] = comp.coeffs;
    }
    InputTables(&f);
    f.meta = &meta_;
  }
  if (w < 32 || h < 32) {
    // no butteraugli (:832-838): the input re-written with optimised Huffman codes
    Frame f444;
    if (fac_ == 1) {
      FrameFromImage(sc_.orig.data(), q_in_, w, h, &f444);
      f444.ncomp = 3;
      InputTables(&f444);
      f444.meta = &meta_;
    }
    return WriteTooSmall(fac_ == 2 ? in_frame_ : f444, out);
  }
  // The comparator's original is DecodeJpegToRGB(jpg) (jpeg_data_decoder.cc:45-54): the
  // integer IDCT of the input, computed by the context itself.
  int err = 0;
  {
    std::vector<uint8_t> blank((size_t)3 * w * h, 0);
    ctx_ = gz_create(params_.device, w, h, blank.data(), params_.butteraugli_target, &err);
    if (!ctx_) return Fail("gz_create", err);
    int rc = fac_ == 2 ? gz_set_orig_coeffs_420(ctx_, sc_.orig.data()) : gz_set_orig_coeffs(ctx_, sc_.orig.data());
    if (rc == GZ_OK) rc = gz_quantize(ctx_, nullptr, nullptr);
    if (rc == GZ_OK) rc = gz_reconstruct(ctx_, blank.data(), nullptr);
    if (rc == GZ_OK) rc = gz_set_rgb(ctx_, blank.data());
    if (rc != GZ_OK) return Fail("decode of the input JPEG", rc);
  }
  sc_.img.resize(sc_.orig.size());
  return Search(q_in_, start, out);
}

// no butteraugli (processor.cc:832-838, :940): the reference emits
// the unquantised JPEG of EncodeRGBToJpeg; the forward transform runs on the device.
bool Encoder::RunTooSmall(const uint8_t* rgb, int w, int h, std::string* out) {
  sc_.orig.resize((size_t)3 * nb_ * 64);
  const int rc0 = gz_encode_rgb_only(params_.device, rgb, w, h, sc_.orig.data());
  if (rc0 != GZ_OK) return Fail("gz_encode_rgb_only", rc0);
  Frame f;
  FrameFromOriginal(sc_.orig.data(), w, h, &f);
  return WriteTooSmall(f, out);
}

bool Encoder::RunFromContext(const Stopwatch& start, std::string* out) {
  sc_.orig.resize((size_t)3 * nb_ * 64);
  sc_.img.resize(sc_.orig.size());
  int rc = gz_encode_rgb(ctx_, sc_.orig.data());
  if (rc != GZ_OK) return Fail("gz_encode_rgb", rc);
  QuantMatrix ones;
  AllOnes(ones);
  return Search(ones, start, out);
}

bool Encoder::Run(const std::vector<uint8_t>& rgb, int w, int h, std::string* out) {
  const Stopwatch start;
  if (TargetRefused()) return false;
  if (w < 0 || w >= 1 << 16 || h < 0 || h >= 1 << 16 || rgb.size() != (size_t)3 * w * h) {
    fprintf(stderr, "Could not create jpg data from rgb pixels\n");   // EncodeRGBToJpeg failed
    return false;
  }
  SetGeometry(w, h, 1);
  if (w < 32 || h < 32) {
    if (w < 1 || h < 1) {
      fprintf(stderr, "Could not create jpg data from rgb pixels\n");
      return false;
    }
    return RunTooSmall(rgb.data(), w, h, out);
  }
  int err = 0;
  ctx_ = gz_create(params_.device, w, h, rgb.data(), params_.butteraugli_target, &err);
  if (!ctx_) return Fail("gz_create", err);
  return RunFromContext(start, out);
}

bool Encoder::RunDevice(const DeviceImage& image, int w, int h, std::string* out) {
  const Stopwatch start;
  if (TargetRefused()) return false;
  if (w < 1 || w >= 1 << 16 || h < 1 || h >= 1 << 16 || image.data == nullptr) {
    fprintf(stderr, "Could not create jpg data from rgb pixels\n");
    return false;
  }
  if (!gz_create_from_device_pixels || !gz_pack_rgb_device_pixels) return Fail("device-resident input (not in this device library)", GZ_E_STATE);
  gz_device_pixels img;
  memset(&img, 0, sizeof(img));
  img.struct_size = (int)sizeof(img);
  img.dtype = image.dtype;
  img.data = image.data;
  img.stride_y = image.stride_y; img.stride_x = image.stride_x; img.stride_c = image.stride_c;
  img.producer_stream = image.producer_stream;
  img.alpha = image.alpha;
  memcpy(img.background, image.background, 3);
  SetGeometry(w, h, 1);
  if (w < 32 || h < 32) {   // too small for a context: the kernel's bytes come to the host, the rest is Run's
    std::vector<uint8_t> rgb((size_t)3 * w * h);
    const int rc0 = gz_pack_rgb_device_pixels(params_.device, &img, w, h, rgb.data());
    if (rc0 != GZ_OK) return Fail("gz_pack_rgb_device_pixels", rc0);
    return RunTooSmall(rgb.data(), w, h, out);
  }
  int err = 0;
  ctx_ = gz_create_from_device_pixels(params_.device, w, h, &img, params_.butteraugli_target, &err);
  if (!ctx_) return Fail("gz_create_from_device_pixels", err);
  return RunFromContext(start, out);
}

// ------------------------------------------------------------- DecodeJpegToRGB ------
namespace {
// The stream's dequantised coefficients in the frame layout of include/guetzli_amd.h, as RunJpeg lays out its original
// (RemoveOriginalQuantization; of a 4:2:0 input the blocks inside the image's grid, CopyFromJpegComponent).  A
// one-component file gets two zero chroma components, as CopyFromJpegData leaves them.
// What a decode with EntropyOptions::device gives the reader's hook: where the coefficients (or, with `out`, the pixels)
// of a scan the device decodes go.
struct DeviceScan {
  int device = 0;
  EntropyOptions opt;
  const gz_device_output* out = nullptr;   // pixels straight into the caller's image ...
  std::vector<int16_t>* coeffs = nullptr;  // ... or coefficients to the host
  int expect_w = 0, expect_h = 0;
  // A batch (DecodeJpegBatchToRGB) asks the device for many files at once, so the hook runs twice per file: collecting --
  // the request is kept as the gz_scan the device takes, and the parse stops -- and, after the device call, replaying: the
  // hook answers with that call's return code and result for this scan.
  gz_scan* collect = nullptr;
  bool collected = false;
  const gz_scan_result* replay = nullptr;
  int replay_rc = 0;
  DecodeInfo info;
  bool operator()(const ScanRequest& rq, size_t* end_offset) {
    if (collect || replay ? !gz_decode_scan_batch_device : out ? !gz_decode_scan_device : !gz_decode_scan) return false;
    if ((expect_w > 0 || expect_h > 0) && (rq.width != expect_w || rq.height != expect_h)) return false;   // (refused below)
    if (rq.ncomp == 3 && !HasYCbCrColorSpace(*rq.so_far)) return false;
    if (collect) {
      ScanFromRequest(rq, opt, collect);
      collected = true;
      *end_offset = kScanDecoderStop;
      return true;
    }
    static thread_local gz_scan sc;
    if (!replay) ScanFromRequest(rq, opt, &sc);
    gz_scan_result res;
    memset(&res, 0, sizeof(res));
    int rc;
    if (replay) {
      rc = replay_rc;
      res = *replay;
      if (rc != GZ_OK) {   // (the batch's call failed, and has said so once for all its scans)
        info.rc = rc;
        return false;
      }
    } else if (out) {
      rc = gz_decode_scan_device(device, &sc, out, &res);
    } else {
      const int f = rq.chroma_factor;
      const size_t nb = (size_t)((rq.width + 7) / 8) * ((rq.height + 7) / 8);
      const size_t nbc = (size_t)((rq.width + 8 * f - 1) / (8 * f)) * ((rq.height + 8 * f - 1) / (8 * f));
      coeffs->resize((nb + 2 * nbc) * 64);
      rc = gz_decode_scan(device, &sc, coeffs->data(), &res);
    }
    info.rc = rc;
    if (rc != GZ_OK) {   // the host reads the scan: the call's failure costs the attempt, not the decode -- and is on record
      fprintf(stderr, "guetzli_amd: the device's scan decoder failed (%s): the host reads the scan\n", gz_strerror(rc));
      return false;
    }
    info.status = res.status;
    info.subsequences = res.subsequences;
    info.sync_rounds = res.sync_rounds;
    info.end_offset = res.end_offset;
    if (res.status != GZ_SCAN_DECODED) return false;
    *end_offset = (size_t)res.end_offset;
    return true;
  }
};

// (the second half of DecodedCoeffs: what a JpegInput the reader has filled holds)
bool FrameCoeffs(const JpegInput& jpg, int* w_out, int* h_out, int* factor_out, std::vector<int16_t>* coeffs);

bool DecodedCoeffs(const std::string& data, int* w_out, int* h_out, int* factor_out, std::vector<int16_t>* coeffs,
                   DeviceScan* scan = nullptr, JpegInput* meta = nullptr) {
  JpegInput local;
  JpegInput& jpg = meta ? *meta : local;
  ScanDecoder hook;
  if (scan) hook = [scan](const ScanRequest& rq, size_t* end) { return (*scan)(rq, end); };
  if (!ReadJpeg((const uint8_t*)data.data(), data.size(), &jpg, nullptr, scan ? &hook : nullptr)) {
    fprintf(stderr, "Can't read jpg data from input file\n");
    return false;
  }
  if (scan) scan->info.device_path = jpg.scan_decoded_elsewhere;
  if (jpg.stopped_at_scan) return true;   // (a collecting hook: nothing was decoded, and nothing is asked for yet)
  return FrameCoeffs(jpg, w_out, h_out, factor_out, coeffs);
}

bool FrameCoeffs(const JpegInput& jpg, int* w_out, int* h_out, int* factor_out, std::vector<int16_t>* coeffs) {
  const size_t ncomp = jpg.components.size();
  if (!(ncomp == 1 || (ncomp == 3 && HasYCbCrColorSpace(jpg) && (jpg.Is420() || jpg.Is444())))) {   // DecodeJpegToRGB is empty
    fprintf(stderr, "Unsupported input JPEG file (e.g. unsupported downsampling mode).\n");
    return false;
  }
  const int w = jpg.width, h = jpg.height;
  const int factor = ncomp == 3 && jpg.Is420() ? 2 : 1;
  const int bw = (w + 7) / 8, bh = (h + 7) / 8, nb = bw * bh;
  const int cbw = (w + 8 * factor - 1) / (8 * factor), cbh = (h + 8 * factor - 1) / (8 * factor), nbc = cbw * cbh;
  if (jpg.scan_decoded_elsewhere) {   // the device has dequantised, cropped and range-checked them (or made pixels of them)
    *w_out = w; *h_out = h; *factor_out = factor;
    return true;
  }
  coeffs->resize(((size_t)nb + 2 * (size_t)nbc) * 64);
  if (ncomp == 1) std::fill(coeffs->begin() + (size_t)nb * 64, coeffs->end(), (int16_t)0);   // (every other block is written below)
  for (size_t c = 0; c < ncomp; ++c) {
    const JpegComponentIn& comp = jpg.components[c];
    const int* q = jpg.quant[comp.quant_idx].values;
    const int rw = c == 0 ? bw : cbw, rh = c == 0 ? bh : cbh;
    if (comp.width_in_blocks < rw || comp.height_in_blocks < rh) {
      fprintf(stderr, "guetzli_amd: the JPEG's block grid is smaller than its image\n");
      return false;
    }
    int16_t* dst = coeffs->data() + (c == 0 ? (size_t)0 : (size_t)nb + (c - 1) * (size_t)nbc) * 64;
    // (a quantiser is at most 65535 and a coefficient an int16: the product fits 32 bits; the check is kept out of the
    // loop's control flow so that the loop stays a vector loop -- 25 M coefficients at 4K)
    int32_t qv[64];
    for (int k = 0; k < 64; ++k) qv[k] = q[k];
    int32_t wide = 0;
    for (int by = 0; by < rh; ++by) {
      const int16_t* src = &comp.coeffs[(size_t)by * comp.width_in_blocks * 64];
      for (int bx = 0; bx < rw; ++bx, dst += 64, src += 64)
        for (int k = 0; k < 64; ++k) {
          const int32_t v = (int32_t)src[k] * qv[k];
          dst[k] = (int16_t)v;
          wide |= v ^ (int32_t)(int16_t)v;
        }
    }
    if (wide != 0) {   // a product that does not fit the frame's int16
      fprintf(stderr, "Unsupported input JPEG (unexpectedly large coefficient values).\n");
      return false;
    }
  }
  *w_out = w; *h_out = h; *factor_out = factor;
  return true;
}

// The coefficients between the reader and the upload, kept per thread as the encoder's scratch is: a decode after the
// first of a size touches no fresh pages (50 MB at 4K).
std::vector<int16_t>& DecodeScratchCoeffs() {
  static thread_local std::vector<int16_t> v;
  return v;
}

bool DecodeFailed(const char* what, int rc) {
  fprintf(stderr, "guetzli_amd: %s failed: %s\n", what, gz_strerror(rc));
  return false;
}
}  // namespace

bool JpegSize(const std::string& jpeg, int* w, int* h) {
  JpegInput jpg;
  if (!ReadJpeg((const uint8_t*)jpeg.data(), jpeg.size(), &jpg)) {
    fprintf(stderr, "Can't read jpg data from input file\n");
    return false;
  }
  if (w) *w = jpg.width;
  if (h) *h = jpg.height;
  return true;
}

bool DecodeJpegToRGB(const std::string& jpeg, int device, const DeviceOutput& out, int* w_out, int* h_out, int expect_w,
                     int expect_h) {
  return DecodeJpegToRGB(jpeg, device, out, w_out, h_out, expect_w, expect_h, EntropyOptions(), nullptr);
}

namespace {
gz_device_output OutputOf(const DeviceOutput& out) {
  gz_device_output o;
  memset(&o, 0, sizeof(o));
  o.struct_size = (int)sizeof(o);
  o.dtype = out.dtype;
  o.data = out.data;
  o.stride_y = out.stride_y; o.stride_x = out.stride_x; o.stride_c = out.stride_c;
  o.consumer_stream = out.consumer_stream;
  return o;
}

// One JPEG into `o` with the reader's hook in the state the caller has given it (nullptr: the host reads the scan).  A
// collecting hook that took the scan ends the call there: nothing is decoded yet.
bool DecodeToOutput(const std::string& jpeg, int device, const gz_device_output& o, int* w_out, int* h_out, int expect_w, int expect_h,
                    DeviceScan* scan) {
  int w = 0, h = 0, factor = 1;
  std::vector<int16_t>& coeffs = DecodeScratchCoeffs();
  const bool ok = DecodedCoeffs(jpeg, &w, &h, &factor, &coeffs, scan);
  if (!ok) return false;
  if (scan && scan->collected) return true;
  if (w_out) *w_out = w;
  if (h_out) *h_out = h;
  if (scan && scan->info.device_path) return true;   // (the pixels are in `o`; the size was checked in front of the device call)
  if ((expect_w > 0 || expect_h > 0) && (w != expect_w || h != expect_h)) {
    fprintf(stderr, "guetzli_amd: the JPEG holds %d x %d pixels, the destination was made for %d x %d\n", w, h, expect_w, expect_h);
    return false;
  }
  if (!gz_decode_coeffs_device) return DecodeFailed("device-resident output (not in this device library)", GZ_E_STATE);
  const int rc = gz_decode_coeffs_device(device, coeffs.data(), w, h, factor, &o);
  return rc == GZ_OK ? true : DecodeFailed("gz_decode_coeffs_device", rc);
}
}  // namespace

bool DecodeJpegToRGB(const std::string& jpeg, int device, const DeviceOutput& out, int* w_out, int* h_out, int expect_w,
                     int expect_h, const EntropyOptions& entropy, DecodeInfo* info) {
  const gz_device_output o = OutputOf(out);
  DeviceScan scan;
  scan.device = device;
  scan.opt = entropy;
  scan.out = &o;
  scan.expect_w = expect_w; scan.expect_h = expect_h;
  const bool ok = DecodeToOutput(jpeg, device, o, w_out, h_out, expect_w, expect_h, entropy.device ? &scan : nullptr);
  if (info) *info = scan.info;
  return ok;
}

bool DecodeJpegBatchToRGB(const std::vector<std::string>& jpegs, int device, const DeviceOutputBatch& out, int expect_w, int expect_h,
                          const EntropyOptions& entropy, std::vector<DecodeInfo>* infos, int* failed, size_t scratch_cap_bytes) {
  const int n = (int)jpegs.size();
  if (infos) infos->assign((size_t)n, DecodeInfo());
  if (failed) *failed = -1;
  auto fail = [failed](int i) {
    if (failed) *failed = i;
    fprintf(stderr, "guetzli_amd: image %d of the batch could not be decoded\n", i);
    return false;
  };
  if (n < 1) return true;
  if (expect_w <= 0 || expect_h <= 0) {   // the batch's size is the first file's
    if (!JpegSize(jpegs[0], &expect_w, &expect_h)) return fail(0);
  }
  const size_t elem = out.dtype == DeviceImage::kU8 ? 1 : out.dtype == DeviceImage::kF32 ? 4 : 2;
  auto image = [&](int i) {
    DeviceOutput one;
    one.dtype = out.dtype;
    one.data = (char*)out.data + (size_t)i * (size_t)out.stride_n * elem;
    one.stride_y = out.stride_y; one.stride_x = out.stride_x; one.stride_c = out.stride_c;
    one.consumer_stream = out.consumer_stream;
    return OutputOf(one);
  };
  std::vector<DeviceScan> hooks((size_t)n);
  std::vector<gz_scan> scans;
  std::vector<int> owner;   // scans[k] is image owner[k]'s
  std::vector<gz_scan_result> verdicts;
  std::vector<int> call_rc;
  if (entropy.device && gz_decode_scan_batch_device) {
    // the collecting pass: every file up to its scan; a file whose scan is not offered is read to its end and decoded here
    scans.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
      scans.emplace_back();
      DeviceScan& hook = hooks[(size_t)i];
      hook.device = device;
      hook.opt = entropy;
      hook.expect_w = expect_w; hook.expect_h = expect_h;
      hook.collect = &scans.back();
      const gz_device_output o = image(i);
      hook.out = &o;
      const bool ok = DecodeToOutput(jpegs[(size_t)i], device, o, nullptr, nullptr, expect_w, expect_h, &hook);
      hook.out = nullptr;
      hook.collect = nullptr;
      if (!ok) return fail(i);
      if (hook.collected) owner.push_back(i); else scans.pop_back();
    }
    // one device call per sampling: grey, 4:4:4, 4:2:0
    verdicts.resize(scans.size());
    call_rc.assign(scans.size(), GZ_OK);
    gz_device_output_batch ob;
    memset(&ob, 0, sizeof(ob));
    ob.struct_size = (int)sizeof(ob);
    ob.dtype = out.dtype;
    ob.data = out.data;
    ob.stride_n = out.stride_n; ob.stride_y = out.stride_y; ob.stride_x = out.stride_x; ob.stride_c = out.stride_c;
    ob.consumer_stream = out.consumer_stream;
    ob.n = n;
    for (int group = 0; group < 3; ++group) {
      const int ncomp = group == 0 ? 1 : 3, factor = group == 2 ? 2 : 1;
      std::vector<gz_scan> members;
      std::vector<int> slots, at;
      for (size_t k = 0; k < scans.size(); ++k)
        if (scans[k].ncomp == ncomp && scans[k].chroma_factor == factor) {
          members.push_back(scans[k]);
          slots.push_back(owner[k]);
          at.push_back((int)k);
        }
      if (members.empty()) continue;
      std::vector<gz_scan_result> res(members.size());
      const int rc = gz_decode_scan_batch_device(device, (int)members.size(), members.data(), slots.data(), &ob, res.data(), scratch_cap_bytes);
      if (rc != GZ_OK)
        fprintf(stderr, "guetzli_amd: the device's batched scan decoder failed (%s): the host reads the scans it left\n", gz_strerror(rc));
      for (size_t k = 0; k < members.size(); ++k) {
        verdicts[(size_t)at[k]] = res[k];
        call_rc[(size_t)at[k]] = res[k].subsequences != 0 ? GZ_OK : rc;   // (a chunk in front of the failure has its verdicts)
      }
    }
    // the resuming pass: the reader again, the hook answering with the verdict -- what lies behind the scan is judged as
    // ever, and a scan without the status DECODED is read by the host into its image
    for (size_t k = 0; k < scans.size(); ++k) {
      const int i = owner[k];
      DeviceScan& hook = hooks[(size_t)i];
      const gz_device_output o = image(i);
      hook.out = &o;
      hook.collected = false;
      hook.replay = &verdicts[k];
      hook.replay_rc = call_rc[k];
      const bool ok = DecodeToOutput(jpegs[(size_t)i], device, o, nullptr, nullptr, expect_w, expect_h, &hook);
      hook.out = nullptr;
      hook.replay = nullptr;
      if (!ok) return fail(i);
    }
    if (infos)
      for (int i = 0; i < n; ++i) (*infos)[(size_t)i] = hooks[(size_t)i].info;
    return true;
  }
  for (int i = 0; i < n; ++i) {
    const gz_device_output o = image(i);
    if (!DecodeToOutput(jpegs[(size_t)i], device, o, nullptr, nullptr, expect_w, expect_h, nullptr)) return fail(i);
  }
  return true;
}

bool DecodeJpegCoeffs(const std::string& jpeg, int device, const EntropyOptions& entropy, int* w, int* h, int* factor,
                      std::vector<int16_t>* coeffs, DecodeInfo* info, JpegInput* meta) {
  DeviceScan scan;
  scan.device = device;
  scan.opt = entropy;
  scan.coeffs = coeffs;
  const bool ok = DecodedCoeffs(jpeg, w, h, factor, coeffs, entropy.device ? &scan : nullptr, meta);
  if (info) *info = scan.info;
  return ok;
}

bool DecodeJpegToRGB(const std::string& jpeg, int device, std::vector<uint8_t>* rgb, int* w_out, int* h_out) {
  return DecodeJpegToRGB(jpeg, device, rgb, w_out, h_out, EntropyOptions(), nullptr);
}

bool DecodeJpegToRGB(const std::string& jpeg, int device, std::vector<uint8_t>* rgb, int* w_out, int* h_out,
                     const EntropyOptions& entropy, DecodeInfo* info) {
  int w = 0, h = 0, factor = 1;
  std::vector<int16_t>& coeffs = DecodeScratchCoeffs();
  if (!DecodeJpegCoeffs(jpeg, device, entropy, &w, &h, &factor, &coeffs, info)) return false;
  if (w_out) *w_out = w;
  if (h_out) *h_out = h;
  if (!gz_decode_coeffs) return DecodeFailed("gz_decode_coeffs (not in this device library)", GZ_E_STATE);
  rgb->resize((size_t)3 * w * h);
  const int rc = gz_decode_coeffs(device, coeffs.data(), w, h, factor, rgb->data());
  return rc == GZ_OK ? true : DecodeFailed("gz_decode_coeffs", rc);
}

bool Process(const Params& params, ProcessStats* stats, const std::vector<uint8_t>& rgb, int w,
             int h, std::string* out) {
  ProcessStats dummy;
  if (stats == nullptr) stats = &dummy;
  Encoder enc(params, stats);
  return enc.Run(rgb, w, h, out);
}

bool Process(const Params& params, ProcessStats* stats, const DeviceImage& image, int w, int h,
             std::string* out) {
  ProcessStats dummy;
  if (stats == nullptr) stats = &dummy;
  Encoder enc(params, stats);
  return enc.RunDevice(image, w, h, out);
}

bool Process(const Params& params, ProcessStats* stats, const std::string& jpeg_data,
             std::string* out) {
  return Process(params, stats, jpeg_data, out, EntropyOptions(), nullptr);
}

bool Process(const Params& params, ProcessStats* stats, const std::string& jpeg_data, std::string* out,
             const EntropyOptions& entropy, DecodeInfo* info) {
  ProcessStats dummy;
  if (stats == nullptr) stats = &dummy;
  Encoder enc(params, stats);
  return enc.RunJpeg(jpeg_data, out, entropy, info);
}

}  // namespace guetzli_amd
