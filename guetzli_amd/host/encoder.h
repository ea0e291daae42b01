// Internal to the host search driver: the Encoder behind guetzli_amd::Process and what its pieces share.
//   processor.cc   the driver: quality table, ScoreJPEG, Search, the two input paths, Process
//   candidate.cc   one candidate: symbol statistics, head + scan, comparison, output; the quant-matrix trials
//   phase_b.cc     SelectFrequencyMasking
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/guetzli_amd.h"
#include "code_refresh.h"
#include "jpeg_writer.h"
#include "lazy_sort.h"
#include "matrix_search.h"
#include "processor.h"

// (the driver's internals stay internal to the library, as they were in one translation unit: no exported
// symbols, and calls between the driver's files that bind directly)
#pragma GCC visibility push(hidden)
namespace guetzli_amd {

struct Stopwatch {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double read() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  double lap() {
    const auto t1 = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
    return s;
  }
};

// (these two are in the serial loop's critical path: inline, not calls into another translation unit)
inline int16_t QuantizeCoeff(int16_t raw, int quant) {   // quantize.h:24-29
  const int r = raw % quant;
  const int16_t delta = (int16_t)(2 * r > quant ? quant - r : (-2) * r > quant ? -quant - r : -r);
  return (int16_t)(raw + delta);
}

// "precious" coefficients are never zeroed (processor.cc:722-733): (0,1) and (1,0) of a
// block whose original value is at least 4 (8 when the block has much high-frequency energy).
inline bool IsPrecious(const int16_t* orig_blk, int k) {
  if (k != 1 && k != 8) return false;
  double sum_of_hf = 0;
  for (int ii = 3; ii < 64; ++ii) {
    if ((ii & 7) < 3 && ii < 3 * 8) continue;
    sum_of_hf += std::abs(orig_blk[ii]);
  }
  const int limit = sum_of_hf < 60 ? 4 : 8;
  return std::abs(orig_blk[k]) >= limit;
}

inline bool ChromaAllZero(const SymbolHistogram* dc, const SymbolHistogram* ac) {
  // all DC differences zero (so every DC is zero) and nothing but end-of-block in AC
  for (int c = 1; c < 3; ++c)
    for (int i = 1; i + 1 < kHistoSize; ++i)
      if (dc[c].counts[i] || ac[c].counts[i]) return false;
  return true;
}

// The large host arrays of one encode (60 MB at 1080p, 240 MB at 4K).  Fresh std::vectors of
// this size come from mmap and are paid for in page faults (~15 ms per 1080p encode, measured
// as the gap between the phase timers and the wall clock of a step): a thread keeps them
// between encodes instead, and an Encoder borrows them for its lifetime (every element that is
// read was written by this encode).
struct HostScratch {
  std::vector<int16_t> orig;     // unquantised coefficients (JPEGData of EncodeRGBToJpeg)
  std::vector<int16_t> img;      // coefficients of the working image (OutputImage::coeffs_)
  // phase A's CSR arrays, the fetched part of phase B's order, the winner's scan
  std::vector<uint8_t> cand_idx;
  std::vector<int32_t> cand_off;
  std::vector<std::pair<int, float> > order;
  std::vector<uint8_t> scan;
};

// The host driver's switches, read from the environment ONCE per encode (Encoder's constructor) -- never inside
// the search loops, which run on several encoder threads at once in batch mode.  All of them are test / A-B
// switches: the defaults are the product.
struct HostKnobs {
  int code_threads = -1;              // GZ_CODE_THREADS: helper threads of the code refreshes (-1: by the cores)
  size_t parallel_count_min = (size_t)1 << 20;   // GZ_PARALLEL_COUNT_MIN: step counts on the worker pool from this many entries on
  long code_serial_steps = 30;        // GZ_CODE_SERIAL_STEPS: serial steps before the helpers are called in (0: at once)
  bool check_mirror = false;          // GZ_CHECK_MIRROR: host mirror against the device image after every search
  // GZ_VERIFY_ENTROPY=1|2: every candidate also through the host writer (1: cross-check against the host
  // writer; 2: check the size bound's own, late-scan, path)
  int verify_level = 0;
  bool verify() const { return verify_level > 0; }
  // GZ_ORDER_DEVICE_THRESHOLD: ranges above this are partitioned on the device (32-64 K measured best at 1080p and 4K)
  size_t order_device_threshold = 1 << 16;
  static HostKnobs FromEnvironment() {
    HostKnobs k;
    if (const char* e = getenv("GZ_CODE_THREADS")) k.code_threads = std::max(0, std::min(4, atoi(e)));
    if (const char* e = getenv("GZ_PARALLEL_COUNT_MIN")) k.parallel_count_min = (size_t)atol(e);
    if (const char* e = getenv("GZ_CODE_SERIAL_STEPS")) k.code_serial_steps = atol(e) / 10 * 10;
    k.check_mirror = getenv("GZ_CHECK_MIRROR") != nullptr;
    if (const char* e = getenv("GZ_VERIFY_ENTROPY")) k.verify_level = std::max(1, atoi(e));
    if (const char* e = getenv("GZ_ORDER_DEVICE_THRESHOLD")) k.order_device_threshold = (size_t)std::max(16L, atol(e));
    return k;
  }
};

// phase B's order entries compare by key alone (processor.cc:675-678); lazy_sort.h's AVX2 pass knows the layout
struct OrderKeyLess {
  enum { float_second_key = 1 };
  bool operator()(const std::pair<int, float>& a, const std::pair<int, float>& b) const {
    return a.second < b.second;
  }
};
typedef LazySorted<std::pair<int, float>, OrderKeyLess> SortedOrder;

// The driver's timers (seconds) and counters of one encode: X(id, name in ProcessStats::timers / counters
// [, the value a counter saturates at]).  Encoder::timer_ / count_ are indexed by the ids -- a constant index,
// so that accumulating inside the search loops stays a plain add -- and Search publishes them by the names.
// kTFastRest is not published on its own: pb_loop_fast_steps is the sum of kTFastCount .. kTFastRest.
#define GZ_HOST_TIMERS(X)                                                                           \
  X(kTWrite, "jpeg_write") X(kTCompare, "compare") X(kTQuant, "quantize")                           \
  X(kTBlockSearch, "block_search") X(kTPhaseB, "phase_b_host") X(kTUpload, "block_upload")          \
  /* where the host's time goes at the end of an iteration */                                       \
  X(kTHead, "jpeg_head") X(kTCmpBegin, "compare_begin") X(kTCmpEnd, "compare_end")                  \
  X(kTScanBegin, "jpeg_scan_begin") X(kTScanEnd, "jpeg_scan_end") X(kTAheadBegin, "pb_order_ahead_begin") \
  X(kTOrder, "pb_order") X(kTSort, "pb_sort") X(kTLoop, "pb_loop") X(kTCodes, "pb_loop_codes")      \
  X(kTEnsure, "pb_loop_ensure_sorted")                                                              \
  X(kTFastCount, "pb_fast_count") X(kTFastApply, "pb_fast_apply") X(kTFastMirror, "pb_fast_mirror") \
  X(kTFastDelta, "pb_fast_delta") X(kTFastRest, nullptr)                                            \
  /* seconds inside the device calls (round trips included) */                                      \
  X(kTDevPartition, "pb_device_partitions") X(kTDevFetch, "pb_device_fetches") X(kTDescend, "pb_device_descents")
#define GZ_HOST_COUNTERS(X)                                                                         \
  X(kNExported, "phase B prefixes exported by the device", 2147483647L)                             \
  X(kNReplayed, "phase B partitions made ahead", 2147483647L)                                       \
  X(kNPartitions, "phase B device partitions", 2147483647L)                                         \
  X(kNFetched, "phase B entries fetched", 2147483647L)                                              \
  X(kNEvaluations, "block search evaluations", 2000000000L)                                         \
  X(kNFast, "phase B fast steps", 2147483647L)                                                      \
  /* candidates entropy-coded / known to lose without it */                                         \
  X(kNScans, "candidates entropy-coded", 2147483647L)                                               \
  X(kNScansSkipped, "candidates rejected on their size bound", 2147483647L)                         \
  X(kNSteps, "phase B coefficient steps", 2147483647L)                                              \
  X(kNUndone, "phase B steps taken ahead and undone", 2147483647L)                                  \
  X(kNOrder, "phase B order entries", 2000000000L)
#define GZ_STAT_ID(id, ...) id,
enum Timer { GZ_HOST_TIMERS(GZ_STAT_ID) kNumTimers };
enum Counter { GZ_HOST_COUNTERS(GZ_STAT_ID) kNumCounters };
#undef GZ_STAT_ID

// one serial step of phase B as it was taken, so that it can be priced later and undone
struct SlowStep {
  int32_t b, pos;
  float val;
  int16_t old_val;
  uint8_t changed, first_touch, comp, nsym;
  int16_t sym[kMaxCoeffACSymbolChanges];
};

class Encoder {
 public:
  Encoder(const Params& p, ProcessStats* s);
  ~Encoder();
  bool Run(const std::vector<uint8_t>& rgb, int w, int h, std::string* out);
  bool RunDevice(const DeviceImage& image, int w, int h, std::string* out);
  bool RunJpeg(const std::string& jpeg_data, std::string* out, const EntropyOptions& entropy = EntropyOptions(),
               DecodeInfo* info = nullptr);

 private:
  // ---- processor.cc ----
  void Log(const char* fmt, ...) __attribute__((format(printf, 2, 3)));
  void LogMatrix(const QuantMatrix q);
  bool Fail(const char* what, int rc);
  bool TargetRefused() const;
  void SetGeometry(int w, int h, int factor);
  void SetFrame(int factor);
  bool WriteTooSmall(const Frame& f, std::string* out);
  bool RunTooSmall(const uint8_t* rgb, int w, int h, std::string* out);   // w or h < 32, from host pixels
  bool RunFromContext(const Stopwatch& start, std::string* out);          // ctx_ holds the original's pixels
  int CodeRefreshThreads() const;
  bool Search(const QuantMatrix first_q, const Stopwatch& start, std::string* out);   // ProcessJpegData from :826 on
  const char* FrameStr() const { return fac_ == 2 ? "f112222" : "f111111"; }   // OutputImage::FrameTypeStr
  size_t Pos(int c, int block, int k) const { return ((size_t)coff_[c] + block) * 64 + k; }
  bool DistanceOK(double target_mul) const { return distance_ <= target_mul * params_.butteraugli_target; }
  // ---- candidate.cc ----
  // SaveToJpegData + WriteJpeg of the current image: marker segments and Huffman codes
  // on the host from the symbol statistics, the scan on the device.  *size = jpg.size().
  bool DeviceHistograms(const QuantMatrix q, SymbolHistogram* dc, SymbolHistogram* ac, int ncomp = 3);
  bool Serialize(const int (*q)[64], const SymbolHistogram* dc, const SymbolHistogram* ac,
                 size_t* size);
  bool SerializeEnd(const int (*q)[64], size_t* size);
  bool PrepareHead(const int (*q)[64], const SymbolHistogram* dc, const SymbolHistogram* ac);
  bool ScanBegin();
  size_t SizeLowerBound() const;
  bool CompareBegin();
  bool CompareCurrent();
  bool MaybeOutput(size_t size);
  bool VerifyAgainstHostWriter(const int (*q)[64], size_t size);
  bool TryMatrix(float target_mul, const QuantMatrix q, Trial* t);
  bool SelectMatrix(QuantMatrix best, bool downsample, bool* dist_ok);
  bool SetImageFromQuantization(const QuantMatrix q, bool download);
  // The tables of a frame of this image: quant matrices q, or null for the "original" (the
  // q = 1 frame of EncodeRGBToJpeg, or the input JPEG's own tables), plus the metadata a JPEG
  // input carries into every output.
  void Tables(const int (*q)[64], int ncomp, Frame* f) const;
  void InputTables(Frame* f) const;   // jpg_in as read: its own DQT tables in file order, its component ids
  // ---- phase_b.cc ----
  bool SelectFrequencyMasking(int comp_mask, double target_mul, bool stop_early, bool last_search_of_round);
  struct MaskSearch;   // the state and the pieces of one such search

  Params params_;
  ProcessStats* stats_;
  const HostKnobs knobs_;   // the environment's switches, read once
  gz_ctx* ctx_ = nullptr;
  int w_ = 0, h_ = 0, bw_ = 0, bh_ = 0, nb_ = 0;
  // the frame (OutputImage's component layout): chroma factor 1 (4:4:4) or 2 (4:2:0), blocks
  // per chroma component, first block of every component in sc_.orig / sc_.img, blocks in total
  int fac_ = 1, cbw_ = 0, cbh_ = 0, nbc_ = 0, coff_[3] = {0, 0, 0}, nblk_ = 0;
  int jpg_ncomp_ = 3;            // jpg.components.size() of the round (1: greyscale after Downsample)
  size_t best_size_ = 0;         // final_output_->jpeg_data.size()
  std::string best_full_;        // a best candidate written on the host (the 4:2:0 input as read)
  bool best_on_host_ = false;
  HostScratch sc_;               // the thread's arrays (ThreadScratch), held from construction to destruction
  QuantMatrix quant_;            // the working image's quant matrices
  float distance_ = 0.0f;        // ButteraugliComparator::distance_
  JpegHead head_;                // marker segments + codes of the last Serialize
  std::string best_head_;        // GuetzliOutput: head of the best candidate; its scan is
                                 // kept on the device (gz_jpeg_scan_keep)
  bool jpeg_input_ = false;      // Process(jpeg_data): tables / metadata of the input below
  FrameMeta meta_;
  Frame in_frame_;               // a 4:2:0 input as read (its own padding blocks)
  std::vector<QuantTable> in_quant_;
  int in_quant_idx_[3] = {0, 0, 0};
  int in_comp_id_[3] = {0, 1, 2};
  QuantMatrix q_in_;             // the input's quantisation per component (processor.cc:84-97)
  bool mirror_valid_ = false;    // sc_.img mirrors the device image (phase B)
  double best_score_ = -1;
  double timer_[kNumTimers] = {};
  long count_[kNumCounters] = {};
  int descend_levels_ = 6;       // levels to enqueue per descent (follows what the orders need)
  uint64_t head_bits_ = 0;       // scan bits of the candidate head_ was built for
  // the size model's code refreshes on helper threads (code_refresh.h); null: on this thread
  std::unique_ptr<CodeRefreshers> refreshers_;
  std::vector<SlowStep> slow_log_;
  long slow_steps_last_ = 0;           // serial steps of the previous iteration of phase B
  std::vector<int32_t> bulk_counts_;   // (kept between iterations: no allocation on the host's path)
};

}  // namespace guetzli_amd
#pragma GCC visibility pop
