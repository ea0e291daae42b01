// The caching allocator and the stream / event pools, gz_ctx (one image on one GPU), DeviceScope, the error macros, pinned staging (HostStage and its helpers, the result buffer), the plane arena.
// (part of the one translation unit gz_api.hip, which includes these files in order; split by
// concern in round 5 -- no declaration here is visible outside libguetzli_amd.so but the C ABI)
#pragma once


// ------------------------------------------------------------ caching allocator ------
// One image = one context = ~45 device allocations (0.5 GB at 1080p, 2 GB at 4K) and three
// pinned host buffers; hipMalloc / hipFree (which also synchronises the device) of those cost
// ~10 ms per image.  Freed blocks are kept in exact-size free lists per device and handed to
// the next context that asks for the same size -- a batch of same-sized images allocates once.
// GZ_POOL_MB bounds the cached device bytes per device (default 16384; 0 = no caching);
// gz_trim_pool() releases everything cached.  The emulation build allocates directly, so that
// its poisoning of fresh memory keeps catching reads of never-written buffers.
namespace {
// page-locked AND mapped into the device's address space: k_apply_coeff_edits and k_desc_export access
// staging buffers directly (the default flags give that on ROCm; said explicitly)
#ifdef GZ_EMU
constexpr unsigned kHostAllocFlags = 0;
#else
constexpr unsigned kHostAllocFlags = hipHostMallocMapped;
#endif
struct MemPool {
  std::mutex mu;
  std::unordered_map<void*, std::pair<int, size_t> > live;          // ptr -> (device, bytes)
  std::multimap<std::pair<int, size_t>, void*> idle;                // (device, bytes) -> ptr
  std::unordered_map<int, size_t> idle_bytes;                       // per device
};
MemPool& dev_pool() { static MemPool p; return p; }
MemPool& host_pool() { static MemPool p; return p; }
size_t pool_limit_bytes() {
  static const size_t lim = [] {
    const char* e = getenv("GZ_POOL_MB");
    return (size_t)(e ? std::max(0L, atol(e)) : 16384L) << 20;
  }();
  return lim;
}
void pool_release_idle(MemPool& p, bool host, int device /* -1: all */) {
  for (auto it = p.idle.begin(); it != p.idle.end();) {
    if (device >= 0 && it->first.first != device) { ++it; continue; }
    if (host) (void)hipHostFree(it->second); else (void)hipFree(it->second);
    p.idle_bytes[it->first.first] -= it->first.second;
    it = p.idle.erase(it);
  }
}
hipError_t pool_alloc(MemPool& p, bool host, void** out, size_t bytes) {
  if (bytes == 0) bytes = 1;
#ifdef GZ_EMU
  return host ? hipHostMalloc(out, bytes, kHostAllocFlags) : hipMalloc(out, bytes);
#else
  int device = 0;
  (void)hipGetDevice(&device);
  std::lock_guard<std::mutex> lk(p.mu);
  auto it = p.idle.find(std::make_pair(device, bytes));
  if (it != p.idle.end()) {
    *out = it->second;
    p.idle.erase(it);
    p.idle_bytes[device] -= bytes;
    p.live[*out] = std::make_pair(device, bytes);
    return hipSuccess;
  }
  hipError_t e = host ? hipHostMalloc(out, bytes, kHostAllocFlags) : hipMalloc(out, bytes);
  if (e != hipSuccess) {   // make room: drop what is cached on this device and try once more
    (void)hipGetLastError();
    pool_release_idle(p, host, device);
    e = host ? hipHostMalloc(out, bytes, kHostAllocFlags) : hipMalloc(out, bytes);
  }
  if (e == hipSuccess) p.live[*out] = std::make_pair(device, bytes);
  return e;
#endif
}
void pool_release(MemPool& p, bool host, void* ptr) {
  if (!ptr) return;
#ifdef GZ_EMU
  if (host) (void)hipHostFree(ptr); else (void)hipFree(ptr);
#else
  std::lock_guard<std::mutex> lk(p.mu);
  auto it = p.live.find(ptr);
  if (it == p.live.end()) {   // not ours
    if (host) (void)hipHostFree(ptr); else (void)hipFree(ptr);
    return;
  }
  const std::pair<int, size_t> key = it->second;
  p.live.erase(it);
  if (key.second <= pool_limit_bytes() && p.idle_bytes[key.first] + key.second > pool_limit_bytes())
    pool_release_idle(p, host, key.first);   // full of sizes nobody asks for any more: start over
  if (p.idle_bytes[key.first] + key.second <= pool_limit_bytes()) {
    p.idle.insert(std::make_pair(key, ptr));
    p.idle_bytes[key.first] += key.second;
  } else if (host) {
    (void)hipHostFree(ptr);
  } else {
    (void)hipFree(ptr);
  }
#endif
}
inline hipError_t pool_malloc(void** out, size_t bytes) { return pool_alloc(dev_pool(), false, out, bytes); }
inline void pool_free(void* ptr) { pool_release(dev_pool(), false, ptr); }
inline hipError_t pool_host_malloc(void** out, size_t bytes) { return pool_alloc(host_pool(), true, out, bytes); }
inline void pool_host_free(void* ptr) { pool_release(host_pool(), true, ptr); }

// Streams and (timing-less) events are pooled the same way: creating and destroying a
// context's four streams costs several milliseconds.  Only idle ones come back (the context
// synchronises its streams before it returns them).
struct HandlePool {
  std::mutex mu;
  std::multimap<int, hipEvent_t> events;
};
HandlePool& handle_pool() { static HandlePool p; return p; }
// Slots of the contexts alive per device (the lowest free one first).  A context's slot picks the rotation of its
// stream set (create_context), and the number of slots taken says whether the device has company (chain.h).
struct DeviceSlots {
  std::mutex mu;
  std::map<int, std::vector<bool> > used;
};
inline DeviceSlots& device_slots() { static DeviceSlots s; return s; }
// Takes the lowest free slot on `device`; *taken_before = the slots that were taken before.
inline int slot_take(int device, int* taken_before) {
  DeviceSlots& ds = device_slots();
  std::lock_guard<std::mutex> lk(ds.mu);
  std::vector<bool>& u = ds.used[device];
  *taken_before = (int)std::count(u.begin(), u.end(), true);
  for (size_t i = 0; i < u.size(); ++i) if (!u[i]) { u[i] = true; return (int)i; }
  u.push_back(true);
  return (int)u.size() - 1;
}
inline void slot_release(int device, int slot) {
  DeviceSlots& ds = device_slots();
  std::lock_guard<std::mutex> lk(ds.mu);
  std::vector<bool>& u = ds.used[device];
  if (slot >= 0 && (size_t)slot < u.size()) u[(size_t)slot] = false;
}
inline int slots_taken(int device) {
  DeviceSlots& ds = device_slots();
  std::lock_guard<std::mutex> lk(ds.mu);
  const std::vector<bool>& u = ds.used[device];
  return (int)std::count(u.begin(), u.end(), true);
}
// A context's four streams are created, pooled and reused TOGETHER.  The HIP runtime spreads streams
// over its hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in creation order, so four streams made
// back to back sit on four queues; pooled one by one (rounds 1-4), the streams that came back from the
// contexts of a batch were handed out in whatever order the threads had destroyed them, and a later
// context could get its main and side streams on ONE queue: its chain then ran serialised -- 1.58
// instead of 0.96 ms per Compare at 4K after a four-in-flight batch in the same process, a 4K
// quality-84 encode 0.177 instead of 0.150 s (profiles/r05_chain_experiments.log, section 10).
struct StreamSet {
  hipStream_t own = nullptr, side = nullptr, side2 = nullptr, entropy = nullptr;
};
struct StreamSetPool {
  std::mutex mu;
  std::multimap<int, StreamSet> sets;   // stream_set_key(): device, rotation, main stream at the highest priority (bit 0)
};
inline StreamSetPool& stream_set_pool() { static StreamSetPool p; return p; }
inline int stream_set_key(int device, bool prio_main, int rot) { return (device * 4 + rot) * 2 + (prio_main ? 1 : 0); }

// A set of rotation `rot` (0..3) is created in an order rotated by `rot`: its MAIN stream at position `rot` -- the
// hardware queue (mod 4) it sits on -- and its three other streams on the three other queues.  With every set made in
// the same order the main streams of the four images in flight all shared one queue, and a batch of eight 4K images
// fell from 39 to 32 MPix/s (section 10 of the experiment log).  prio_main: the main stream at the device's highest
// priority (who takes one: create_context).  Up to 4 idle sets are kept per key, 16 per device and priority.
hipError_t pool_stream_set_create(StreamSet* out, bool prio_main, int rot) {
#ifndef GZ_EMU
  int device = 0;
  (void)hipGetDevice(&device);
  StreamSetPool& p = stream_set_pool();
  std::lock_guard<std::mutex> lk(p.mu);   // (also keeps two threads' creations from interleaving)
  auto it = p.sets.find(stream_set_key(device, prio_main, rot));
  if (it != p.sets.end()) { *out = it->second; p.sets.erase(it); return hipSuccess; }
  hipStream_t* dst[4] = {&out->own, &out->side, &out->side2, &out->entropy};
  int least = 0, greatest = 0;
  const bool prio = prio_main && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
  hipError_t e = hipSuccess;
  for (int j = 0; j < 4 && e == hipSuccess; ++j) {
    const int which = (j + 4 - rot) & 3;   // position j of the creation order takes stream `which`: own at position rot
    e = which == 0 && prio ? hipStreamCreateWithPriority(dst[which], hipStreamDefault, greatest)
                           : hipStreamCreate(dst[which]);
  }
  return e;
#else
  hipError_t e = hipStreamCreate(&out->own);
  if (e == hipSuccess) e = hipStreamCreate(&out->side);
  if (e == hipSuccess) e = hipStreamCreate(&out->side2);
  if (e == hipSuccess) e = hipStreamCreate(&out->entropy);
  return e;
#endif
}
// The streams of a set that leaves the pool, or never got into it (a set whose creation failed half way has null ones).
inline void stream_set_teardown(const StreamSet& s_) {
  for (hipStream_t s : {s_.own, s_.side, s_.side2, s_.entropy}) if (s) (void)hipStreamDestroy(s);
}
void pool_stream_set_destroy(const StreamSet& s_, bool prio_main, int rot) {
#ifndef GZ_EMU
  if (s_.own && s_.side && s_.side2 && s_.entropy && pool_limit_bytes() != 0) {
    int device = 0;
    (void)hipGetDevice(&device);
    const int key = stream_set_key(device, prio_main, rot);
    StreamSetPool& p = stream_set_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.sets.count(key) < 4) { p.sets.insert(std::make_pair(key, s_)); return; }
  }
#endif
  stream_set_teardown(s_);
}
hipError_t pool_event_create(hipEvent_t* out) {
#ifndef GZ_EMU
  int device = 0;
  (void)hipGetDevice(&device);
  {
    HandlePool& p = handle_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    auto it = p.events.find(device);
    if (it != p.events.end()) { *out = it->second; p.events.erase(it); return hipSuccess; }
  }
#endif
  return hipEventCreateWithFlags(out, hipEventDisableTiming);
}
void pool_event_destroy(hipEvent_t e_) {
  if (!e_) return;
#ifndef GZ_EMU
  if (pool_limit_bytes() != 0) {
    int device = 0;
    (void)hipGetDevice(&device);
    HandlePool& p = handle_pool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.events.count(device) < 256) { p.events.insert(std::make_pair(device, e_)); return; }
  }
#endif
  (void)hipEventDestroy(e_);
}
}  // namespace

// Pinned host staging for the small per-iteration uploads (step lists, coefficient edits,
// next_cand, Huffman codes): the caller's buffer is copied here, the H2D copy is asynchronous
// and nobody has to wait for it -- the buffer is only waited for when it is reused.
// (stage_reserve / stage_sent and the result buffer: below the error macros they use)
struct HostStage {
  void* h = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool busy = false;
};

// What is in flight between a _begin and its _end: phase B's order, the descent enqueued behind it, and the Compare
// whose distance may arrive with them.  The transitions are the only writers (entry_phaseb.h, entry_compare.h, set_frame).
struct Pending {
  enum Landing { kNoOrder, kOwnBuffer, kResultsSlot };   // the order's results land in h_order_results / h_desc[kDescResultsSlot]
  enum Distance { kNoCompare, kMaxBits, kWithResults };  // gz_compare_end copies d_max_bits / finds the distance in the results slot too
  // how much a call makes void: the order and the descent behind it (gz_order_build_auto_end fails, gz_order_descend_end
  // returns nothing), the distance's ride with them too, and (a new frame) the Compare and the exported prefix as well
  enum Void { kOrder, kRide, kEverything };
  Landing order = kNoOrder;
  Distance compare = kNoCompare;
  int levels = -1;         // of the pending descent (-1: none)
  unsigned epoch = 0;      // the descent enqueued last (0: none yet): what its states in h_desc carry
  unsigned published = 0;  // the descent whose results slot the order's results and the distance are in
  bool exported = false;   // descent `epoch` ran k_desc_export into the host mirror
  bool busy() const { return order != kNoOrder || levels >= 0 || compare != kNoCompare; }
  unsigned next_epoch() { exported = false; if (++epoch == 0) epoch = 1; return epoch; }
  void compare_begun() { compare = kMaxBits; }
  void order_begun(Landing where) { order = where; }
  // published: its first level put the order's results -- and a pending Compare's distance -- into the results slot
  void descent_begun(int levels_, bool published_, bool exported_) {
    levels = levels_; exported = exported_;
    if (published_) { published = epoch; if (compare != kNoCompare) compare = kWithResults; }
  }
  void order_taken() { order = kNoOrder; }
  int descent_taken() { const int launched = levels; levels = -1; return launched; }
  void distance_taken() { compare = kNoCompare; }
  void mirror_replaced() { exported = false; }   // (what k_desc_export wrote went with the old array)
  void void_up_to(Void v) {
    order = kNoOrder; levels = -1;
    if (v >= kRide && compare == kWithResults) compare = kMaxBits;
    if (v == kEverything) { compare = kNoCompare; exported = false; }
  }
};

struct gz_ctx {
  // What the context owns: the ADDRESSES of its members that hold a device block, a pinned block or an event, each
  // entered once, when regrow() / own_event() first fill it (the context lives on the heap and never moves).
  // gz_destroy gives back what they hold by walking these two lists; nothing else frees a member.
  struct Owned { void** p; bool host; };
  std::vector<Owned> owned;
  std::vector<hipEvent_t*> owned_events;
  // The groups made on first use, each made only through its mark here (regrow() below: set last)
  struct Made { bool entropy = false, rank = false, order_blocks = false, part = false, descent = false, step_delta = false, scan_state[2] = {false, false}, silver = false, emit = false, heat = false; } made;
  int device = 0;
  int w = 0, h = 0, bw = 0, bh = 0, nb = 0, pitch = 0;
  size_t plane = 0;   // floats per plane
  // The current frame (OutputImage's component layout): chroma subsampling factor 1 (4:4:4)
  // or 2 (4:2:0: OutputImageComponent::Reset(2, 2), output_image.cc:40-49), the chroma block
  // grid under it, the first block of every component in d_orig / d_cand, blocks in total.
  int cfac = 1, cbw = 0, cbh = 0, nbc = 0, coff[3] = {0, 0, 0}, nblk = 0;
  uint8_t* d_csamp = nullptr;      // 4:2:0: IDCT samples of the two chroma components (k_chroma_samples)
  // grid of the last block search (gz_block_zeroing_orders*), which phase B's order works on
  int sg_w = 0, sg_h = 0, sg_n = 0, sg_factor = 1, sg_mask = 7;
  float* d_gmax = nullptr;         // per-16x16 maxima of the distance map (sg_factor == 2)
  // scratch of k_scan_offsets, one set per stream that runs it (main: order build; entropy: scan)
  void* d_scan_state[2] = {nullptr, nullptr};
  unsigned scan_epoch[2] = {0, 0};
  float target = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // second stream for the branch of Compare that does not depend on the Malta path (the
  // mask: DiffPrecompute + three blurs), forked and joined with events
  hipStream_t side_stream = nullptr, side_stream2 = nullptr;
  bool prio_streams = false;   // (see create_context)
  bool compare_forked = false;   // the Compare enqueued last went onto the side streams too (written by chain.h enqueue_compare only)
  gz_config cfg;             // run-time configuration (include/guetzli_amd.h): the environment's, read once at gz_create
  int slot = -1;             // the context's slot on its device (slot_take); its stream set has rotation slot % 4
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr, ev_mask_pre = nullptr;
  hipEvent_t ev_next_cand = nullptr;   // next_cand uploaded beside a Compare chain in flight
  hipEvent_t ev_xyb = nullptr, ev_lfy = nullptr;   // B plane's LF blur on side stream 2 (stage_separate)
  // the entropy coder's kernels (gz_jpeg_scan) run on their own stream, beside a Compare that
  // gz_compare_begin has put on the main stream: both only read the candidate coefficients
  hipStream_t entropy_stream = nullptr;
  hipEvent_t ev_candidate = nullptr;   // main stream: the candidate is in place
  hipEvent_t ev_ingest = nullptr;      // gz_set_rgb_device: the producer's stream has written the source (made on first use)
  hipEvent_t ev_emit = nullptr;        // gz_reconstruct_device: the consumer's stream before, this context's stream behind the emit kernel (made on first use)
  float* d_emit_lut = nullptr;         // ... and the float32 elements of the 256 bytes (made.emit)
  float* d_heat_tab = nullptr;         // gz_heatmap_device: those 256 floats, and behind them the 255 thresholds of a byte (made.heat)
  std::string err;

  uint8_t* d_rgb = nullptr;
  int16_t* d_orig = nullptr;   // [3][nb][64] original coefficients
  int16_t* d_cand = nullptr;   // candidate coefficients
  int* d_q = nullptr;          // [3][64]
  float* d_srgb_lut = nullptr; // float(Srgb8ToLinearTable[i])
  double* d_mask_luts = nullptr;
  float* d_block_max = nullptr;
  // [kResultWords]: [0] the image maximum the chain accumulates (its float bits); behind it, so that ONE copy fetches
  // them with the distance, what the linear entries count (entry_linear.h): [kWordClamped] the elements k_ingest_linear
  // altered, [kWordRegionMax] k_region_max's maximum of a small image's window.  Each is cleared by a fill in front of
  // the kernel that accumulates into it.
  enum { kWordClamped = 1, kWordRegionMax = 2, kResultWords = 4 };
  unsigned* d_max_bits = nullptr;
  uint8_t* d_srgb_out = nullptr;
  int32_t* d_blkidx = nullptr; size_t blkidx_cap = 0;
  int16_t* d_blkdata = nullptr;

  float* arena = nullptr;
  float* extra_arena = nullptr;   // probe-only planes (ensure_pip)
  // A batched chain (entry_batch.h; n == 0: none, the state of every context the other entries make).  The context's plane
  // pointers are then image 0's of n arenas laid out back to back, and every launch of the chain's dispatchers (chain.h)
  // covers the n images: idx moves the kernels' pointers, max_bits are the n image-maximum words.
  struct Batch { int n = 0; BatchIdx idx = {0, 0}; unsigned* max_bits = nullptr; } batch;
  std::vector<float*> free_planes;
  BlurCfg blur[B_COUNT];

  Psycho pi0;   // original
  Psycho pi1;   // candidate
  Psycho pip;   // probe "image 0" (allocated lazily)
  bool have_pip = false;
  // scratch
  float *lin[3], *tmp[3], *xyb[3], *lf_raw[2], *hfp[2];
  float *snb, *diffx, *diffy, *mxb, *myb1, *myb2, *ac[2], *dsq, *distmap;
  float* sup0[2];   // the original's half of DiffPrecompute (k_mask_sup of pi0: X, Y), per image
  float* sup_scratch[2] = {nullptr, nullptr};   // the same for Mask() on raw planes (block mask, probe)
  float *mask_out[3], *mask_dc_out[3];

  float* d_block_mask = nullptr;   // [3][nb] mask_xyz_ at block corners (StartBlockComparisons)
  bool have_block_mask = false;   // (see "What the flags claim" below)
  int32_t* d_rank_cnt = nullptr; uint8_t* d_rank_idx = nullptr; float* d_rank_tables = nullptr;
  int32_t* d_out_cnt = nullptr; uint8_t* d_out_idx = nullptr; float* d_out_err = nullptr;
  int32_t* d_csr_off = nullptr;   // the search's CSR offsets (k_csr_offsets); the packed indices reuse d_rank_idx

  // device entropy coder (gz_kernels_entropy.h)
  int* d_jq = nullptr;                    // [3][64] quant matrices of the frame being written
  unsigned* d_hist = nullptr;             // [2][3][256]
  unsigned char* d_code_depth = nullptr;  // [2][3][256]
  unsigned short* d_code_bits = nullptr;  // [2][3][256]
  unsigned* d_mcu_bits = nullptr;         // [nb]
  unsigned long long* d_mcu_off = nullptr;   // [nb+1]
  unsigned long long* d_ff_count = nullptr;
  unsigned* d_words = nullptr; size_t words_cap = 0;        // scan bits of the last gz_jpeg_scan
  unsigned* d_words_kept = nullptr; size_t words_kept_cap = 0;
  unsigned long long scan_bits = 0, scan_ff = 0, kept_bits = 0, kept_ff = 0;
  bool have_jq = false, have_scan = false, have_kept = false;
  bool scan_pending = false;           // between gz_jpeg_scan_begin and _end
  void* h_scan_result = nullptr;       // pinned: total bits, 0xFF count of the scan in flight

  // global candidate order of phase B (gz_kernels_order.h)
  OrderEntry* d_order = nullptr; size_t order_cap = 0; size_t order_n = 0;
  unsigned* d_pos_l = nullptr; unsigned* d_pos_r = nullptr;       // [order_cap]
  unsigned* d_chunk = nullptr; size_t chunk_cap = 0;              // cnt_l, cnt_r, base_l, base_r
  PartScalars* d_part = nullptr;
  // gz_order_build_auto_begin .. _end: results land here (pinned; not the shared landing area,
  // which gz_compare_end uses in between)
  struct OrderResults { unsigned long long total; unsigned counters[2]; };
  OrderResults* h_order_results = nullptr;
  // quick-select descent decided on the device (gz_order_descend*): per-level ranges and pivots, the ranges' pinned
  // copy for the host's replay [kDescStates] -- with gz_order_build_auto_descend_begin the order's counters (and the
  // distance of the Compare in flight) arrive in it too, in h_desc[kDescResultsSlot]
  DescState* d_desc_st = nullptr; DescPivot* d_desc_pv = nullptr; DescState* h_desc = nullptr;
  Pending pending;
  void* h_order_mirror = nullptr;      // gz_order_host_mirror: pinned, order entries land in it directly
  size_t order_mirror_cap = 0;         // entries
  unsigned* d_order_nb = nullptr;                                 // [nb]
  unsigned long long* d_order_off = nullptr;                      // [nb+1]: [nb] = the order's size; the first 4 nb BYTES: every block's offset inside its group
  unsigned* d_order_counters = nullptr;                           // [2]
  unsigned* d_order_groups = nullptr;                             // [2 * ceil(nb / kOrderGroup)]: sum of n_b, blocks with n_b > 0
  int* d_next_cand = nullptr; float* d_weight = nullptr; float* d_max_err = nullptr;   // [nb]
  bool adv_pending = false; float adv_threshold = 0.0f; int adv_direction = 0;         // gz_order_advance's update, still due
  bool have_search = false;
  unsigned char* d_wflag = nullptr;                               // [nb]
  int* d_edit_pos = nullptr; short* d_edit_val = nullptr; size_t edit_cap = 0;

  // ---- What the flags claim.
  // The original: have_orig (d_orig holds its coefficients), have_block_mask (d_block_mask is StartBlockComparisons'
  // mask of d_rgb); pi0 and sup0 have no flag: gz_set_rgb writes them, and a failed gz_set_rgb leaves them undefined.
  // The candidate: have_cand (d_cand holds one), and what is derived from it: lin_is_cand, xyb_is_cand, have_distmap
  // (the last Compare's distance map and block maxima are in place), h_block_max_valid (h_block_max is d_block_max).
  // Pending two-phase calls: `pending` (the order, its descent, the Compare: written by Pending's transitions only),
  // scan_pending, adv_pending.  A pending state is entered as the last state change before `return GZ_OK`; a call that
  // replaces what a pending call worked on voids it first (void_up_to), and a voided call's _end fails or returns nothing.
  // Memory has no claim of its own: a group of buffers made on first use is there if and only if its mark in `made` is
  // set, and the mark is set behind the group's allocations AND its initialising memsets / copies (regrow, below).
  // Rules:  DROP BEFORE WRITE -- a call that writes d_orig, d_cand, d_rgb / pi0, lin[] or xyb[] drops every claim that
  // depends on that buffer before its first copy or launch.  RE-ARM ONLY ON SUCCESS -- a claim is set again only as the
  // last state change before `return GZ_OK`.  Dropping is always safe: it costs one full reconstruction or opsin pass.
  bool have_orig = false, have_cand = false, have_distmap = false;
  // The original is a linear float image (gz_create_from_device_linear / gz_set_linear_device, entry_linear.h): pi0 and
  // sup0 are its, d_rgb is NOT -- there are no 8-bit pixels of it, so no coefficients either.  The entries that read
  // d_rgb or d_orig refuse such a context (byte_original below); gz_set_rgb* give it an 8-bit original again and clear
  // this.  Set as the last state change of a successful call, dropped before the first write of a new original.
  bool orig_linear = false;
  unsigned long long orig_clamped = 0;   // elements of that image the value rule altered (gz_kernels_ingestlin.h)
  // c->distmap holds the distance map of the last comparison (gz_distmap_device emits it): only a comparison asked for
  // its map stores one (kWantDistmap), and the plane is scratch of every SeparateFrequencies (stage_separate drops this)
  bool have_map_plane = false;
  // lin[] holds the reconstruction of d_cand as it is now (4:4:4 frames; cfg.patch_reconstruct): set by the Compare
  // chain's full reconstruction, kept by the mutators that transform the block positions they change
  // (gz_apply_candidate_steps, gz_apply_coeff_edits: PatchClaims), dropped by everything else that writes d_cand or lin[]
  bool lin_is_cand = false;
  // ... and xyb[] the opsin image of those planes (cfg.opsin_ahead): the Compare chain's second kernel enqueued AHEAD,
  // behind the bulk steps' patches, while the host takes its serial steps; their edits then cost the opsin tiles around
  // the edited blocks (gz_apply_coeff_edits), and the Compare starts at its third kernel.  Consumed by that Compare.
  bool xyb_is_cand = false;
  std::vector<unsigned char> tile_mark;   // opsin tiles already listed (gz_apply_coeff_edits)
  std::vector<float> h_block_max;
  bool h_block_max_valid = false;
  int h_jq[192] = {0};       // the matrix d_jq holds
  unsigned* d_step_delta = nullptr; bool have_step_delta = false;   // AC statistics change of the last bulk steps
  hipEvent_t ev_steps = nullptr; bool step_delta_event = false;     // ... are in place (recorded when more work follows them on the stream)
  void* h_step_delta = nullptr;   // ... as k_steps_hist_sum writes it: 768 ints, page-locked + mapped
  HostStage stage_main, stage_entropy;
  HostStage stage_edits;   // gz_apply_coeff_edits' own: its kernel reads the buffer, and the next order's upload (stage_main) must not wait for it
  // pinned landing area for the small results every call waits for (a copy into pageable
  // memory costs 27 us per round trip on this system, into pinned memory 15)
  void* h_res = nullptr; size_t h_res_cap = 0;
  void* d_cmp_stage = nullptr; size_t cmp_stage_cap = 0;   // gz_compare_blocks / _block_pixels staging
  // gz_downsample_silver (made.silver): the list of cells for the host, GammaToLinear of a byte, the pinned + mapped staging
  unsigned* d_silver_list = nullptr; float* d_silver_lut = nullptr; float* h_silver = nullptr;
  size_t search_total = 0;   // candidates phase A produced (bounds every global order)
  unsigned long long search_evaluations = 0;   // CompareBlock evaluations of the last block search
  float last_distance = 0.0f;
};

// Every context entry point runs with the context's device current and leaves the caller's
// device as it found it: a thread may own contexts on several GPUs (the pools key on the
// current device, kernels launch on it).
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(const gz_ctx* c) {
    if (!c) return;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
    if (cur != c->device) {
      (void)hipSetDevice(c->device);
      prev = cur;
    }
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};
// Its counterpart for the entries without a context, which make `device` current on their way (create_context,
// probe_device): the caller's device stays current.  It is remembered here -- if it cannot be asked for, there is
// nothing to restore -- and restored at the end of the scope if it is another one than `device`.
struct CallerDevice {
  int device, prev = -1;
  explicit CallerDevice(int device_) : device(device_) {
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
  }
  ~CallerDevice() { if (prev >= 0 && prev != device) (void)hipSetDevice(prev); }
  CallerDevice(const CallerDevice&) = delete;
  CallerDevice& operator=(const CallerDevice&) = delete;
};
// A context that lives for one call (declared behind the call's CallerDevice: destroyed before the device is restored).
struct CallContext {
  gz_ctx* c;
  explicit CallContext(gz_ctx* c_) : c(c_) {}
  ~CallContext() { gz_destroy(c); }   // (synchronises the streams whatever was enqueued, then everything goes back to the pools)
  CallContext(const CallContext&) = delete;
  CallContext& operator=(const CallContext&) = delete;
};

namespace {

#define HIPCHK(ctx, call)                                                            \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) {                                                          \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                \
      return e_ == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP;                      \
    }                                                                                \
  } while (0)

#define KCHK(ctx)                                                                    \
  do {                                                                               \
    hipError_t e_ = hipGetLastError();                                               \
    if (e_ != hipSuccess) {                                                          \
      (ctx)->err = std::string("kernel launch: ") + hipGetErrorString(e_);           \
      return GZ_E_HIP;                                                               \
    }                                                                                \
  } while (0)

// For the entries that read d_rgb or d_orig: a context whose original is a linear float image has neither.
static int byte_original(gz_ctx* c, const char* who) {
  if (!c->orig_linear) return GZ_OK;
  c->err = std::string(who) + ": the context's original is a linear float image (gz_create_from_device_linear / gz_set_linear_device), "
           "which has no 8-bit pixels and no coefficients; gz_set_rgb* gives the context an 8-bit original";
  return GZ_E_STATE;
}

// The one way a context comes by memory: the buffers of `bufs`, device or pinned, all of them or none.  What they held
// goes back to the pool first, the pointers null and the capacity zero BEFORE the allocations that may fail; if one
// fails, those already obtained go back too (nothing is left half-owned).  Every member is entered into the context's
// record the first time it is filled.
// Growing buffers that share a capacity: `cap` is set behind the last allocation, and the old buffers are given back
// behind everything on `behind`, if given: the pool hands memory on without waiting.
// A group made once: cap == nullptr, and the caller sets the group's mark (gz_ctx::made) as its LAST statement, behind
// the memsets and copies that initialise the group -- a failed attempt is repeated in full by the next call, which waits
// for `behind` only if that attempt left it something to give back.
struct Regrown { void** p; size_t bytes; bool host = false; };
static void give_back(void** p, bool host) { if (host) pool_host_free(*p); else pool_free(*p); *p = nullptr; }
static int regrow(gz_ctx* c, hipStream_t behind, size_t* cap, size_t new_cap, std::initializer_list<Regrown> bufs) {
  const bool held = std::any_of(bufs.begin(), bufs.end(), [](const Regrown& b) { return *b.p != nullptr; });
  if (behind && (cap || held)) HIPCHK(c, hipStreamSynchronize(behind));
  for (const Regrown& b : bufs) give_back(b.p, b.host);
  if (cap) *cap = 0;
  for (const Regrown& b : bufs) {
    const hipError_t e = b.host ? pool_host_malloc(b.p, b.bytes) : pool_malloc(b.p, b.bytes);
    if (e != hipSuccess) {
      *b.p = nullptr;
      for (const Regrown& u : bufs) give_back(u.p, u.host);
      (void)hipGetLastError();   // (the repeated call's first launch check must not find this failure)
      c->err = std::string(b.host ? "pinned" : "device") + " allocation of " + std::to_string(b.bytes) + " bytes: " + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP;
    }
    if (std::none_of(c->owned.begin(), c->owned.end(), [&](const gz_ctx::Owned& o) { return o.p == b.p; })) c->owned.push_back({b.p, b.host});
  }
  if (cap) *cap = new_cap;
  return GZ_OK;
}
// ... and by an event (one member, filled once).
static int own_event(gz_ctx* c, hipEvent_t* e) {
  HIPCHK(c, pool_event_create(e));
  c->owned_events.push_back(e);
  return GZ_OK;
}
// gz_destroy's walk of the record (the caller has synchronised the streams).
static void release_owned(gz_ctx* c) {
  for (hipEvent_t* e : c->owned_events) { pool_event_destroy(*e); *e = nullptr; }
  for (const gz_ctx::Owned& o : c->owned) give_back(o.p, o.host);
  c->owned_events.clear();
  c->owned.clear();
}

// Reserves `bytes` of the staging buffer (waiting for its previous upload if that is still
// running) and returns it; stage_sent() marks the upload that was just enqueued on `stream`.
static int stage_reserve(gz_ctx* c, HostStage* st, size_t bytes, void** out) {
  if (!st->ev) if (int rc = own_event(c, &st->ev)) return rc;
  if (st->busy) {
    HIPCHK(c, hipEventSynchronize(st->ev));
    st->busy = false;
  }
  if (bytes > st->cap) {
    const size_t cap = bytes + bytes / 2 + 4096;
    if (int rc = regrow(c, nullptr, &st->cap, cap, {{&st->h, cap, true}})) return rc;
  }
  *out = st->h;
  return GZ_OK;
}
static int stage_sent(gz_ctx* c, HostStage* st, hipStream_t stream) {
  HIPCHK(c, hipEventRecord(st->ev, stream));
  st->busy = true;
  return GZ_OK;
}
static int result_buffer(gz_ctx* c, size_t bytes, void** out) {
  if (bytes > c->h_res_cap) {
    const size_t cap = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    if (int rc = regrow(c, nullptr, &c->h_res_cap, cap, {{&c->h_res, cap, true}})) return rc;
  }
  *out = c->h_res;
  return GZ_OK;
}

const int kNumPlanes = 9 + 9 + 3 + 3 + 3 + 2 + 2 + 10 + 2;   // pi0, pi1, lin, tmp, xyb, lf_raw, hfp, 10 singles, sup0[2]
// Floats from one image's arena to the next in a batched context: the planes, rounded up to a multiple of 4 floats (an
// image's planes are then 16-byte aligned exactly where image 0's are).
inline size_t batch_arena_stride(size_t plane) { return (plane * kNumPlanes + 3) & ~(size_t)3; }

// A new frame layout: the candidate, the search and whatever was pending or kept belonged to the old one (a stale
// gz_order_build_auto_end / gz_order_descend_end / gz_compare_end / gz_jpeg_scan_end must fail, not return its data).
void set_frame(gz_ctx* c, int factor) {
  c->cfac = factor;
  c->cbw = (c->w + 8 * factor - 1) / (8 * factor);
  c->cbh = (c->h + 8 * factor - 1) / (8 * factor);
  c->nbc = c->cbw * c->cbh;
  c->coff[0] = 0;
  c->coff[1] = c->nb;
  c->coff[2] = c->nb + c->nbc;
  c->nblk = c->nb + 2 * c->nbc;
  c->have_cand = false;
  c->lin_is_cand = c->xyb_is_cand = false;
  c->have_search = false;
  c->pending.void_up_to(Pending::kEverything);
  c->scan_pending = false;
  c->have_distmap = c->have_map_plane = false;
  c->have_scan = false;
}
size_t csamp_plane(const gz_ctx* c) {   // bytes of one chroma sample plane of a 4:2:0 frame
  return (size_t)((c->w + 15) / 16 * 8) * (size_t)((c->h + 15) / 16 * 8);
}

float* take_plane(gz_ctx* c) {
  float* p = c->free_planes.back();
  c->free_planes.pop_back();
  return p;
}
void alloc_psycho(gz_ctx* c, Psycho* p) {
  for (int i = 0; i < 3; ++i) p->lfv[i] = take_plane(c);
  for (int i = 0; i < 2; ++i) p->mf[i] = take_plane(c);
  for (int i = 0; i < 2; ++i) p->hf[i] = take_plane(c);
  for (int i = 0; i < 2; ++i) p->uhf[i] = take_plane(c);
}

}  // namespace
