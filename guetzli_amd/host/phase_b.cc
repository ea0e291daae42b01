// Phase B of the search: SelectFrequencyMasking (processor.cc:539-780).
#include <string.h>

#include <exception>
#include <optional>

#include "device_order.h"
#include "encoder.h"
#include "parallel.h"

namespace guetzli_amd {

// ---------------------------------------------------------------------------------------------------
// SelectFrequencyMasking (processor.cc:539-780), in the pieces it is made of (round 6: one 716-line function
// until then).  MaskSearch = what one search owns: the state it keeps between its iterations, `it` = the
// current pass of the reference's loop body (:607-772) with its order.  Order of the calls, of the device's entry
// points and of every decision is the reference's; the --verbose trace test and the byte-exact goldens hold it there.
//   SearchBlocks            phase A on the device + the size model of the starting point
//   AcquireOrder            the iteration's global order (built ahead behind the last evaluation, or now)
//   BulkSteps               the steps no estimate can observe: device descent, prefix, per-block counts
//   TakeStep                one serial step without its price (PriceStep, or the refresh of the codes)
//   StepsAsTheReference     the reference's serial loop over [from, to)
//   StepsWithHelpers        the same decisions with the code refreshes on helper threads
//   EvaluateCandidate       edits to the device, evaluation + next order enqueued, exact size only if it can win
//   SettleBlock / SettleAll the host mirror of the image catching up
struct Encoder::MaskSearch {
  MaskSearch(Encoder& enc, int mask, double mul, int last_c)
      : e(enc), comp_mask(mask), target_mul(mul), factor(last_c > 0 ? enc.fac_ : 1),
        nb(factor == 2 ? enc.nbc_ : enc.nb_), ncomp(enc.jpg_ncomp_) {}
  bool Run(bool stop_early, bool last_search_of_round);
  bool SearchBlocks(Stopwatch* sw);
  void RecountRawBits() {
    for (int c = 0; c < ncomp; ++c) ac_raw_bits[c] = HistogramRawBits(ac_histo[c], &ac_depths[c * kHistoSize]);
  }
  size_t DataBytes() const {   // EntropyDataSize(ac_histo, ncomp, ac_depths) from the raw bits that follow the steps
    size_t data_bits = 0;
    for (int c = 0; c < ncomp; ++c) data_bits += EntropyBitsFromRaw(ac_raw_bits[c]);
    return (data_bits + 7) / 8;
  }
  int EstimateSize() const { return header_size + dc_size + ac_header + (int)DataBytes(); }
  void SettleBlock(int b);
  void SettleAll();
  bool AcquireOrder();
  bool BulkSteps(size_t fast_until);
  void PrefetchFor(size_t i);
  void TakeStep(size_t i, SlowStep* st);
  void PriceStep(const SlowStep& st);
  void UndoStep(const SlowStep& st);
  bool StepsAsTheReference(size_t from, size_t to);
  void StepsWithHelpers(size_t base);
  bool EvaluateCandidate(Stopwatch* sw);
  bool Helpers() const { return e.refreshers_ && !e.knobs_.verify(); }   // the code refreshes go to helper threads

  Encoder& e;
  const int comp_mask;
  const double target_mul;
  const int factor, nb, ncomp;   // the grid of the mask's last component (:548-552), the frame's components
  // the size model (:592-604): symbol statistics, the parts of the estimate, the AC codes' depths and the
  // raw bits HistogramRawBits gives for them (kept incrementally between refreshes)
  SymbolHistogram dc_histo[3], ac_histo[3];
  int header_size = 0, dc_size = 0, ac_header = 0, base_size = 0, prev_size = 0;
  std::vector<uint8_t> ac_depths;
  int64_t ac_raw_bits[3] = {0, 0, 0};
  std::vector<int> next_cand;     // last_indexes: how far every block has advanced
  std::vector<int> mirror_cand;   // ... and up to where the host mirror sc_.img has followed (SettleBlock)
  std::vector<int32_t> edit_pos;  // coefficient changes of one iteration
  std::vector<int16_t> edit_val;
  std::vector<char> touched;      // blocks changed in this iteration (listed in `dirty`)
  std::vector<int32_t> dirty, first_touch;
  std::vector<int> step_count;
  bool first_up = true;
  // the next iteration's order, constructed on the device behind the evaluation (EvaluateCandidate): the
  // direction it was built for (0: none in flight) and the partitions the device made behind it
  int ahead = 0;
  uint64_t ahead_log[3 * 12];
  int ahead_levels = 0;
  uint64_t ahead_last = 0;
  // the current pass of the reference's loop body (:607-772) and its order
  struct Iteration {
    int direction = 1;
    float below_limit = 0.0f, per_block = 0.0f;
    uint64_t total = 0, below = 0;        // the order's size; its keys below the limit (first "up" iteration)
    int blocks_to_change = 0;
    bool have_ahead_log = false;          // the device's descent came with the order
    std::pair<int, float>* order = nullptr;   // the context's page-locked mirror of the order's fetched ranges
    size_t n_order = 0;
    double min_size_delta = 0.0;
    int min_coeffs_to_change = 0;
    float val_threshold = 0.0f;
    int changed_coeffs = 0;
    int est_size = 0;
    bool verify_failed = false;
  } it;
  std::optional<DeviceOrder> dev_order;
  std::optional<SortedOrder> sorted;
};

// last_search_of_round: no other search of this frame follows (its host mirror of the image is not read again)
bool Encoder::SelectFrequencyMasking(int comp_mask, double target_mul, bool stop_early,
                                     bool last_search_of_round) {   // processor.cc:539-780
  int last_c = 0;
  for (int c = 0; c < 3; ++c)
    if (comp_mask & (1 << c)) last_c = c;
  if (last_c >= jpg_ncomp_) return true;   // :546-547
  MaskSearch ms(*this, comp_mask, target_mul, last_c);
  return ms.Run(stop_early, last_search_of_round);
}

bool Encoder::MaskSearch::Run(bool stop_early, bool last_search_of_round) {
  Stopwatch sw;
  if (!e.refreshers_) {
    const int t = e.CodeRefreshThreads();
    if (t > 0) {
      try {
        e.refreshers_.reset(new CodeRefreshers(t));
      } catch (const std::exception&) {   // (no thread to be had: the reference's serial loop)
        e.refreshers_.reset();
      }
    }
  }
  if (!SearchBlocks(&sw)) return false;

  int rc = gz_order_reset(e.ctx_);           // max_block_error := 0, kept on the device
  if (rc != GZ_OK) return e.Fail("gz_order_reset", rc);
  next_cand.assign(nb, 0);     // last_indexes
  mirror_cand.assign(nb, 0);
  touched.assign(nb, 0);
  step_count.assign(nb, 0);
  const size_t device_threshold = e.knobs_.order_device_threshold;
  long* const n = e.count_;
  double* const t = e.timer_;

  for (int direction = 1; direction >= -1; direction -= 2) {
    for (;;) {
      if (stop_early && direction == -1) {
        // down-adjusting only makes the output larger (:613-621)
        if (prev_size > 1.01 * (double)e.best_size_) break;
      }
      it = Iteration();
      it.direction = direction;
      it.below_limit = 0.75f * e.params_.butteraugli_target;   // 0.75f * BlockErrorLimit()
      Stopwatch pw;
      if (!AcquireOrder()) return false;
      t[kTOrder] += pw.lap();
      if (it.total == 0) break;
      // (an iteration takes about as many serial steps as the one before it: after a long one the helpers
      // are woken now, while the prefix is selected and the bulk steps are applied)
      if (Helpers() && e.slow_steps_last_ >= 30) e.refreshers_->Activate();
      n[kNOrder] += (long)it.total;
      {
        void* mirror = nullptr;
        rc = gz_order_host_mirror(e.ctx_, it.total, &mirror);
        if (rc != GZ_OK) return e.Fail("gz_order_host_mirror", rc);
        it.order = static_cast<std::pair<int, float>*>(mirror);
      }
      it.n_order = (size_t)it.total;

      // The reference std::sort-s `order` here (processor.cc:675-678) and then consumes a
      // prefix.  Equal keys occur across different blocks and std::sort is not stable, so
      // the permutation must be libstdc++'s; LazySorted yields exactly that permutation,
      // front first, without sorting the part the scan never reaches.  The partitions of the
      // large ranges run on the device (gz_order_partition); ranges that have become small
      // are fetched and finished here.
      dev_order.emplace(e.ctx_, t, n);
      sorted.emplace(it.order, it.n_order, OrderKeyLess(), -1, 1 << 17, &*dev_order, device_threshold);
      t[kTSort] += pw.lap();

      double rel_size_delta = direction > 0 ? 0.01 : 0.0005;
      if (direction > 0 && e.DistanceOK(1.0)) rel_size_delta = 0.05;
      it.min_size_delta = base_size * rel_size_delta;
      it.per_block = direction > 0 ? 2.0f : factor * factor * 0.2f;
      it.min_coeffs_to_change = it.per_block * it.blocks_to_change;
      if (first_up) {
        // partition_point over the sorted sequence == number of keys below the limit
        it.min_coeffs_to_change = std::max<int>(it.min_coeffs_to_change, (int)it.below);
        first_up = false;
      }

      t[kTSort] += pw.lap();
      // (touched[] and step_count[] are all zero here: whoever sets an entry records the block in
      // `dirty`, and the entries of the blocks in `dirty` are cleared before the list is)
      for (int32_t b : dirty) { touched[b] = 0; step_count[b] = 0; }
      dirty.clear();
      edit_pos.clear();
      edit_val.clear();
      it.est_size = prev_size;
      // The stopping rule can only fire once changed_coeffs > min_coeffs_to_change, and the
      // size estimate of step i uses the Huffman depths refreshed at the last multiple of 10
      // not above i.  Up to that refresh point nothing the estimate produces is observable,
      // so those steps only edit coefficients ("fast steps"); the symbol statistics are
      // rebuilt once after them.
      {
        const size_t n_order = it.n_order;
        const size_t last_needed = std::min<size_t>((size_t)std::max(it.min_coeffs_to_change, 0), n_order - 1);
        const size_t fast_until = last_needed / 10 * 10;
        if (!BulkSteps(fast_until)) return false;
        n[kNSteps] += (long)fast_until;
        n[kNFast] += (long)fast_until;
        const long slow_steps_before = n[kNSteps] - n[kNFast];
        // EntropyDataSize(ac_histo, ncomp, ac_depths) after every step, without its pass over the
        // histograms: ac_raw_bits[c] follows HistogramRawBits(ac_histo[c], depths of c) through
        // the serial steps and is recounted when the depths change
        RecountRawBits();
        // Three quarters of an encode's iterations stop within ten steps of the bulk (the first
        // refresh's estimate already differs enough): waking the helpers for those costs more than the
        // one refresh they could take over.  An iteration takes about as many serial steps as the one
        // before it: after a short one the first windows are taken as the reference takes them, and
        // the helpers are called in only if the loop goes on.
        size_t base = fast_until;   // first step of the pipelined part (a multiple of 10)
        bool stopped_early = false;
        const long serial_first = e.knobs_.code_serial_steps;   // (the tests: 0 = helpers from the first step on)
        if (Helpers() && serial_first > 0 && e.slow_steps_last_ < serial_first) {
          const size_t to = std::min(n_order, fast_until + (size_t)serial_first);
          stopped_early = StepsAsTheReference(fast_until, to);
          base = to;
        }
        if (Helpers() && !stopped_early && base < n_order) {
          StepsWithHelpers(base);
        } else if (!Helpers()) {
          (void)StepsAsTheReference(fast_until, n_order);
          if (it.verify_failed) return false;
        }
        e.slow_steps_last_ = n[kNSteps] - n[kNFast] - slow_steps_before;
      }
      if (e.refreshers_) e.refreshers_->Deactivate();
      t[kTLoop] += pw.lap();
      if (sorted->failed()) return e.Fail("gz_order_partition/fetch", dev_order->rc);
      if (dev_order->log_n > 0) {
        // as many levels next time as this order needed, plus one in reserve (an unused level
        // costs two empty launches, a missing one a round trip per partition)
        e.descend_levels_ = std::min(12, std::max(2, dev_order->log_n + (dev_order->n_partition > 0 ? 2 : 1)));
      }
      rc = gz_order_advance(e.ctx_, it.val_threshold, direction);   // max_block_error += weight * ...
      if (rc != GZ_OK) return e.Fail("gz_order_advance", rc);

      ++e.stats_->counters[kNumItersCnt];
      ++e.stats_->counters[direction > 0 ? kNumItersUpCnt : kNumItersDownCnt];
      t[kTPhaseB] += sw.lap();
      if (!EvaluateCandidate(&sw)) return false;
      prev_size = it.est_size;
      sw.lap();
    }
    // (sc_.img is exact for the blocks the serial steps visited; the others catch up when they are
    // visited -- or here, if the whole mirror is going to be read)
    if (e.knobs_.verify() || (direction == -1 && !last_search_of_round)) SettleAll();
  }
  if (e.knobs_.check_mirror) {
    // self-check of the lazily maintained mirror (the tests): every block caught up now, the host's
    // image must be the device's, coefficient for coefficient
    SettleAll();
    std::vector<int16_t> co((size_t)e.nblk_ * 64);
    rc = gz_get_coeffs(e.ctx_, co.data());
    if (rc != GZ_OK) return e.Fail("gz_get_coeffs", rc);
    if (memcmp(co.data(), e.sc_.img.data(), co.size() * sizeof(int16_t)) != 0) {
      fprintf(stderr, "guetzli_amd: the host mirror of the image differs from the device image after the search\n");
      return false;
    }
  }
  return true;
}

// Phase A on the device (ComputeBlockZeroingOrder of every block, :553-590) and the size model of the starting
// point (:592-604).
bool Encoder::MaskSearch::SearchBlocks(Stopwatch* sw) {
  std::vector<int32_t>& cand_off = e.sc_.cand_off;
  std::vector<uint8_t>& cand_idx = e.sc_.cand_idx;
  if (cand_off.size() != (size_t)nb + 1) cand_off.resize((size_t)nb + 1);
  if (cand_idx.size() != (size_t)nb * 189) cand_idx.resize((size_t)nb * 189);
  // the candidates' errors stay on the device, where the global order is built from them
  int rc = gz_block_zeroing_orders_masked(e.ctx_, comp_mask, e.params_.zeroing_greedy_lookahead,
                                          e.params_.new_zeroing_model ? 1 : 0, cand_off.data(),
                                          cand_idx.data(), nullptr, nb * 189);
  e.timer_[kTBlockSearch] += sw->lap();
  if (rc != GZ_OK) return e.Fail("gz_block_zeroing_orders", rc);
  {
    uint64_t ev = 0;
    if (gz_search_evaluations(e.ctx_, &ev) == GZ_OK) e.count_[kNEvaluations] += (long)ev;
  }
  // ---- size model of the starting point ----
  {
    if (!e.DeviceHistograms(e.quant_, dc_histo, ac_histo)) return false;
    Frame f;
    e.Tables(e.quant_, ChromaAllZero(dc_histo, ac_histo) ? 1 : 3, &f);
    header_size = (int)HeaderSize(f);
    SymbolHistogram dcs[3] = {dc_histo[0], dc_histo[1], dc_histo[2]};
    size_t num = f.ncomp;
    int indexes[3];
    uint8_t depths[3 * kHistoSize];
    dc_size = (int)ClusterHistograms(dcs, &num, indexes, depths);   // EstimateDCSize
    // BuildACHistograms fills one histogram per component SaveToJpegData wrote: with all-zero
    // chroma that is luma only, and the other entries of ac_histograms(ncomp) stay empty (:592-600)
    if (f.ncomp == 1) { ac_histo[1].Clear(); ac_histo[2].Clear(); }
  }
  ac_depths.assign(3 * kHistoSize, 0);
  ac_header = (int)EntropyCodes(ac_histo, ncomp, ac_depths.data());
  base_size = header_size + dc_size + ac_header + (int)EntropyDataSize(ac_histo, ncomp, ac_depths.data());
  prev_size = base_size;
  return true;
}

// The host mirror sc_.img follows the bulk ("fast") steps lazily: mirror_cand[b] says up to
// which candidate position block b's coefficients in the mirror are current.  Only the blocks the
// slow steps touch (a hundred per iteration) need their mirror at once.  What a block looks like
// is a function of how far it has advanced, not of the way there: its candidates are distinct
// coefficients, those below next_cand are zeroed (the precious ones excepted), those from next_cand
// on hold their quantised original values -- so a block catches up in whichever direction it lags,
// also across the turn from "up" to "down", and the rest of the image is brought up to date only
// when somebody reads all of it (GZ_VERIFY_ENTROPY, a second mask's search; on the worker pool):
// 7.5 M pending steps at the turn of a 4K encode, 3.4 ms with the device idle, for blocks most of
// which the serial steps never visit.
void Encoder::MaskSearch::SettleBlock(int b) {
  HostScratch& sc = e.sc_;
  int m = mirror_cand[b];
  const int n = next_cand[b];
  for (; m < n; ++m) {   // behind: the steps up
    const int idx = sc.cand_idx[sc.cand_off[b] + m];
    const int c = idx / 64, k = idx % 64;
    if (!IsPrecious(&sc.orig[e.Pos(c, b, 0)], k)) sc.img[e.Pos(c, b, k)] = 0;
  }
  for (; m > n; --m) {   // ahead: the steps down
    const int idx = sc.cand_idx[sc.cand_off[b] + m - 1];
    const int c = idx / 64, k = idx % 64;
    const int16_t* orig_blk = &sc.orig[e.Pos(c, b, 0)];
    const int newval = QuantizeCoeff(orig_blk[k], e.quant_[c][k]);
    if (!(newval == 0 && IsPrecious(orig_blk, k))) sc.img[e.Pos(c, b, k)] = (int16_t)newval;
  }
  mirror_cand[b] = n;
}

void Encoder::MaskSearch::SettleAll() {
  WorkerPool& pool = WorkerPool::Get();
  const int chunks = nb < 4096 ? 1 : 4 * pool.size();
  const int per = (nb + chunks - 1) / chunks;
  pool.Run(chunks, [&](int ch) {
    for (int b = ch * per; b < std::min(nb, (ch + 1) * per); ++b) SettleBlock(b);
  });
}

// `order` (global_order, processor.cc:622-663) is built on the device from the CSR arrays phase A left
// there, in the reference's sequence: blocks ascending; within a block the remaining candidates ascending
// for "up", the applied ones descending for "down".  The order of the next iteration is constructed on the
// device right behind the evaluation of this iteration's candidate (EvaluateCandidate): `ahead` says that
// such a construction is in flight, and for which direction.
bool Encoder::MaskSearch::AcquireOrder() {
  int rc = GZ_OK;
  for (int radius = 1; radius <= 4; ++radius) {
    // block weights (ComputeBlockErrorAdjustmentWeights) and max_block_error stay on the
    // device; the host only supplies how far each block has advanced
    int32_t btc = 0;
    if (radius == 1 && ahead == it.direction && !first_up) {
      rc = gz_order_build_auto_end(e.ctx_, &it.total, &btc, &it.below);
      if (rc == GZ_OK) {
        rc = gz_order_descend_end(e.ctx_, ahead_log, 12, &ahead_levels, &ahead_last);
        it.have_ahead_log = rc == GZ_OK && ahead_levels > 0;
      }
    } else {
      rc = gz_order_build_auto(e.ctx_, it.direction, radius, target_mul, first_up ? 0 : 1,
                               next_cand.data(), first_up ? 1 : 0, it.below_limit, &it.total, &btc,
                               &it.below);
    }
    ahead = 0;
    if (rc != GZ_OK) return e.Fail("gz_order_build_auto", rc);
    it.blocks_to_change = btc;
    if (it.total != 0) break;
    it.have_ahead_log = false;   // (an empty order: the next radius builds another one)
  }
  return true;
}

// Steps [0, fast_until) of the sorted order: the introsort partitions that lead there on the device, the
// prefix as a set, the steps applied block by block on the device image, their effect on the AC symbol
// statistics from the device.
bool Encoder::MaskSearch::BulkSteps(size_t fast_until) {
  const int direction = it.direction;
  const size_t n_order = it.n_order;
  const size_t device_threshold = e.knobs_.order_device_threshold;
  std::pair<int, float>* order = it.order;
  double* const t = e.timer_;
  int rc = GZ_OK;
  Stopwatch fw;
  // The introsort partitions that lead to position fast_until - 1, made by the device
  // without the host in between: behind the order's construction when that was enqueued
  // ahead (the device derives the position as the caller does), else now, in one call.
  if (n_order > device_threshold) {
    const uint64_t want = fast_until ? fast_until - 1 : 0;
    if (it.have_ahead_log) {
      if (ahead_last != want) return e.Fail("gz_order_descend: position", GZ_E_STATE);
      memcpy(dev_order->log, ahead_log, sizeof(uint64_t) * 3 * ahead_levels);
      dev_order->log_n = ahead_levels;
    } else {
      int levels = 0;
      rc = gz_order_descend(e.ctx_, want, device_threshold, e.descend_levels_, dev_order->log, &levels);
      if (rc != GZ_OK) return e.Fail("gz_order_descend", rc);
      dev_order->log_n = levels;
    }
    if (dev_order->log_n > 0) {
      // the range the descent ended in, and with it everything SelectPrefix will fetch
      uint64_t flo = 0, fhi = n_order;
      for (int l = 0; l < dev_order->log_n; ++l) {
        const uint64_t cut = dev_order->log[3 * l + 2];
        if (want < cut) fhi = cut; else flo = cut;
      }
      // (only when the descent got there: a range that is still large will be partitioned
      // further on the device, and a copy taken now would be stale)
      if (fhi - flo <= device_threshold && fhi <= ((size_t)1 << 19)) {
        // ... unless the device has put exactly that prefix into the mirror already, behind
        // the descent it made ahead (k_desc_export)
        uint64_t exported = 0;
        if (it.have_ahead_log) {
          rc = gz_order_exported(e.ctx_, &exported);
          if (rc != GZ_OK) return e.Fail("gz_order_exported", rc);
        }
        if (exported == fhi) {
          dev_order->have_hi = (size_t)fhi;
          ++e.count_[kNExported];
        } else if (!dev_order->Prefetch((size_t)fhi, order)) {
          return e.Fail("gz_order_fetch", dev_order->rc);
        }
      }
    }
    t[kTDescend] += fw.lap();
  }
  sorted->SelectPrefix(fast_until);   // the set [0, fast_until) and element fast_until - 1
  t[kTEnsure] += fw.lap();
  // Steps [0, fast_until): only how many steps each block takes matters (the n-th step
  // of a block applies its n-th remaining candidate whatever the key), so they are
  // applied block by block: on the device image by gz_apply_candidate_steps, on the
  // host mirror by the worker pool.
  {
    // first touches go to `dirty` without a branch (which block an entry belongs to is as
    // good as random: the branch mispredicted for a third of the 63 000 entries of a 4K
    // iteration)
    if (first_touch.size() != (size_t)nb + 1) first_touch.resize((size_t)nb + 1);
    int32_t* dl = first_touch.data();
    int* sc = step_count.data();
    char* tc = touched.data();
    WorkerPool& pool = WorkerPool::Get();
    const size_t parallel_from = e.knobs_.parallel_count_min;   // (the tests: this path on small images)
    if (fast_until >= parallel_from && pool.size() > 1) {
      // The first "up" iteration of an encode takes every candidate below the error limit at
      // once -- 7.5 M entries at 4K, 7.5 of this loop's 9 ms per encode: the entries in `parts`
      // ranges, a private count array per range (0.5 MB: it stays in the core's cache), summed
      // afterwards.  Which order the touched blocks are listed in matters to nobody (independent
      // blocks on the device, a set to be cleared here).
      const int parts = std::min(pool.size(), 8);
      std::vector<std::vector<int32_t> > part_count((size_t)parts);
      pool.Run(parts, [&](int p) {
        std::vector<int32_t>& cnt = part_count[(size_t)p];
        cnt.assign((size_t)nb, 0);
        const size_t i0 = fast_until * (size_t)p / parts, i1 = fast_until * (size_t)(p + 1) / parts;
        for (size_t i = i0; i < i1; ++i) ++cnt[(size_t)order[i].first];
      });
      size_t nd = 0;
      for (int b = 0; b < nb; ++b) {
        int n = 0;
        for (int p = 0; p < parts; ++p) n += part_count[(size_t)p][(size_t)b];
        if (n == 0) continue;
        if (sc[b] == 0) dl[nd++] = b;
        sc[b] += n;
        tc[b] = 1;
      }
      dirty.assign(dl, dl + nd);
    } else {
      size_t nd = 0;
      for (size_t i = 0; i < fast_until; ++i) {
        const int b = order[i].first;
        dl[nd] = b;
        nd += sc[b] == 0;
        ++sc[b];
        tc[b] = 1;
      }
      dirty.assign(dl, dl + nd);
    }
  }
  t[kTFastCount] += fw.lap();
  if (fast_until > 0) {
    it.val_threshold = order[fast_until - 1].second;
    it.changed_coeffs += (int)fast_until;
    // the device applies the same steps to its image (and advances its next_cand) ...
    std::vector<int32_t>& counts = e.bulk_counts_;
    counts.resize(dirty.size());
    for (size_t di = 0; di < dirty.size(); ++di) counts[di] = step_count[dirty[di]];
    rc = gz_apply_candidate_steps(e.ctx_, direction, dirty.data(), counts.data(), (int)dirty.size());
    if (rc != GZ_OK) return e.Fail("gz_apply_candidate_steps", rc);
    t[kTFastApply] += fw.lap();
    // ... while the host only notes how far each block has advanced; its mirror of the
    // coefficients follows when a slow step needs the block (SettleBlock)
    // (step_count holds exactly these counts and zeros elsewhere: with a fifth of the blocks
    // touched, one pass over the two arrays -- 20 us -- beats 26 000 scattered updates -- 40-120)
    if (dirty.size() * 16 > (size_t)nb) {
      int* nc = next_cand.data();
      const int* scp = step_count.data();
      for (int b = 0; b < nb; ++b) nc[b] += direction * scp[b];
    } else {
      for (size_t di = 0; di < dirty.size(); ++di) next_cand[dirty[di]] += direction * counts[di];
    }
    if (e.knobs_.verify()) SettleAll();   // GZ_VERIFY_ENTROPY compares the whole mirror
    // the symbol statistics of the edited image come from the device: the change the
    // steps made to BuildACHistograms, counted over the touched blocks (the host's
    // ac_histo was exact before them: the slow steps keep it so)
    t[kTFastMirror] += fw.lap();
    std::vector<int32_t> delta(3 * 256);
    rc = gz_steps_histogram_delta(e.ctx_, delta.data());
    t[kTFastDelta] += fw.lap();
    if (rc != GZ_OK) return e.Fail("gz_steps_histogram_delta", rc);
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 256; ++i)
        if (delta[c * 256 + i]) ac_histo[c].Add(i, delta[c * 256 + i]);
    if (e.knobs_.verify()) {   // GZ_VERIFY_ENTROPY=1: against a recount of the whole image
      SymbolHistogram dc_now[3], ac_now[3];
      if (!e.DeviceHistograms(e.quant_, dc_now, ac_now)) return false;
      for (int c = 0; c < ncomp; ++c)
        if (memcmp(ac_now[c].counts, ac_histo[c].counts, sizeof(ac_now[c].counts)) != 0) {
          fprintf(stderr, "guetzli_amd: incremental AC statistics differ from a recount\n");
          return false;
        }
    }
  }
  t[kTFastRest] += fw.lap();
  return true;
}

// A step touches one block out of 130 000 at random: its entry of the per-block arrays, its
// candidate list, its coefficient blocks in the original and in the image -- four dependent
// cache misses, which is what a step costs.  The steps to come are known (the sorted order),
// so their lines are asked for ahead, one dependency per stage.  (A block that advances in
// between makes a prefetch miss its mark by a candidate; nothing depends on these.)
inline void Encoder::MaskSearch::PrefetchFor(size_t i) {
  const HostScratch& sc = e.sc_;
  const size_t n_order = it.n_order;
  const int back = std::min(it.direction, 0);
  if (i + 12 < n_order) {
    const int b1 = (*sorted)[i + 12].first;
    __builtin_prefetch(&sc.cand_off[b1]);
    __builtin_prefetch(&next_cand[b1]);
    __builtin_prefetch(&mirror_cand[b1]);
    __builtin_prefetch(&touched[b1]);
  }
  if (i + 8 < n_order) {
    const int b2 = (*sorted)[i + 8].first;
    __builtin_prefetch(&sc.cand_idx[sc.cand_off[b2] + next_cand[b2] + back]);
  }
  if (i + 4 < n_order) {
    const int b3 = (*sorted)[i + 4].first;
    const int idx3 = sc.cand_idx[sc.cand_off[b3] + next_cand[b3] + back];
    const size_t p3 = e.Pos(idx3 / 64, b3, 0);
    __builtin_prefetch(&sc.orig[p3]);
    __builtin_prefetch(&sc.orig[p3 + 32]);
    __builtin_prefetch(&sc.img[p3], 1);
    __builtin_prefetch(&sc.img[p3 + 32], 1);
  }
}

// One step of the reference loop (processor.cc:704-750) without its size estimate: change one coefficient of
// block b (host mirror + edit list for the device), keep ac_histo current and leave in *st what pricing the
// step (PriceStep) or taking it back (UndoStep) needs.
inline void Encoder::MaskSearch::TakeStep(size_t i, SlowStep* st) {
  HostScratch& sc = e.sc_;
  const int direction = it.direction;
  const std::pair<int, float>& entry = (*sorted)[i];   // (operator[] sorts lazily)
  const int b = entry.first;
  SettleBlock(b);
  const int idx = sc.cand_idx[sc.cand_off[b] + next_cand[b] + std::min(direction, 0)];
  const int c = idx / 64, k = idx % 64;
  const int* q = e.quant_[c];
  const int16_t* orig_blk = &sc.orig[e.Pos(c, b, 0)];
  int16_t* blk = &sc.img[e.Pos(c, b, 0)];
  const int newval = direction > 0 ? 0 : QuantizeCoeff(orig_blk[k], q[k]);
  st->b = b;
  st->val = entry.second;
  st->comp = (uint8_t)c;
  st->changed = st->nsym = 0;
  st->pos = st->old_val = 0;
  if (!(newval == 0 && IsPrecious(orig_blk, k))) {
    st->changed = 1;
    st->pos = (int32_t)e.Pos(c, b, k);
    st->old_val = blk[k];
    // UpdateACHistogram before and after the change (processor.cc:715-722): only the symbols
    // around the coefficient differ (k == 0: a block's AC symbols do not depend on its DC coefficient)
    if (k >= 1) st->nsym = (uint8_t)CoeffACSymbolChanges(blk, q, k, newval, st->sym);
    for (int j = 0; j < st->nsym; ++j)
      ac_histo[c].Add(std::abs(st->sym[j]) - 1, st->sym[j] > 0 ? 1 : -1);
    blk[k] = (int16_t)newval;
    edit_pos.push_back(st->pos);
    edit_val.push_back((int16_t)newval);
  }
  next_cand[b] += direction;
  mirror_cand[b] = next_cand[b];
  st->first_touch = !touched[b];
  if (!touched[b]) {
    touched[b] = 1;
    dirty.push_back(b);
  }
}

// What the step's symbol changes do to HistogramRawBits under the current depths.
inline void Encoder::MaskSearch::PriceStep(const SlowStep& st) {
  const uint8_t* depth = &ac_depths[st.comp * kHistoSize];
  int64_t bits = 0;
  for (int j = 0; j < st.nsym; ++j) {
    const int symbol = std::abs(st.sym[j]) - 1;
    const int cost = depth[symbol] + (symbol & 0xf);
    bits += st.sym[j] > 0 ? cost : -cost;
  }
  ac_raw_bits[st.comp] += bits;
}

void Encoder::MaskSearch::UndoStep(const SlowStep& st) {   // (of the last step taken)
  const int b = st.b;
  if (st.first_touch) {
    touched[b] = 0;
    dirty.pop_back();
  }
  next_cand[b] -= it.direction;
  mirror_cand[b] = next_cand[b];
  if (st.changed) {
    edit_pos.pop_back();
    edit_val.pop_back();
    e.sc_.img[st.pos] = st.old_val;
    for (int j = 0; j < st.nsym; ++j)
      ac_histo[st.comp].Add(std::abs(st.sym[j]) - 1, st.sym[j] > 0 ? -1 : 1);
  }
}

// The reference's loop (processor.cc:704-750) over the steps [from, to): true = the stopping rule fired (at
// the last step taken).
bool Encoder::MaskSearch::StepsAsTheReference(size_t from, size_t to) {
  for (size_t i = from; i < to; ++i) {
    SlowStep st;
    TakeStep(i, &st);
    it.val_threshold = st.val;
    ++it.changed_coeffs;
    if (i % 10 == 0) {   // (the refresh counts the step's symbols with the others)
      Stopwatch cw;
      ac_header = (int)EntropyCodes(ac_histo, ncomp, ac_depths.data());
      RecountRawBits();
      e.timer_[kTCodes] += cw.lap();
    } else {
      PriceStep(st);
    }
    ++e.count_[kNSteps];
    it.est_size = EstimateSize();
    if (e.knobs_.verify() && DataBytes() != EntropyDataSize(ac_histo, ncomp, ac_depths.data())) {
      fprintf(stderr, "guetzli_amd: incremental size estimate differs from a recount\n");
      it.verify_failed = true;
      return true;
    }
    if (it.changed_coeffs > it.min_coeffs_to_change &&
        std::abs(it.est_size - prev_size) > it.min_size_delta)
      return true;
  }
  return false;
}

// The serial steps from `base` (a multiple of 10) on with their code refreshes on the helper threads
// (code_refresh.h).  Window w = the steps base + 10 w .. + 9; its first step is a refresh step.  This
// thread takes the steps of up to `lag + 1` windows before it prices the oldest of them:
// the statistics right after a window's first step go to a helper, the steps' symbol changes
// are kept, and when the window's codes are there every step gets the size estimate the
// reference computes for it -- raw bits of the statistics at the refresh under the new
// depths, then the steps' changes priced with those depths (PriceStep) -- and the stopping rule
// is applied in step order.  Steps taken beyond the one it fires at are undone, last first.
void Encoder::MaskSearch::StepsWithHelpers(size_t base) {
  const size_t n_order = it.n_order;
  CodeRefreshers& refreshers = *e.refreshers_;
  refreshers.Activate();
  std::vector<SlowStep>& slog = e.slow_log_;
  slog.clear();
  const long lag = refreshers.threads();
  const long w0 = refreshers.NextWindow();
  long applied_w = 0, priced_w = 0;
  size_t next_apply = base;
  bool stopped = false;
  size_t last_priced = base;   // the last step with an estimate (valid once a window is priced)
  for (;;) {
    if (next_apply < n_order && applied_w - priced_w <= lag) {
      // take the steps of the next window; the refresh of its first step goes out at once
      const size_t i0 = next_apply, i1 = std::min(i0 + 10, n_order);
      for (size_t i = i0; i < i1; ++i) {
        PrefetchFor(i);
        slog.emplace_back();
        TakeStep(i, &slog.back());
        if (i == i0) {
          CodeRefresh* in = refreshers.Input(w0 + applied_w);
          memcpy(in->histo, ac_histo, sizeof(in->histo));
          in->ncomp = ncomp;
          refreshers.Submit(w0 + applied_w);
        }
      }
      next_apply = i1;
      ++applied_w;
      continue;
    }
    if (priced_w == applied_w) break;   // every step of the order taken and priced
    Stopwatch cw;
    const CodeRefresh* r = refreshers.Wait(w0 + priced_w);
    e.timer_[kTCodes] += cw.lap();
    // (the helper writes the depths of the frame's components only)
    memcpy(ac_depths.data(), r->depths, std::min(ac_depths.size(), (size_t)ncomp * kHistoSize));
    ac_header = r->ac_header;
    for (int c = 0; c < 3; ++c) ac_raw_bits[c] = r->raw_bits[c];
    const size_t i0 = base + 10 * (size_t)priced_w, i1 = std::min(i0 + 10, n_order);
    for (size_t i = i0; i < i1; ++i) {
      // (the refresh step's own changes are in the statistics the codes were made for)
      if (i > i0) PriceStep(slog[i - base]);
      it.est_size = EstimateSize();
      last_priced = i;
      if ((int)i + 1 > it.min_coeffs_to_change &&
          std::abs(it.est_size - prev_size) > it.min_size_delta) {
        stopped = true;
        break;
      }
    }
    ++priced_w;
    if (stopped) break;
  }
  // the steps beyond the last one the reference takes, last first; then the refreshes that
  // were asked for on their behalf (a slot is handed out again only after its window is done)
  const size_t keep = last_priced + 1;   // steps [base, keep) stay
  for (size_t i = next_apply; i > keep; --i) UndoStep(slog[i - 1 - base]);
  e.count_[kNUndone] += (long)(next_apply - keep);
  for (long w = priced_w; w < applied_w; ++w) (void)refreshers.Wait(w0 + w);
  it.changed_coeffs += (int)(keep - base);
  it.val_threshold = slog[keep - 1 - base].val;
  e.count_[kNSteps] += (long)(keep - base);
}

// The iteration's candidate: its changed coefficients to the device image, the evaluation enqueued with the
// next iteration's order behind it, the exact size where it is observable (processor.cc:752-772).
bool Encoder::MaskSearch::EvaluateCandidate(Stopwatch* sw) {
  const int direction = it.direction;
  // push the changed coefficients to the device image (positions are distinct: a block's
  // candidates are distinct coefficients and a block advances in one direction)
  int rc = gz_apply_coeff_edits(e.ctx_, edit_pos.data(), edit_val.data(), (int)edit_pos.size());
  e.timer_[kTUpload] += sw->lap();
  if (rc != GZ_OK) return e.Fail("gz_apply_coeff_edits", rc);

  size_t jpg_size = 0;
  if (!e.CompareBegin()) return false;
  // The candidate's exact size is observable in two places only: the --verbose trace
  // (Out[...], EstErr[...]) and MaybeOutput's comparison of scores (processor.cc:139-148,767).
  // Its head and the exact length of its scan in bits follow from the symbol statistics the
  // host holds anyway (PrepareHead); only the bytes stuffed behind 0xFF need the coder.  Without
  // a trace the candidate is therefore entropy-coded only if it can win: ScoreJPEG grows with
  // the size, so a candidate whose score at its size's LOWER bound does not beat the best so
  // far loses whatever it weighs -- 140 of the 149 candidates of a 4K encode at quality 95,
  // whose evaluation then has the device to itself (the coder's kernels took a sixth of the
  // summed kernel time, profiles/r03_bench_kernel_stats.csv).
  // GZ_VERIFY_ENTROPY=2 checks the DEFAULT path: the bound decision is taken first and the
  // candidate is coded regardless, late (behind the evaluation, as a winner is) -- the bound must
  // not exceed the coded size, and a candidate the bound rejects must lose with its real size too
  // (with =1 / --verbose every candidate takes the early-scan path instead).
  const bool trace = e.stats_->debug_output || e.stats_->debug_output_file;
  const bool verify_late = e.knobs_.verify_level >= 2 && !trace;
  const bool every_size = (trace || e.knobs_.verify()) && !verify_late;
  // the entropy coder goes to its own stream before anything else is enqueued: it runs beside
  // the evaluation, not behind the host work below.  Without it the head is built (15 us of Huffman codes) AFTER
  // the next order's launches: up to 1080p the device finishes an evaluation before the host has enqueued what
  // follows it, and whatever the host does in between is time the device idles.
  if (every_size && (!e.PrepareHead(e.quant_, dc_histo, ac_histo) || !e.ScanBegin())) return false;
  Stopwatch aw;
  {
    // the next iteration of this direction, radius 1, if it comes to that (processor.cc:
    // 622-663 behind :767): everything it reads is final -- next_cand, max_block_error
    // (gz_order_advance in the caller), and the distance map the device is about to produce -- with the
    // descent behind it, and everything the host waits for at this point (the order's size and
    // counters, the descent's cuts, the candidate's distance) in one transfer
    rc = gz_order_build_auto_descend_begin(e.ctx_, direction, 1, target_mul, 1, next_cand.data(), 0,
                                           it.below_limit, it.per_block, e.knobs_.order_device_threshold,
                                           e.descend_levels_);
    if (rc != GZ_OK) return e.Fail("gz_order_build_auto_descend_begin", rc);
    ahead = direction;
  }
  e.timer_[kTAheadBegin] += aw.lap();
  if (!every_size && !e.PrepareHead(e.quant_, dc_histo, ac_histo)) return false;
  if (every_size) {
    if (!e.SerializeEnd(e.quant_, &jpg_size)) return false;
    e.Log("Iter %2d: %s(%d) %s Coeffs[%d/%zd] Blocks[%zd/%d/%d] ValThres[%.4f] Out[%7zd] "
          "EstErr[%.2f%%]",
          e.stats_->counters[kNumItersCnt], e.FrameStr(), comp_mask, direction > 0 ? "up" : "down",
          it.changed_coeffs, it.n_order, dirty.size(), it.blocks_to_change, nb, it.val_threshold,
          jpg_size, 100.0 - (100.0 * it.est_size) / jpg_size);
    if (!e.CompareCurrent()) return false;
    if (!e.MaybeOutput(jpg_size)) return false;
  } else {
    if (!e.CompareCurrent()) return false;
    const bool may_win = e.best_score_ < 0 ||
        ScoreJPEG(e.distance_, (int)e.SizeLowerBound(), e.params_.butteraugli_target) < e.best_score_;
    if (may_win) {
      if (!e.ScanBegin() || !e.SerializeEnd(e.quant_, &jpg_size) || !e.MaybeOutput(jpg_size)) return false;
    } else {
      if (verify_late) {
        if (!e.ScanBegin() || !e.SerializeEnd(e.quant_, &jpg_size)) return false;   // (checks bound <= size itself)
        if (ScoreJPEG(e.distance_, (int)jpg_size, e.params_.butteraugli_target) < e.best_score_) {
          fprintf(stderr, "guetzli_amd: a candidate rejected on its size bound would have won\n");
          return false;
        }
      }
      ++e.count_[kNScansSkipped];
    }
  }
  return true;
}

}  // namespace guetzli_amd
