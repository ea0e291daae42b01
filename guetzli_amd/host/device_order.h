// Phase B's global candidate order where it lives -- on the device -- as LazySorted's back end (lazy_sort.h).
#pragma once
#include "encoder.h"

namespace guetzli_amd {

// The device-resident global candidate order as LazySorted's back end.
struct DeviceOrder : RangeDevice {
  DeviceOrder(gz_ctx* c, double* timers, long* counts) : ctx(c), t(timers), n(counts) {}
  // Partitions the device has already made on its own (gz_order_descend*: the quick-select
  // descent towards the position phase B needs, enqueued behind the order's construction), in
  // the order LazySorted is going to ask for them: (lo, hi, cut) triples.
  uint64_t log[3 * 12];
  int log_n = 0, log_next = 0;
  bool Partition(size_t lo, size_t hi, size_t* cut) override {
    if (log_next < log_n && log[3 * log_next] == lo && log[3 * log_next + 1] == hi) {
      *cut = (size_t)log[3 * log_next + 2];
      ++log_next;
      ++n[kNReplayed];
      return true;
    }
    if (log_next < log_n) {   // the device went another way than the host: its array is not what we think
      rc = GZ_E_STATE;
      return false;
    }
    Stopwatch w;
    uint64_t c64 = 0;
    rc = gz_order_partition(ctx, lo, hi, &c64);
    *cut = (size_t)c64;
    t[kTDevPartition] += w.lap();
    ++n[kNPartitions];
    ++n_partition;
    return rc == GZ_OK;
  }
  // After a descent everything below the end of the range that holds the wanted position is
  // going to be fetched, range by range; one copy brings it all (to where Fetch would put it).
  bool Prefetch(size_t hi, void* base) {
    Stopwatch w;
    rc = gz_order_fetch(ctx, 0, hi, base);
    t[kTDevFetch] += w.lap();
    n[kNFetched] += (long)hi;
    if (rc == GZ_OK) have_hi = hi;
    return rc == GZ_OK;
  }
  size_t have_hi = 0;   // entries [0, have_hi) are on the host already
  bool Fetch(size_t lo, size_t hi, void* dst) override {
    if (hi <= have_hi) return true;
    Stopwatch w;
    rc = gz_order_fetch(ctx, lo, hi, dst);
    t[kTDevFetch] += w.lap();
    n[kNFetched] += (long)(hi - lo);
    return rc == GZ_OK;
  }
  gz_ctx* ctx;
  double* t;   // the encoder's timers and counters (encoder.h)
  long* n;
  int rc = GZ_OK;
  int n_partition = 0;   // partitions this order asked the device for
};

}  // namespace guetzli_amd
