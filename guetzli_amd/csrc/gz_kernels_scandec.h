// A baseline JPEG scan read on the device: the self-synchronising parallel Huffman decode (Klein & Wiseman; Weissenberger &
// Schmidt, ICPP 2018) on JPEG's block structure -- the mirror image of gz_kernels_entropy.h, which writes such a scan.
//
// The scan's raw bytes [0, end) -- byte stuffing included; `end` is where the host's BitReader stops handing out data:
// the first 0xff that no 0x00 follows, or two bytes before the end of the file -- are cut into subsequences of
// subseq_bytes bytes, one lane each.  A lane owns the symbols (a Huffman code and the extra bits behind it) whose first
// bit lies in its subsequence.  Its state at a boundary is the triple
//   p  the raw bit offset of the first symbol that starts in the subsequence (never inside a stuffed 0x00),
//   u  the unit within the MCU (which selects the component and so the tables),
//   k  the zig-zag position (0: a DC symbol comes next),
// in one 64-bit word: p | (u << 8 | k) << 32.
//
//   1. k_scandec_sync_first   every lane decodes from the blind state (its first bit, u = 0, k = 0), then lane i takes
//                             lane i-1's exit state as its entry state until nothing changes in the workgroup: at most
//                             256 rounds behind barriers, lane 0 never changes.
//      k_scandec_sync_next    the same from the exit state of the workgroup before, as the launch BEFORE left it (two
//                             boundary arrays, written and read in turns: no workgroup reads what another one writes
//                             in the same launch); a boundary that changed sets the round's word, which the host reads.
//   2. k_scan_offsets         (gz_kernels_entropy.h) exclusive prefix sums of the lanes' block counts.
//   3. k_scandec_write        every lane decodes once more, knowing its first block: AC values times their quantiser into
//                             the frame layout (blocks inside the image's grid only), DC differences into an array over
//                             all blocks in scan order; the first error in scan order by atomicMin on block << 3 | reason.
//   4. k_scandec_dc           per component the running sum of the differences, its range checks, coefficient 0.
//
// Passes 3 and 4 have a second store mode, INPUT (k_scandec_write_input, k_scandec_dc_input): what the host READER leaves
// in JpegComponentIn::coeffs -- the values QUANTISED, as coded, on grids padded to whole MCUs, every block of the scan
// stored (scandec_input_block_at) -- and CheckJpegSanity's verdict over them in res[2]: a word that is set where
// |value * quantiser| > 4096 for any stored coefficient, the padding's included.
//
// Every loop is bounded by a launch-time quantity: a lane decodes at most 8 * subseq_bytes symbols (each takes a bit or
// more and starts inside the subsequence), a workgroup settles in at most 256 rounds, the DC pass walks
// ceil(blocks / 256) blocks per thread.  Nothing waits for another workgroup inside a launch.  Reads of the stream are
// bounded by `end`, stores by the block count: a block index below `total` is the only thing an address depends on.
//
// While synchronising a lane may be decoding garbage from a wrong offset: a code that does not exist, a run past
// position 63, a DC category above 11 restart the block (k = 0) one bit further on.  The write pass refuses them.
#pragma once
#include <string.h>

#include "gz_common.h"
#include "gz_kernels_entropy.h"

namespace gz {

constexpr int kScanDecLanes = 256;
constexpr int kScanDecTables = 6;   // DC of component 0..2, AC of component 0..2

enum { kScanErrBadSymbol = 1, kScanErrRunPastBand = 2, kScanErrDcRange = 3, kScanErrCoeffRange = 4, kScanErrEndsEarly = 5 };

// The code tables as the host reader's HuffTable keeps them (T.81 C.2, F.2.2.3), and the quantisers in natural order.
struct ScanDecTables {
  uint16_t fast[kScanDecTables][512];   // ((length << 8) | symbol) + 1 for codes of <= 9 bits, 0 otherwise
  int maxcode[kScanDecTables][18];
  int mincode[kScanDecTables][17];
  int valptr[kScanDecTables][17];
  int num_values[kScanDecTables];
  uint8_t values[kScanDecTables][256];
  int quant[3][64];
};

struct ScanDecGeom {
  int units;            // blocks per MCU: 1 (one component), 3 (4:4:4), 6 (4:2:0: Y Y Y Y Cb Cr)
  int mcu_cols;
  int total;            // blocks of the scan: MCUs * units, the padding included
  int bw, bh, cbw, cbh; // the grids inside the image: component 0, components 1 and 2
  unsigned end_bits;    // 8 * end
  int subseq_bytes;
  int nsub;             // lanes
};

struct ScanDecState {
  unsigned long long* entry;   // [nsub]
  unsigned long long* exit;    // [nsub]
  unsigned* count;             // [nsub] blocks whose last symbol starts in the subsequence
};

GZ_DEVFN int scandec_comp(int units, int u) { return units == 6 ? (u < 4 ? 0 : u - 3) : u; }
GZ_DEVFN unsigned long long scandec_pack(unsigned p, int u, int k) { return (unsigned long long)p | ((unsigned long long)((u << 8) | k) << 32); }

// 32 bits of the stream from raw bit p on (first bit in bit 31), and the raw index of the byte each of the next five
// stream bytes comes from: behind 0xff its stuffed 0x00 is skipped, from `end` on the stream is zeros.
GZ_DEVFN unsigned scandec_peek(const uint8_t* __restrict__ data, unsigned end, unsigned p, unsigned idx[5]) {
  unsigned r = p >> 3;
  unsigned long long acc = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    idx[j] = r;
    unsigned b = 0;
    if (r < end) {
      b = data[r];
      r += b == 0xffu ? 2u : 1u;
    } else {
      r += 1u;
    }
    acc = (acc << 8) | b;
  }
  return (unsigned)((acc << (p & 7u)) >> 8);
}
// p behind n <= 27 bits.
GZ_DEVFN unsigned scandec_advance(unsigned p, int n, const unsigned idx[5]) {
  const unsigned vb = (p & 7u) + (unsigned)n, j = vb >> 3;
  unsigned at = idx[0];   // (selected, not indexed: the five indices stay in registers)
#pragma unroll
  for (unsigned i = 1; i < 5; ++i) at = j == i ? idx[i] : at;
  return at * 8u + (vb & 7u);
}
// The first bit a lane owns: its first byte, or the one behind it where that byte is a stuffed 0x00.
GZ_DEVFN unsigned scandec_first_bit(const uint8_t* __restrict__ data, unsigned end, unsigned byte) {
  if (byte > 0 && byte < end && data[byte] == 0 && data[byte - 1] == 0xffu) ++byte;
  return byte * 8u;
}

GZ_DEVFN int scandec_extend(int v, int nbits) { return v < (1 << (nbits - 1)) ? v - (1 << nbits) + 1 : v; }

// One symbol at the head of `w` in state (u, k): its bits (code and extra bits), its value and the zig-zag position the
// value belongs to (0: a DC difference, -1: none), whether it ends the block; the state moves on.  A return other than 0
// is what the host reader refuses the block for; the state is then untouched.
struct ScanDecSymbol { int bits, value, pos; bool done; };
GZ_DEVFN int scandec_symbol(const uint16_t (*fast)[512], const ScanDecTables* __restrict__ T, int units, unsigned w, int* u, int* k,
                            ScanDecSymbol* s) {
  const int tbl = (*k == 0 ? 0 : 3) + scandec_comp(units, *u);
  const unsigned f = fast[tbl][w >> 23];
  int len, sym;
  if (f) {
    len = (int)((f - 1) >> 8);
    sym = (int)((f - 1) & 0xff);
  } else {   // codes longer than 9 bits: extend bit by bit (F.2.2.3), as the host's DecodeSymbol does
    len = 9;
    int code = (int)(w >> 23);
    while (len <= 16 && (T->maxcode[tbl][len] < 0 || code > T->maxcode[tbl][len] || code < T->mincode[tbl][len])) {
      ++len;
      code = (int)(w >> (32 - len));
    }
    if (len > 16) return kScanErrBadSymbol;
    const int i = T->valptr[tbl][len] + code - T->mincode[tbl][len];
    if (i < 0 || i >= T->num_values[tbl]) return kScanErrBadSymbol;
    sym = T->values[tbl][i];
  }
  s->done = false;
  s->value = 0;
  s->pos = -1;
  s->bits = len;
  if (*k == 0) {
    if (sym > 11) return kScanErrBadSymbol;
    if (sym) s->value = scandec_extend((int)((w << len) >> (32 - sym)), sym);
    s->bits = len + sym;
    s->pos = 0;
    *k = 1;
    return 0;
  }
  const int r = sym >> 4, sz = sym & 15;
  if (sz) {
    const int at = *k + r;
    if (at > 63) return kScanErrRunPastBand;
    if (sz >= 12) return kScanErrCoeffRange;   // (the host's "AC coefficient out of range")
    s->value = scandec_extend((int)((w << len) >> (32 - sz)), sz);
    s->bits = len + sz;
    s->pos = at;
    *k = at + 1;
  } else if (r == 15) {
    *k += 16;
  } else if (r == 0) {
    *k = 64;
  } else {
    return kScanErrBadSymbol;   // an end-of-band run in a scan that carries DC
  }
  if (*k >= 64) {
    s->done = true;
    *k = 0;
    *u = *u + 1 == units ? 0 : *u + 1;
  }
  return 0;
}

// A lane's subsequence from state (p, u, k) to the first symbol that starts behind it: the synchronising decode.
GZ_DEVFN void scandec_run(const uint8_t* __restrict__ data, const uint16_t (*fast)[512], const ScanDecTables* __restrict__ T,
                          const ScanDecGeom& g, unsigned lane_end, unsigned long long in, unsigned long long* out, unsigned* blocks) {
  unsigned p = (unsigned)in;
  int u = (int)(in >> 40) & 0xff, k = (int)(in >> 32) & 0xff;
  const unsigned end = g.end_bits >> 3;
  unsigned n = 0;
  for (int it = 0; it < 8 * g.subseq_bytes && p < lane_end; ++it) {
    unsigned idx[5];
    const unsigned w = scandec_peek(data, end, p, idx);
    ScanDecSymbol s;
    if (scandec_symbol(fast, T, g.units, w, &u, &k, &s) != 0) {
      k = 0;   // garbage, or a stream the write pass will refuse: the block starts over one bit further on
      s.bits = 1;
      s.done = false;
    }
    p = scandec_advance(p, s.bits, idx);
    n += s.done ? 1u : 0u;
  }
  *out = scandec_pack(p, u, k);
  *blocks = n;
}

GZ_DEVFN void scandec_load_fast(uint16_t (*fast)[512], const ScanDecTables* __restrict__ T) {
  for (int i = threadIdx.x; i < kScanDecTables * 512; i += kScanDecLanes) fast[i >> 9][i & 511] = T->fast[i >> 9][i & 511];
}

// Passes 1a / 1b.  FIRST: blind start, no boundary read; otherwise lane 0 of workgroup b > 0 enters with bnd_in[b - 1].
// wg: the workgroup's index within its stream -- blockIdx.x of a launch over one stream; the state and the boundary
// arrays are the stream's own (element 0 is its lane 0, its workgroup 0).
template <bool FIRST>
GZ_DEVFN void scandec_sync_body(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T, const ScanDecGeom& g,
                                const ScanDecState& st, const unsigned long long* __restrict__ bnd_in,
                                unsigned long long* __restrict__ bnd_out, unsigned* __restrict__ changed, int wg) {
  __shared__ uint16_t s_fast[kScanDecTables][512];
  __shared__ unsigned long long s_exit[kScanDecLanes];
  __shared__ int s_flag[2];
  const int t = threadIdx.x;
  const int lane = wg * kScanDecLanes + t;
  const bool active = lane < g.nsub;
  scandec_load_fast(s_fast, T);
  if (t == 0) s_flag[0] = s_flag[1] = 0;
  __syncthreads();
  const unsigned end = g.end_bits >> 3;
  unsigned lane_end = 0;
  unsigned long long my_in = 0, my_out = 0, was_out = 0;
  unsigned cnt = 0;
  bool dirty = false;
  if (active) {
    const unsigned long long e = ((unsigned long long)lane + 1) * (unsigned long long)g.subseq_bytes * 8ull;
    lane_end = e < g.end_bits ? (unsigned)e : g.end_bits;
    if (FIRST) {
      my_in = scandec_pack(scandec_first_bit(data, end, (unsigned)lane * (unsigned)g.subseq_bytes), 0, 0);
      scandec_run(data, s_fast, T, g, lane_end, my_in, &my_out, &cnt);
      dirty = true;
    } else {
      my_in = st.entry[lane];
      my_out = st.exit[lane];
      cnt = st.count[lane];
    }
    was_out = my_out;
  }
  s_exit[t] = my_out;
  __syncthreads();
  for (int r = 0; r < kScanDecLanes; ++r) {
    unsigned long long in = my_in;
    if (t > 0) in = s_exit[t - 1];
    else if (!FIRST && wg > 0) in = bnd_in[wg - 1];
    __syncthreads();   // every lane has read its neighbour's exit state, and last round's flag
    if (t == 0) s_flag[(r + 1) & 1] = 0;
    if (active && in != my_in) {
      my_in = in;
      unsigned long long o;
      scandec_run(data, s_fast, T, g, lane_end, my_in, &o, &cnt);
      dirty = true;
      if (o != my_out) {
        my_out = o;
        s_exit[t] = o;
        s_flag[r & 1] = 1;
      }
    }
    __syncthreads();
    if (!s_flag[r & 1]) break;
  }
  if (!active) return;
  if (dirty) {
    st.entry[lane] = my_in;
    st.exit[lane] = my_out;
    st.count[lane] = cnt;
  }
  if (t == kScanDecLanes - 1 || lane == g.nsub - 1) {
    bnd_out[wg] = my_out;
    if (!FIRST && my_out != was_out) atomicOr(changed, 1u);
  }
}

__global__ __launch_bounds__(256) void k_scandec_sync_first(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T,
                                                            ScanDecGeom g, ScanDecState st, unsigned long long* __restrict__ bnd_out) {
  scandec_sync_body<true>(data, T, g, st, nullptr, bnd_out, nullptr, (int)blockIdx.x);
}
__global__ __launch_bounds__(256) void k_scandec_sync_next(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T,
                                                           ScanDecGeom g, ScanDecState st, const unsigned long long* __restrict__ bnd_in,
                                                           unsigned long long* __restrict__ bnd_out, unsigned* __restrict__ changed) {
  scandec_sync_body<false>(data, T, g, st, bnd_in, bnd_out, changed, (int)blockIdx.x);
}

// Where block b of the scan goes: its component, and its first coefficient in the frame layout or -1 (MCU padding).
GZ_DEVFN long long scandec_block_at(const ScanDecGeom& g, int b, int* comp) {
  const int mcu = b / g.units, u = b - mcu * g.units;
  const int my = mcu / g.mcu_cols, mx = mcu - my * g.mcu_cols;
  const int c = scandec_comp(g.units, u);
  *comp = c;
  int x = mx, y = my;
  if (g.units == 6 && c == 0) {
    x = 2 * mx + (u & 1);
    y = 2 * my + (u >> 1);
  }
  const int rw = c == 0 ? g.bw : g.cbw, rh = c == 0 ? g.bh : g.cbh;
  if (x >= rw || y >= rh) return -1;
  const long long first = c == 0 ? 0 : (long long)g.bw * g.bh + (long long)(c - 1) * g.cbw * g.cbh;
  return (first + (long long)y * rw + x) * 64;
}

// The same in the reader's own layout: the components one after the other, each [height_in_blocks][width_in_blocks][64]
// on its grid padded to whole MCUs -- of a 4:2:0 scan 2 mcu_cols x 2 mcu_rows for component 0, mcu_cols x mcu_rows
// otherwise.  Every block b < total has an address below total * 64.
GZ_DEVFN long long scandec_input_block_at(const ScanDecGeom& g, int b, int* comp) {
  const int mcu = b / g.units, u = b - mcu * g.units;
  const int my = mcu / g.mcu_cols, mx = mcu - my * g.mcu_cols;
  const int c = scandec_comp(g.units, u);
  *comp = c;
  const long long mcus = g.total / g.units;
  if (g.units == 6 && c == 0) return ((long long)(2 * my + (u >> 1)) * (2 * g.mcu_cols) + 2 * mx + (u & 1)) * 64;
  const long long first = g.units == 6 ? (3 + c) * mcus : c * mcus;
  return (first + mcu) * 64;
}
template <bool INPUT>
GZ_DEVFN long long scandec_store_at(const ScanDecGeom& g, int b, int* comp) {
  return INPUT ? scandec_input_block_at(g, b, comp) : scandec_block_at(g, b, comp);
}
// CheckJpegSanity's condition on one stored value (the product in 32 bits: |v| < 2^15, q < 2^16).
GZ_DEVFN bool scandec_large(int v, int q) {
  const int p = v * q;
  return (p < 0 ? -p : p) > (1 << 12);
}

GZ_DEVFN void scandec_fail(unsigned* res, int b, int reason) { atomicMin(&res[0], ((unsigned)b << 3) | (unsigned)reason); }

__constant__ unsigned char kScanDecNatural[64] = {
  0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

// Pass 3.  res[0]: the first error (block << 3 | reason, 0xffffffff: none), res[1]: the bit behind the last block's last
// symbol (0xffffffff: the scan never got there), INPUT: res[2] the large-coefficient word (zero when the kernel starts).
// coeffs and dcd are zero when the kernel starts.  wg as in scandec_sync_body; off[lane] - off_base is the lane's first
// block (off_base: what the prefix sums hold at the stream's lane 0 -- 0 where they cover one stream).
template <bool INPUT>
GZ_DEVFN void scandec_write_body(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T, const ScanDecGeom& g,
                                 const unsigned long long* __restrict__ entry, const unsigned long long* __restrict__ off,
                                 int16_t* __restrict__ coeffs, int16_t* __restrict__ dcd, unsigned* __restrict__ res, int wg,
                                 unsigned long long off_base) {
  __shared__ uint16_t s_fast[kScanDecTables][512];
  scandec_load_fast(s_fast, T);
  __syncthreads();
  const int lane = wg * kScanDecLanes + (int)threadIdx.x;
  if (lane >= g.nsub) return;
  const unsigned long long first = off[lane] - off_base;
  if (first >= (unsigned long long)g.total) return;
  int b = (int)first;
  const unsigned long long in = entry[lane];
  unsigned p = (unsigned)in;
  int k = (int)(in >> 32) & 0xff;
  if (k > 63) return;                  // (no state the passes before leave)
  int u = b % g.units;                 // (the state's own u, for a stream the host accepts)
  const unsigned long long e = ((unsigned long long)lane + 1) * (unsigned long long)g.subseq_bytes * 8ull;
  const unsigned lane_end = e < g.end_bits ? (unsigned)e : g.end_bits;
  const unsigned end = g.end_bits >> 3;
  int comp = 0;
  long long at = scandec_store_at<INPUT>(g, b, &comp);
  for (int it = 0; it < 8 * g.subseq_bytes && p < lane_end; ++it) {
    unsigned idx[5];
    const unsigned w = scandec_peek(data, end, p, idx);
    ScanDecSymbol s;
    const int bad = scandec_symbol(s_fast, T, g.units, w, &u, &k, &s);
    if (bad) { scandec_fail(res, b, bad); return; }
    p = scandec_advance(p, s.bits, idx);
    if (p > g.end_bits) { scandec_fail(res, b, kScanErrEndsEarly); return; }   // a bit the stream does not have
    if (s.pos == 0) {
      dcd[b] = (int16_t)s.value;
    } else if (s.pos > 0 && at >= 0) {
      const int nat = kScanDecNatural[s.pos];
      if (INPUT) {   // as coded (|value| <= 2047: an int16), and CheckJpegSanity where it is stored
        if (scandec_large(s.value, T->quant[comp][nat])) atomicOr(&res[2], 1u);
        coeffs[at + nat] = (int16_t)s.value;
      } else {
        const int v = s.value * T->quant[comp][nat];
        if (v != (int)(int16_t)v) { scandec_fail(res, b, kScanErrCoeffRange); return; }
        coeffs[at + nat] = (int16_t)v;
      }
    }
    if (s.done) {
      if (++b == g.total) { res[1] = p; return; }
      at = scandec_store_at<INPUT>(g, b, &comp);
    }
  }
}

__global__ __launch_bounds__(256) void k_scandec_write(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T, ScanDecGeom g,
                                                       const unsigned long long* __restrict__ entry,
                                                       const unsigned long long* __restrict__ off, int16_t* __restrict__ coeffs,
                                                       int16_t* __restrict__ dcd, unsigned* __restrict__ res) {
  scandec_write_body<false>(data, T, g, entry, off, coeffs, dcd, res, (int)blockIdx.x, 0ull);
}
__global__ __launch_bounds__(256) void k_scandec_write_input(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T,
                                                             ScanDecGeom g, const unsigned long long* __restrict__ entry,
                                                             const unsigned long long* __restrict__ off, int16_t* __restrict__ coeffs,
                                                             int16_t* __restrict__ dcd, unsigned* __restrict__ res) {
  scandec_write_body<true>(data, T, g, entry, off, coeffs, dcd, res, (int)blockIdx.x, 0ull);
}

// Pass 4: one workgroup per component; a thread sums a run of ceil(n / 256) of the component's blocks in scan order.
// INPUT: the sum itself is stored, of every block, and checked as CheckJpegSanity checks it.
template <bool INPUT>
GZ_DEVFN void scandec_dc_body(const int16_t* __restrict__ dcd, const ScanDecTables* __restrict__ T, const ScanDecGeom& g,
                              int16_t* __restrict__ coeffs, unsigned* __restrict__ res) {
  __shared__ long long s_sum[kScanDecLanes];   // (2^21 blocks of +-2047 leave 32 bits)
  const int t = threadIdx.x, c = (int)blockIdx.x;
  const int per = g.units == 6 && c == 0 ? 4 : 1;           // the component's blocks in an MCU
  const int ubase = g.units == 6 && c > 0 ? 3 + c : c;      // ... and the first of them
  const int n = g.total / g.units * per;
  const int chunk = (n + kScanDecLanes - 1) / kScanDecLanes;
  const int j0 = t * chunk < n ? t * chunk : n, j1 = j0 + chunk < n ? j0 + chunk : n;
  long long sum = 0;
  for (int j = j0; j < j1; ++j) sum += dcd[(j / per) * g.units + ubase + j % per];
  s_sum[t] = sum;
  __syncthreads();
  for (int d = 1; d < kScanDecLanes; d <<= 1) {   // inclusive sums over the threads
    const long long add = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  long long run = s_sum[t] - sum;
  const int q = T->quant[c][0];
  for (int j = j0; j < j1; ++j) {
    const int b = (j / per) * g.units + ubase + j % per;
    run += dcd[b];
    if (run != (long long)(int16_t)run) { scandec_fail(res, b, kScanErrDcRange); return; }
    int comp;
    const long long at = scandec_store_at<INPUT>(g, b, &comp);
    if (at < 0) continue;
    if (INPUT) {
      if (scandec_large((int)run, q)) atomicOr(&res[2], 1u);
      coeffs[at] = (int16_t)run;
    } else {
      const int v = (int)run * q;
      if (v != (int)(int16_t)v) { scandec_fail(res, b, kScanErrCoeffRange); return; }
      coeffs[at] = (int16_t)v;
    }
  }
}
__global__ __launch_bounds__(256) void k_scandec_dc(const int16_t* __restrict__ dcd, const ScanDecTables* __restrict__ T, ScanDecGeom g,
                                                    int16_t* __restrict__ coeffs, unsigned* __restrict__ res) {
  scandec_dc_body<false>(dcd, T, g, coeffs, res);
}
__global__ __launch_bounds__(256) void k_scandec_dc_input(const int16_t* __restrict__ dcd, const ScanDecTables* __restrict__ T, ScanDecGeom g,
                                                          int16_t* __restrict__ coeffs, unsigned* __restrict__ res) {
  scandec_dc_body<true>(dcd, T, g, coeffs, res);
}

// ------------------------------------------------------------------------------------------------ batches ----
// N streams of one frame size through ONE launch of each pass (gz_decode_scan_batch_device, api/entry_scandec_batch.h).
// The streams lie in one buffer, each at a 16-byte aligned offset; stream i has its own tables T[i] and its descriptor:
// its geometry (end_bits and nsub its own; bit offsets stay relative to its own first byte, 32 bits), and where its
// parts begin in the arrays the streams share.  Every stream's lanes are padded to whole workgroups, so a workgroup
// belongs to ONE stream -- wg_image[blockIdx.x] -- and its LDS tables are that stream's; entry, exit, count and the
// prefix sums span the padded lanes, of which the padding is inactive and counts 0 blocks (count is zero when the
// first kernel starts).  The bodies are the single stream's, on pointers moved to the stream's first lane, workgroup
// and block: no lane of one stream reads or writes a word of another's, and lane 0 of a stream's first workgroup has
// no workgroup before it, whatever lies in front of it in the arrays.
struct ScanDecImage {
  ScanDecGeom g;
  unsigned long long data_at;    // its first byte in the streams' buffer
  unsigned long long coeff_at;   // its coefficient arena (frame layout), in int16 from the arenas' base
  int wg0;                       // its first workgroup
  int lane0;                     // its first lane in the padded lane space: wg0 * kScanDecLanes
  int block0;                    // its first block in the DC differences
  int nwg;                       // its workgroups
};

__global__ __launch_bounds__(256) void k_scandec_sync_first_batch(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T,
                                                                  const ScanDecImage* __restrict__ images, const int* __restrict__ wg_image,
                                                                  ScanDecState st, unsigned long long* __restrict__ bnd_out) {
  const int i = wg_image[blockIdx.x];
  const ScanDecImage im = images[i];
  const ScanDecState mine = {st.entry + im.lane0, st.exit + im.lane0, st.count + im.lane0};
  scandec_sync_body<true>(data + im.data_at, T + i, im.g, mine, nullptr, bnd_out + im.wg0, nullptr, (int)blockIdx.x - im.wg0);
}
// changed: one word per stream, zero when the kernel starts.  A stream of one workgroup has nothing to do here.
__global__ __launch_bounds__(256) void k_scandec_sync_next_batch(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T,
                                                                 const ScanDecImage* __restrict__ images, const int* __restrict__ wg_image,
                                                                 ScanDecState st, const unsigned long long* __restrict__ bnd_in,
                                                                 unsigned long long* __restrict__ bnd_out, unsigned* __restrict__ changed) {
  const int i = wg_image[blockIdx.x];
  const ScanDecImage im = images[i];
  if (im.nwg == 1) return;   // (the whole workgroup)
  const ScanDecState mine = {st.entry + im.lane0, st.exit + im.lane0, st.count + im.lane0};
  scandec_sync_body<false>(data + im.data_at, T + i, im.g, mine, bnd_in + im.wg0, bnd_out + im.wg0, changed + i, (int)blockIdx.x - im.wg0);
}
// off: the prefix sums over ALL padded lanes; res: four words per stream.  (the output mode only)
__global__ __launch_bounds__(256) void k_scandec_write_batch(const uint8_t* __restrict__ data, const ScanDecTables* __restrict__ T,
                                                             const ScanDecImage* __restrict__ images, const int* __restrict__ wg_image,
                                                             const unsigned long long* __restrict__ entry,
                                                             const unsigned long long* __restrict__ off, int16_t* __restrict__ coeffs,
                                                             int16_t* __restrict__ dcd, unsigned* __restrict__ res) {
  const int i = wg_image[blockIdx.x];
  const ScanDecImage im = images[i];
  scandec_write_body<false>(data + im.data_at, T + i, im.g, entry + im.lane0, off + im.lane0, coeffs + im.coeff_at, dcd + im.block0,
                            res + 4 * i, (int)blockIdx.x - im.wg0, off[im.lane0]);
}
// grid (component, stream): one workgroup per pair.
__global__ __launch_bounds__(256) void k_scandec_dc_batch(const int16_t* __restrict__ dcd, const ScanDecTables* __restrict__ T,
                                                          const ScanDecImage* __restrict__ images, int16_t* __restrict__ coeffs,
                                                          unsigned* __restrict__ res) {
  const int i = (int)blockIdx.y;
  const ScanDecImage im = images[i];
  scandec_dc_body<false>(dcd + im.block0, T + i, im.g, coeffs + im.coeff_at, res + 4 * i);
}

// ---------------------------------------------------------------------------------------------- host side ----
// Where the host's BitReader stops handing out data in [0, len): the first 0xff that no 0x00 follows (pairs taken in
// order), or len - 2.  len >= 2.
inline size_t scandec_data_end(const uint8_t* data, size_t len) {
  const size_t stop = len - 2;
  size_t i = 0;
  while (i < stop) {
    const uint8_t* f = (const uint8_t*)memchr(data + i, 0xff, stop - i);
    if (!f) return stop;
    i = (size_t)(f - data);
    if (data[i + 1] != 0) return i;   // (i + 1 <= len - 2)
    i += 2;
  }
  return stop;
}

// One table from a DHT's 16 counts and its values, as HuffTable::Build; false for what ProcessDHT refuses.
inline bool scandec_build_table(ScanDecTables* T, int slot, bool is_ac, const uint8_t counts[16], const uint8_t* values) {
  int total = 0, longest = 1;
  long space = 1L << 16;
  for (int l = 1; l <= 16; ++l) {
    if (counts[l - 1]) longest = l;
    total += counts[l - 1];
    space -= (long)counts[l - 1] << (16 - l);
  }
  if (total > (is_ac ? 256 : 12)) return false;
  bool used[256] = {false};
  for (int i = 0; i < total; ++i) {
    if ((!is_ac && values[i] > 11) || used[values[i]]) return false;
    used[values[i]] = true;
  }
  if (space - (1L << (16 - longest)) < 0) return false;
  memset(T->fast[slot], 0, sizeof(T->fast[slot]));
  memset(T->values[slot], 0, sizeof(T->values[slot]));
  memcpy(T->values[slot], values, (size_t)total);
  T->num_values[slot] = total;
  T->maxcode[slot][0] = -1;
  T->mincode[slot][0] = T->valptr[slot][0] = 0;
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    T->valptr[slot][len] = k;
    T->mincode[slot][len] = code;
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code)
      if (len <= 9)
        for (int j = 0; j < (1 << (9 - len)); ++j) T->fast[slot][(code << (9 - len)) + j] = (uint16_t)(((len << 8) | values[k]) + 1);
    T->maxcode[slot][len] = counts[len - 1] ? code - 1 : -1;
    code <<= 1;
  }
  T->maxcode[slot][17] = 0x7fffffff;
  return true;
}

inline void launch_scandec_sync_first(hipStream_t stream, const uint8_t* data, const ScanDecTables* T, const ScanDecGeom& g,
                                      const ScanDecState& st, unsigned long long* bnd_out) {
  GZ_LAUNCH(k_scandec_sync_first, dim3(gz_div_up(g.nsub, kScanDecLanes)), dim3(kScanDecLanes), stream, data, T, g, st, bnd_out);
}
inline void launch_scandec_sync_next(hipStream_t stream, const uint8_t* data, const ScanDecTables* T, const ScanDecGeom& g,
                                     const ScanDecState& st, const unsigned long long* bnd_in, unsigned long long* bnd_out, unsigned* changed) {
  GZ_LAUNCH(k_scandec_sync_next, dim3(gz_div_up(g.nsub, kScanDecLanes)), dim3(kScanDecLanes), stream, data, T, g, st, bnd_in, bnd_out, changed);
}
inline void launch_scandec_write(hipStream_t stream, const uint8_t* data, const ScanDecTables* T, const ScanDecGeom& g,
                                 const unsigned long long* entry, const unsigned long long* off, int16_t* coeffs, int16_t* dcd, unsigned* res) {
  GZ_LAUNCH(k_scandec_write, dim3(gz_div_up(g.nsub, kScanDecLanes)), dim3(kScanDecLanes), stream, data, T, g, entry, off, coeffs, dcd, res);
}
inline void launch_scandec_dc(hipStream_t stream, int ncomp, const int16_t* dcd, const ScanDecTables* T, const ScanDecGeom& g, int16_t* coeffs,
                              unsigned* res) {
  GZ_LAUNCH(k_scandec_dc, dim3(ncomp), dim3(kScanDecLanes), stream, dcd, T, g, coeffs, res);
}
// The input mode: coeffs holds g.total * 64 elements, res four words of which res[2] is zero.
inline void launch_scandec_write_input(hipStream_t stream, const uint8_t* data, const ScanDecTables* T, const ScanDecGeom& g,
                                       const unsigned long long* entry, const unsigned long long* off, int16_t* coeffs, int16_t* dcd,
                                       unsigned* res) {
  GZ_LAUNCH(k_scandec_write_input, dim3(gz_div_up(g.nsub, kScanDecLanes)), dim3(kScanDecLanes), stream, data, T, g, entry, off, coeffs, dcd, res);
}
inline void launch_scandec_dc_input(hipStream_t stream, int ncomp, const int16_t* dcd, const ScanDecTables* T, const ScanDecGeom& g,
                                    int16_t* coeffs, unsigned* res) {
  GZ_LAUNCH(k_scandec_dc_input, dim3(ncomp), dim3(kScanDecLanes), stream, dcd, T, g, coeffs, res);
}
// The batched forms: nwg workgroups in all, n streams.
inline void launch_scandec_sync_first_batch(hipStream_t stream, int nwg, const uint8_t* data, const ScanDecTables* T, const ScanDecImage* images,
                                            const int* wg_image, const ScanDecState& st, unsigned long long* bnd_out) {
  GZ_LAUNCH(k_scandec_sync_first_batch, dim3(nwg), dim3(kScanDecLanes), stream, data, T, images, wg_image, st, bnd_out);
}
inline void launch_scandec_sync_next_batch(hipStream_t stream, int nwg, const uint8_t* data, const ScanDecTables* T, const ScanDecImage* images,
                                           const int* wg_image, const ScanDecState& st, const unsigned long long* bnd_in,
                                           unsigned long long* bnd_out, unsigned* changed) {
  GZ_LAUNCH(k_scandec_sync_next_batch, dim3(nwg), dim3(kScanDecLanes), stream, data, T, images, wg_image, st, bnd_in, bnd_out, changed);
}
inline void launch_scandec_write_batch(hipStream_t stream, int nwg, const uint8_t* data, const ScanDecTables* T, const ScanDecImage* images,
                                       const int* wg_image, const unsigned long long* entry, const unsigned long long* off, int16_t* coeffs,
                                       int16_t* dcd, unsigned* res) {
  GZ_LAUNCH(k_scandec_write_batch, dim3(nwg), dim3(kScanDecLanes), stream, data, T, images, wg_image, entry, off, coeffs, dcd, res);
}
inline void launch_scandec_dc_batch(hipStream_t stream, int ncomp, int n, const int16_t* dcd, const ScanDecTables* T, const ScanDecImage* images,
                                    int16_t* coeffs, unsigned* res) {
  GZ_LAUNCH(k_scandec_dc_batch, dim3(ncomp, n), dim3(kScanDecLanes), stream, dcd, T, images, coeffs, res);
}

}  // namespace gz
