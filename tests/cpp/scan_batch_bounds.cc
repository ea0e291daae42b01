// TEST ONLY (CPU, host sanitizers): the batched kernels of gz_kernels_scandec.h (and k_scan_offsets between them) through
// their launch code, every buffer malloc'ed to EXACTLY the bytes the batch's layout gives it: the streams one after the
// other at 16-byte aligned offsets up to the last stream's last readable byte, one ScanDecTables and one ScanDecImage per
// stream, the workgroups' images, entry / exit / count to the last padded lane, the prefix sums to lanes + 1, the two
// boundary arrays to the last workgroup, one word per stream for the round, the DC differences to the last stream's last
// block, the coefficient arenas to the last frame's last block, four result words per stream.  Built with -DGZ_EMU
// -fsanitize=address,undefined against tests/emu/hip_emu.h: a read or a store outside any of them is a
// heap-buffer-overflow report.  The batches: streams of exactly 256, 257 and 1 lanes at 16 bytes a lane in every order;
// a stream that does not synchronise inside a workgroup between two that need no round; 2000 mutated streams of the
// JPEGs of tests/golden/scan_decode/ (argv[1]) in batches of 8, the unmutated file among them.  Every stream is also run
// ALONE through the same kernels (a batch of one): verdict, rounds and end must be the same inside the batch, and so
// must the coefficients of a stream that decodes.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_kernels_scandec.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

const int kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One member of a batch: the frame, the tables, the scan's bytes to the end of the file.
struct Stream {
  int w = 0, h = 0, ncomp = 0, factor = 1;
  gz::ScanDecTables tables;
  std::vector<uint8_t> scan;
};

// The segments in front of the first SOS of a well-formed baseline file.
bool parse(const std::vector<uint8_t>& d, Stream* p, size_t* scan_at) {
  int quant[4][64] = {{0}};
  uint8_t counts[2][4][16] = {{{0}}}, values[2][4][256] = {{{0}}};
  int comp_tq[3] = {0, 0, 0}, hv0 = 0x11;
  memset(&p->tables, 0, sizeof(p->tables));
  size_t pos = 2;
  while (pos + 4 <= d.size()) {
    if (d[pos] != 0xff) return false;
    const int m = d[pos + 1];
    const size_t n = (size_t)(d[pos + 2] << 8 | d[pos + 3]);
    const uint8_t* s = &d[pos + 4];
    const size_t len = n - 2;
    if (m == 0xdb) {
      for (size_t i = 0; i < len;) {
        const int prec = s[i] >> 4, tq = s[i] & 3;
        ++i;
        for (int k = 0; k < 64; ++k) {
          quant[tq][kNatural[k]] = prec ? (s[i] << 8 | s[i + 1]) : s[i];
          i += prec ? 2 : 1;
        }
      }
    } else if (m == 0xc4) {
      for (size_t i = 0; i < len;) {
        const int tc = s[i] >> 4, th = s[i] & 3;
        int total = 0;
        for (int l = 0; l < 16; ++l) total += (counts[tc][th][l] = s[i + 1 + l]);
        memcpy(values[tc][th], s + i + 17, (size_t)total);
        i += 17 + (size_t)total;
      }
    } else if (m == 0xc0 || m == 0xc1) {
      p->h = s[1] << 8 | s[2];
      p->w = s[3] << 8 | s[4];
      p->ncomp = s[5];
      if (p->ncomp != 1 && p->ncomp != 3) return false;
      hv0 = s[7];
      for (int c = 0; c < p->ncomp; ++c) comp_tq[c] = s[8 + 3 * c] & 3;
    } else if (m == 0xda) {
      p->factor = p->ncomp == 3 && hv0 == 0x22 ? 2 : 1;
      for (int c = 0; c < p->ncomp; ++c) {
        const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 3;
        if (!gz::scandec_build_table(&p->tables, c, false, counts[0][td & 3], values[0][td & 3])) return false;
        if (!gz::scandec_build_table(&p->tables, 3 + c, true, counts[1][ta], values[1][ta])) return false;
        for (int k = 0; k < 64; ++k) p->tables.quant[c][k] = quant[comp_tq[c]][k];
      }
      *scan_at = pos + 2 + n;
      return true;
    } else if (m == 0xc2) {
      return false;
    }
    pos += 2 + n;
  }
  return false;
}

template <class T>
T* exact(size_t count) {
  T* p = (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1);
  if (!p) abort();
  return p;
}

struct Verdict {
  int status = 1;   // 0 decoded, 1 not converged, 2 refused
  int rounds = 0;
  unsigned end_bit = 0;
  std::vector<int16_t> coeffs;   // of a stream that decoded
  bool operator==(const Verdict& o) const { return status == o.status && rounds == o.rounds && end_bit == o.end_bit && coeffs == o.coeffs; }
};

// The passes as the library's batched entry runs them, on one chunk.
std::vector<Verdict> run(const std::vector<const Stream*>& batch, int subseq, int max_rounds) {
  const int m = (int)batch.size();
  const Stream& s0 = *batch[0];
  const int f = s0.factor;
  const int mcu_cols = (s0.w + 8 * f - 1) / (8 * f), mcu_rows = (s0.h + 8 * f - 1) / (8 * f);
  const int bw = (s0.w + 7) / 8, bh = (s0.h + 7) / 8;
  const size_t nblk = (size_t)bw * bh + 2 * (size_t)mcu_cols * mcu_rows;
  std::vector<gz::ScanDecImage> im((size_t)m);
  std::vector<size_t> ends((size_t)m);
  size_t upload = 0, lanes = 0, wgs = 0, blocks = 0, last_end = 0;
  for (int j = 0; j < m; ++j) {
    const Stream& s = *batch[(size_t)j];
    gz::ScanDecGeom g;
    memset(&g, 0, sizeof(g));
    g.mcu_cols = mcu_cols;
    g.units = s.ncomp == 1 ? 1 : f == 2 ? 6 : 3;
    g.total = mcu_cols * mcu_rows * g.units;
    g.bw = bw; g.bh = bh; g.cbw = mcu_cols; g.cbh = mcu_rows;
    g.subseq_bytes = subseq;
    const size_t end = gz::scandec_data_end(s.scan.data(), s.scan.size());
    ends[(size_t)j] = end;
    g.end_bits = (unsigned)(end * 8);
    g.nsub = std::max(1, (int)((end + (size_t)subseq - 1) / (size_t)subseq));
    memset(&im[(size_t)j], 0, sizeof(gz::ScanDecImage));
    im[(size_t)j].g = g;
    im[(size_t)j].nwg = gz_div_up(g.nsub, gz::kScanDecLanes);
    im[(size_t)j].data_at = upload;
    im[(size_t)j].coeff_at = (unsigned long long)j * nblk * 64;
    im[(size_t)j].wg0 = (int)wgs;
    im[(size_t)j].lane0 = (int)lanes;
    im[(size_t)j].block0 = (int)blocks;
    last_end = upload + end;
    upload += (std::max<size_t>(end, 1) + 15) & ~(size_t)15;
    lanes += (size_t)im[(size_t)j].nwg * gz::kScanDecLanes;
    wgs += (size_t)im[(size_t)j].nwg;
    blocks += (size_t)g.total;
  }
  // (the last stream's padding is not part of the buffer: nothing may read it)
  uint8_t* data = exact<uint8_t>(last_end);
  gz::ScanDecTables* T = exact<gz::ScanDecTables>((size_t)m);
  gz::ScanDecImage* images = exact<gz::ScanDecImage>((size_t)m);
  int* wg_image = exact<int>(wgs);
  for (int j = 0; j < m; ++j) {
    memcpy(data + im[(size_t)j].data_at, batch[(size_t)j]->scan.data(), ends[(size_t)j]);
    T[j] = batch[(size_t)j]->tables;
    images[j] = im[(size_t)j];
    for (int k = 0; k < im[(size_t)j].nwg; ++k) wg_image[im[(size_t)j].wg0 + k] = j;
  }
  gz::ScanDecState st;
  st.entry = exact<unsigned long long>(lanes);
  st.exit = exact<unsigned long long>(lanes);
  st.count = exact<unsigned>(lanes);
  memset(st.count, 0, 4 * lanes);
  unsigned long long* off = exact<unsigned long long>(lanes + 1);
  unsigned long long* bnd = exact<unsigned long long>(2 * wgs);
  unsigned* changed = exact<unsigned>((size_t)m);
  unsigned* res = exact<unsigned>(4 * (size_t)m);
  int16_t* coeffs = exact<int16_t>((size_t)m * nblk * 64);
  int16_t* dcd = exact<int16_t>(blocks);
  const int tiles = gz_div_up((int)lanes, gz::kScanTile);
  gz::ScanState ss;
  ss.agg = exact<unsigned long long>(tiles);
  ss.incl = exact<unsigned long long>(tiles);
  ss.status = exact<unsigned>(tiles);
  ss.ticket = exact<unsigned>(1);
  memset(ss.agg, 0, 8 * (size_t)tiles); memset(ss.incl, 0, 8 * (size_t)tiles); memset(ss.status, 0, 4 * (size_t)tiles);
  *ss.ticket = 0;
  memset(coeffs, 0, (size_t)m * nblk * 128);
  memset(dcd, 0, 2 * blocks);
  memset(res, 0xff, 16 * (size_t)m);

  const hipStream_t stream = nullptr;
  const int nwg = (int)wgs;
  std::vector<Verdict> out((size_t)m);
  gz::launch_scandec_sync_first_batch(stream, nwg, data, T, images, wg_image, st, bnd);
  std::vector<char> converged((size_t)m);
  int open = 0, used = 0;
  for (int j = 0; j < m; ++j) open += (converged[(size_t)j] = im[(size_t)j].nwg == 1) ? 0 : 1;
  while (open > 0 && used < max_rounds) {
    ++used;
    memset(changed, 0, 4 * (size_t)m);
    gz::launch_scandec_sync_next_batch(stream, nwg, data, T, images, wg_image, st, bnd + (size_t)((used - 1) & 1) * wgs, bnd + (size_t)(used & 1) * wgs,
                                       changed);
    for (int j = 0; j < m; ++j) {
      if (converged[(size_t)j]) continue;
      out[(size_t)j].rounds = used;
      if (changed[j] == 0) { converged[(size_t)j] = 1; --open; }
    }
  }
  if (open < m) {
    GZ_LAUNCH(gz::k_scan_offsets, dim3(std::max(1, tiles)), dim3(256), stream, (const unsigned*)st.count, (int)lanes, off, ss, 1u);
    gz::launch_scandec_write_batch(stream, nwg, data, T, images, wg_image, st.entry, off, coeffs, dcd, res);
    gz::launch_scandec_dc_batch(stream, s0.ncomp, m, dcd, T, images, coeffs, res);
    for (int j = 0; j < m; ++j) {
      if (!converged[(size_t)j]) continue;
      const unsigned* r = res + 4 * j;
      Verdict& v = out[(size_t)j];
      v.status = r[0] == 0xffffffffu && r[1] != 0xffffffffu && r[1] <= im[(size_t)j].g.end_bits ? 0 : 2;
      if (v.status == 0) {
        v.end_bit = r[1];
        v.coeffs.assign(coeffs + (size_t)j * nblk * 64, coeffs + (size_t)(j + 1) * nblk * 64);
      }
    }
  }
  free(data); free(T); free(images); free(wg_image); free(st.entry); free(st.exit); free(st.count); free(off); free(bnd); free(changed);
  free(res); free(coeffs); free(dcd); free(ss.agg); free(ss.incl); free(ss.status); free(ss.ticket);
  return out;
}

// The batch, and every member alone: the same verdicts.
bool agree(const std::vector<const Stream*>& batch, int subseq, int max_rounds, std::vector<Verdict>* got, const char* what) {
  *got = run(batch, subseq, max_rounds);
  for (size_t j = 0; j < batch.size(); ++j) {
    const std::vector<Verdict> alone = run({batch[j]}, subseq, max_rounds);
    if (!(alone[0] == (*got)[j])) {
      printf("MISMATCH %s: member %zu is %d after %d rounds in the batch, %d after %d alone\n", what, j, (*got)[j].status, (*got)[j].rounds,
             alone[0].status, alone[0].rounds);
      return false;
    }
  }
  return true;
}

bool read_file(const std::string& path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
  fclose(f);
  return true;
}

// A grey stream coded by hand (tests/decode_batch_cases.py: grey_jpeg, slow_jpeg).  DC: the one symbol 0 under the code
// '0'.  AC of the plain streams: end of block '0', (run 0, size 1) '10', (run 0, size 10) '110'; of the slow one: (run 0,
// size 1) '0' alone.  bits: the scan's bits; ones are added to the next byte, then the EOI.
Stream grey(int w, int h, bool slow, const std::vector<uint8_t>& bits) {
  Stream s;
  s.w = w; s.h = h; s.ncomp = 1; s.factor = 1;
  memset(&s.tables, 0, sizeof(s.tables));
  uint8_t dc_counts[16] = {1}, dc_values[1] = {0};
  uint8_t ac_counts[16] = {1, 1, 1}, ac_values[3] = {0x00, 0x01, 0x0a};
  uint8_t slow_counts[16] = {1}, slow_values[1] = {0x01};
  if (!gz::scandec_build_table(&s.tables, 0, false, dc_counts, dc_values)) abort();
  if (!gz::scandec_build_table(&s.tables, 3, true, slow ? slow_counts : ac_counts, slow ? slow_values : ac_values)) abort();
  for (int k = 0; k < 64; ++k) s.tables.quant[0][k] = 1;
  std::vector<uint8_t> b = bits;
  while (b.size() % 8) b.push_back(1);
  for (size_t i = 0; i < b.size(); i += 8) {
    uint8_t v = 0;
    for (int k = 0; k < 8; ++k) v = (uint8_t)(v << 1 | b[i + k]);
    if (v == 0xff) abort();
    s.scan.push_back(v);
  }
  s.scan.push_back(0xff);
  s.scan.push_back(0xd9);
  return s;
}
// Blocks of `big` coefficients of 512 and, in the first `ones` blocks, one more of +1; then the end of block.
Stream grey_of(int w, int h, int big, int ones) {
  const int n = ((w + 7) / 8) * ((h + 7) / 8);
  std::vector<uint8_t> bits;
  for (int i = 0; i < n; ++i) {
    bits.push_back(0);
    for (int k = 0; k < big; ++k) {
      const uint8_t v[13] = {1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      bits.insert(bits.end(), v, v + 13);
    }
    for (int k = 0; k < (ones + n - 1 - i) / n; ++k) { bits.push_back(1); bits.push_back(0); bits.push_back(1); }
    bits.push_back(0);
  }
  return grey(w, h, false, bits);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: scan_batch_bounds <tests/golden/scan_decode>\n"); return 2; }
  long runs = 0;
  std::vector<Verdict> got;
  {
    // 64 x 64 grey, 64 blocks: 39 coefficients of 512 a block are 32576 bits; 44 more of +1 make 4089 bytes, 256 lanes at
    // 16 bytes; 65 make 4097 bytes, 257 lanes; none at all 16 bytes, one lane.
    const Stream s256 = grey_of(64, 64, 39, 44), s257 = grey_of(64, 64, 39, 65), s1 = grey_of(64, 64, 0, 0);
    if (s256.scan.size() - 2 != 4089 || s257.scan.size() - 2 != 4097 || s1.scan.size() - 2 != 16) { printf("the lane streams are not what they should be\n"); return 2; }
    const Stream* all[3] = {&s256, &s257, &s1};
    int order[3] = {0, 1, 2};
    do {
      const std::vector<const Stream*> batch = {all[order[0]], all[order[1]], all[order[2]]};
      if (!agree(batch, 16, 16, &got, "the 256 / 257 / 1-lane batch")) return 1;
      ++runs;
      for (int j = 0; j < 3; ++j)
        if (got[(size_t)j].status != 0 || got[(size_t)j].rounds != (order[j] == 1 ? 1 : 0)) { printf("MISMATCH the lane batch: member %d\n", j); return 1; }
    } while (std::next_permutation(order, order + 3));
  }
  {
    // 184 x 184 grey, 529 blocks of 127 zero bits: just over two workgroups at 16 bytes a lane, two rounds; between two
    // streams of a few lanes
    const Stream slow = grey(184, 184, true, std::vector<uint8_t>(127 * 529, 0));
    const Stream quick = grey_of(184, 184, 0, 0), other = grey_of(184, 184, 0, 100);
    const std::vector<const Stream*> batch = {&quick, &slow, &other};
    if (!agree(batch, 16, 16, &got, "the slow stream between neighbours")) return 1;
    if (got[0].status != 0 || got[1].status != 0 || got[2].status != 0 || got[0].rounds != 0 || got[1].rounds != 2 || got[2].rounds != 0) {
      printf("MISMATCH the slow stream: %d rounds, its neighbours %d and %d\n", got[1].rounds, got[0].rounds, got[2].rounds);
      return 1;
    }
    if (!agree(batch, 16, 1, &got, "the slow stream with one round")) return 1;
    if (got[0].status != 0 || got[1].status != 1 || got[2].status != 0) { printf("MISMATCH the slow stream with one round\n"); return 1; }
    if (!agree({&slow, &quick, &slow}, 16, 16, &got, "the slow stream first and last")) return 1;
    runs += 3;
  }
  // 2000 mutated streams of four files in batches of 8: the file as it is, and seven mutations of it
  const char* names[] = {"64x48_q90_444", "61x43_q85_420", "96x64_q75_444_opt", "160x120_q95_444"};
  const int sizes[] = {16, 64, 128};
  uint64_t seed = 88172645463325252ull;
  auto next = [&seed]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
  long verdicts[3] = {0, 0, 0}, mutated = 0;
  std::vector<Stream> files;
  for (const char* name : names) {
    std::vector<uint8_t> d;
    Stream s;
    size_t at = 0;
    if (!read_file(std::string(argv[1]) + "/" + name + ".jpg", &d) || !parse(d, &s, &at)) { printf("cannot read %s\n", name); return 2; }
    s.scan.assign(d.begin() + (long)at, d.end());
    files.push_back(s);
  }
  for (int b = 0; mutated < 2000; ++b) {
    const Stream& file = files[(size_t)b % files.size()];
    std::vector<Stream> members(8, file);
    for (int j = 1; j < 8; ++j, ++mutated) {
      std::vector<uint8_t>& d = members[(size_t)j].scan;
      const size_t at = next() % d.size();   // (the EOI included: the end of the data moves too)
      if (j & 4) d[at] = (uint8_t)next(); else d[at] ^= (uint8_t)(1u << (next() & 7));
    }
    std::vector<const Stream*> batch;
    for (const Stream& s : members) batch.push_back(&s);
    std::swap(batch[0], batch[(size_t)b % 8]);   // (the file as it is in every position)
    // (one round now and then: the verdict "not converged" is a path too)
    if (!agree(batch, sizes[b % 3], b % 7 == 0 ? 1 : 16, &got, file.scan.size() > 9000 ? "mutations of the multi-workgroup file" : "mutations")) return 1;
    ++runs;
    for (const Verdict& v : got) ++verdicts[v.status];
  }
  printf("%ld batches; of their members %ld decoded, %ld not converged, %ld refused\n", runs, verdicts[0], verdicts[1], verdicts[2]);
  printf("no access outside the buffers\n");
  return 0;
}
