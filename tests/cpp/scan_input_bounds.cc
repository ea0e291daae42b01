// TEST ONLY (CPU, host sanitizers): the scan decoder with passes 3 and 4 in their INPUT mode (k_scandec_write_input,
// k_scandec_dc_input of gz_kernels_scandec.h) through its launch code, as gz_decode_scan_input runs it, at 16, 64 and 128
// bytes per lane on
//   argv[1]  the JPEGs of tests/golden/scan_decode/,
//   argv[2]  those of tests/golden/jpeg_input_device/ (MCU padding with content),
//   argv[3]  the padded synthetic streams of tests/jpeg_input_device_cases.py, written out by the test that runs this,
// and on 2000 mutated streams of them -- single-bit flips and single-byte replacements in the scan.  The destination is
// malloc'ed to EXACTLY total * 64 int16 -- the blocks of the scan, MCU padding included, and not one more --, the result
// words to the three the kernels use, the stream to the bytes the decoder may read, every state array to its last lane,
// the DC differences to the scan's last block.  Built with -DGZ_EMU -fsanitize=address,undefined against
// tests/emu/hip_emu.h: a read or a store outside any of them is a heap-buffer-overflow report, a shift or an index out of
// range a UBSan report.  For the files as they are the scan must come back decoded with its end at the EOI, the
// large-coefficient word as CheckJpegSanity judges the file, and as many values at every lane size; for the mutated ones
// any verdict will do: what the program looks for is an access outside the buffers.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_kernels_scandec.h"

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

struct Parsed {
  int w = 0, h = 0, ncomp = 0, factor = 1;
  size_t scan_at = 0;
  gz::ScanDecTables tables;
};

// The segments in front of the first SOS of a well-formed baseline file.
bool parse(const std::vector<uint8_t>& d, Parsed* p) {
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
      p->scan_at = pos + 2 + n;
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

// The passes as gz_decode_scan_input runs them.  Returns 0 decoded, 1 not converged, 2 refused; *end_bit where it ended,
// *large the large-coefficient word, *nonzero how many values the destination holds.
int run(const Parsed& p, const uint8_t* scan, size_t len, int subseq, int max_rounds, unsigned* end_bit, unsigned* large, long* nonzero) {
  const size_t end = gz::scandec_data_end(scan, len);
  gz::ScanDecGeom g;
  memset(&g, 0, sizeof(g));
  const int f = p.factor;
  g.mcu_cols = (p.w + 8 * f - 1) / (8 * f);
  const int mcu_rows = (p.h + 8 * f - 1) / (8 * f);
  g.units = p.ncomp == 1 ? 1 : f == 2 ? 6 : 3;
  g.total = g.mcu_cols * mcu_rows * g.units;
  g.bw = (p.w + 7) / 8; g.bh = (p.h + 7) / 8;
  g.cbw = g.mcu_cols; g.cbh = mcu_rows;
  g.subseq_bytes = subseq;
  g.end_bits = (unsigned)(end * 8);
  g.nsub = (int)((end + (size_t)subseq - 1) / (size_t)subseq);
  if (g.nsub < 1) g.nsub = 1;
  const int nwg = gz_div_up(g.nsub, gz::kScanDecLanes);
  const size_t ncoeff = (size_t)g.total * 64;   // the reader's own grids: every block of the scan, and no more

  uint8_t* data = exact<uint8_t>(end);
  memcpy(data, scan, end);
  gz::ScanDecTables* T = exact<gz::ScanDecTables>(1);
  *T = p.tables;
  gz::ScanDecState st;
  st.entry = exact<unsigned long long>(g.nsub);
  st.exit = exact<unsigned long long>(g.nsub);
  st.count = exact<unsigned>(g.nsub);
  unsigned long long* off = exact<unsigned long long>((size_t)g.nsub + 1);
  unsigned long long* bnd = exact<unsigned long long>(2 * (size_t)nwg);
  unsigned* changed = exact<unsigned>(1);
  unsigned* res = exact<unsigned>(3);
  int16_t* coeffs = exact<int16_t>(ncoeff);
  int16_t* dcd = exact<int16_t>(g.total);
  const int tiles = gz_div_up(g.nsub, gz::kScanTile);
  gz::ScanState ss;
  ss.agg = exact<unsigned long long>(tiles);
  ss.incl = exact<unsigned long long>(tiles);
  ss.status = exact<unsigned>(tiles);
  ss.ticket = exact<unsigned>(1);
  memset(ss.agg, 0, 8 * (size_t)tiles); memset(ss.incl, 0, 8 * (size_t)tiles); memset(ss.status, 0, 4 * (size_t)tiles);
  *ss.ticket = 0;
  memset(coeffs, 0, ncoeff * 2);
  memset(dcd, 0, 2 * (size_t)g.total);
  res[0] = res[1] = 0xffffffffu;
  res[2] = 0;

  const hipStream_t stream = nullptr;
  gz::launch_scandec_sync_first(stream, data, T, g, st, bnd);
  int used = 0;
  bool converged = nwg == 1;
  while (!converged && used < max_rounds) {
    ++used;
    *changed = 0;
    gz::launch_scandec_sync_next(stream, data, T, g, st, bnd + (size_t)((used - 1) & 1) * nwg, bnd + (size_t)(used & 1) * nwg, changed);
    converged = *changed == 0;
  }
  int verdict = 1;
  if (converged) {
    GZ_LAUNCH(gz::k_scan_offsets, dim3(tiles), dim3(256), stream, (const unsigned*)st.count, g.nsub, off, ss, 1u);
    gz::launch_scandec_write_input(stream, data, T, g, st.entry, off, coeffs, dcd, res);
    gz::launch_scandec_dc_input(stream, p.ncomp, dcd, T, g, coeffs, res);
    verdict = res[0] == 0xffffffffu && res[1] != 0xffffffffu && res[1] <= g.end_bits ? 0 : 2;
    *end_bit = res[1];
    *large = res[2];
    long n = 0;
    for (size_t i = 0; i < ncoeff; ++i) n += coeffs[i] != 0;
    *nonzero = n;
  }
  free(data); free(T); free(st.entry); free(st.exit); free(st.count); free(off); free(bnd); free(changed); free(res);
  free(coeffs); free(dcd); free(ss.agg); free(ss.incl); free(ss.status); free(ss.ticket);
  return verdict;
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

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { printf("usage: scan_input_bounds <tests/golden/scan_decode> <tests/golden/jpeg_input_device> <padded streams>\n"); return 2; }
  struct Named { int dir; const char* name; int large; };   // large: what CheckJpegSanity says of the stream
  const Named names[] = {
      {1, "64x48_q90_444", 0}, {1, "61x43_q85_420", 0}, {1, "96x64_q75_444_opt", 0}, {1, "33x31_grey", 0}, {1, "8x8_444", 0},
      {1, "8x8_420", 0}, {1, "1x1_444", 0}, {1, "1x1_420", 0}, {1, "9x8_444", 0}, {1, "9x8_420", 0}, {1, "17x9_444", 0},
      {1, "17x9_420", 0}, {1, "160x120_q95_444", 0},
      {2, "40x40_420", 0}, {2, "72x40_420", 0}, {2, "64x40_420", 0}, {2, "40x40_444", 0},
      {3, "large_dc_in_padding", 1}, {3, "large_ac_in_padding", 1}, {3, "exactly_4096_in_padding", 0}, {3, "extremes_in_padding", 0}};
  const int sizes[] = {16, 64, 128};
  std::vector<std::vector<uint8_t>> files;
  std::vector<Parsed> parsed;
  long runs = 0;
  for (const Named& nm : names) {
    std::vector<uint8_t> d;
    Parsed p;
    if (!read_file(std::string(argv[nm.dir]) + "/" + nm.name + ".jpg", &d) || !parse(d, &p)) { printf("cannot read %s\n", nm.name); return 2; }
    long first_nonzero = -1;
    for (int s : sizes) {
      unsigned end_bit = 0, large = 0;
      long nonzero = 0;
      const int v = run(p, d.data() + p.scan_at, d.size() - p.scan_at, s, 16, &end_bit, &large, &nonzero);
      ++runs;
      if (first_nonzero < 0) first_nonzero = nonzero;
      if (v != 0 || p.scan_at + (end_bit + 7) / 8 != d.size() - 2 || (large != 0) != (nm.large != 0) || nonzero != first_nonzero) {
        printf("MISMATCH %s at %d bytes per lane: verdict %d, the scan ends at bit %u, large %u, %ld values\n", nm.name, s, v, end_bit,
               large, nonzero);
        return 1;
      }
    }
    files.push_back(d);
    parsed.push_back(p);
  }
  // 2000 mutated streams: the first three files, the multi-workgroup one, the 4:2:0 fixtures with padding, two padded streams
  uint64_t s = 88172645463325252ull;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  long verdicts[3] = {0, 0, 0};
  const int pick[8] = {0, 1, 2, 12, 13, 14, 19, 20};
  for (int i = 0; i < 2000; ++i) {
    const int which = pick[i % 8];
    std::vector<uint8_t> d = files[which];
    const Parsed& p = parsed[which];
    const size_t at = p.scan_at + next() % (d.size() - p.scan_at);   // (the EOI included: the end of the data moves too)
    if (i & 8) d[at] = (uint8_t)next(); else d[at] ^= (uint8_t)(1u << (next() & 7));
    unsigned end_bit = 0, large = 0;
    long nonzero = 0;
    // (one round only now and then: the verdict "not converged" is a path too)
    ++verdicts[run(p, d.data() + p.scan_at, d.size() - p.scan_at, sizes[i % 3], i % 7 == 0 ? 1 : 16, &end_bit, &large, &nonzero)];
    ++runs;
  }
  printf("%ld runs; of the mutated streams %ld decoded, %ld not converged, %ld refused\n", runs, verdicts[0], verdicts[1], verdicts[2]);
  printf("no access outside the buffers\n");
  return 0;
}
