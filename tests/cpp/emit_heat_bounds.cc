// TEST ONLY (CPU, host sanitizers): the heat map's kernel k_emit_heat of gz_kernels_emitheat.h through its launch code,
// over every layout, element type and size the tests use, from source planes malloc'ed to EXACTLY w * h floats (and one
// float further on, so that no row starts 16-byte aligned) into destinations malloc'ed to EXACTLY the last addressed
// element + 1.  Built with -DGZ_EMU -fsanitize=address,undefined against tests/emu/hip_emu.h: a 16-byte load or store,
// or a row's tail, that leaves its buffer is a heap-buffer-overflow report, a misaligned 16-byte access an alignment
// report, a conversion of the colour arithmetic that leaves its type's range a UBSan report.  The elements are checked
// against ScoreToRgb restated here with the host's pow, and the elements of a canvas that are no part of the image
// against the sentinel they were filled with.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_kernels_emitheat.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

enum { kU8 = 0, kF32 = 1, kF16 = 2, kBF16 = 3, kU16 = 4 };

void score_to_rgb(double score, double good, double bad, uint8_t rgb[3]) {
  static const double heatmap[12][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {0, 1, 0}, {1, 1, 0}, {1, 0, 0}, {1, 0, 1}, {0.5, 0.5, 1.0},
                                        {1.0, 0.5, 0.5}, {1.0, 1.0, 0.5}, {1, 1, 1}, {1, 1, 1}};
  if (score < good) score = (score / good) * 0.3;
  else if (score < bad) score = 0.3 + (score - good) / (bad - good) * 0.15;
  else score = 0.45 + (score - bad) / (bad * 12) * 0.5;
  score = std::min<double>(std::max<double>(score * 11, 0.0), 10);
  const int ix = static_cast<int>(score);
  const double mix = score - ix;
  volatile double half = 0.5;
  for (int i = 0; i < 3; ++i) {
    const double v = mix * heatmap[ix + 1][i] + (1 - mix) * heatmap[ix][i];
    rgb[i] = static_cast<uint8_t>(255 * pow(v, half) + 0.5);
  }
}

// the storage bits of the element of byte b (tests/cpp/emit_bounds.cc)
uint32_t expected_bits(int dtype, uint8_t b) {
  if (dtype == kU8) return b;
  if (dtype == kU16) return (uint32_t)b * 257u;
  volatile float f = (float)b / 255.0f;
  const float g = f;
  uint32_t u;
  memcpy(&u, &g, 4);
  if (dtype == kF32) return u;
  if (dtype == kBF16) return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  if (u == 0) return 0;
  const uint32_t e = (u >> 23) - 112u, m = u & 0x7fffffu;
  uint32_t h = (e << 10) | (m >> 13);
  const uint32_t rest = m & 0x1fffu;
  if (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ++h;
  return h;
}

// 0 HWC, 1 CHW, 2 HWC crop, 3 CHW crop, 4 WHC, 5 HWC + 1, 6 CHW crop + 1, 7 HWC with a pitch of 3 w + 1
struct Layout { const char* name; int kind; };
const Layout kLayouts[] = {{"HWC", 0}, {"CHW", 1}, {"HWC crop", 2}, {"CHW crop", 3}, {"WHC", 4}, {"HWC base+1", 5}, {"CHW crop base+1", 6},
                           {"HWC pitch+1", 7}};

uint32_t load(const void* mem, size_t elem, size_t i) {
  return elem == 1 ? ((const uint8_t*)mem)[i] : elem == 2 ? ((const uint16_t*)mem)[i] : ((const uint32_t*)mem)[i];
}

int run_case(int dtype, const Layout& lay, int w, int h, int src_lead, const float* lut, const double* thr, long* cases) {
  const size_t elem = dtype == kU8 ? 1 : dtype == kF32 ? 4 : 2;
  int64_t sy, sx, sc;
  const int64_t cw = (w + 16 + 15) / 16 * 16, ch = h + 2;   // the canvas of a crop: rows of a multiple of 16 pixels
  int64_t lead = 0;                                          // elements in front of (0, 0, 0) that belong to the allocation
  switch (lay.kind) {
    case 0: case 5: sy = 3 * (int64_t)w; sx = 3; sc = 1; break;
    case 1: sy = w; sx = 1; sc = (int64_t)w * h; break;
    case 2: sy = 3 * cw; sx = 3; sc = 1; lead = (1 * cw + 16) * 3; break;
    case 3: case 6: sy = cw; sx = 1; sc = cw * ch; lead = 1 * cw + 16; break;
    case 7: sy = 3 * (int64_t)w + 1; sx = 3; sc = 1; break;
    default: sy = 3; sx = 3 * (int64_t)h; sc = 1; break;
  }
  if (lay.kind == 5 || lay.kind == 6) lead += 1;
  const int64_t last = (int64_t)(h - 1) * sy + (int64_t)(w - 1) * sx + 2 * sc;
  const size_t count = (size_t)(lead + last + 1);
  // malloc returns 16-byte aligned memory, so `lead` and `src_lead` alone decide which paths the kernel may take
  void* mem = malloc(count * elem);
  float* plane = (float*)malloc(sizeof(float) * ((size_t)w * h + src_lead));
  if (!mem || !plane) return 2;
  memset(mem, 0xEE, count * elem);
  float* src = plane + src_lead;
  const double good = 0.7654828525846824, bad = 1.1413240259280428;
  uint64_t s = 88172645463325252ull + (uint64_t)w * 131 + (uint64_t)h;
  const float special[] = {0.0f, -0.0f, -1.0f, INFINITY, 3.4028235e38f, 1e-45f, (float)good, (float)bad, 0.25f, 16.2f, 1e-6f, 5.0f};
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    src[i] = (s >> 60) == 0 ? special[(s >> 40) % 12] : (float)((s >> 33) % 100000) * 1.7e-4f;   // 0 .. 17: past 14.2 bad
  }
  const gz::HeatScale hs = gz::heat_scale(good, bad);
  void* out = (char*)mem + (size_t)lead * elem;
  switch (dtype) {
    case kU8: gz::launch_emit_heat((hipStream_t) nullptr, src, w, h, w, (uint8_t*)out, sy, sx, sc, lut, thr, hs); break;
    case kF32: gz::launch_emit_heat((hipStream_t) nullptr, src, w, h, w, (float*)out, sy, sx, sc, lut, thr, hs); break;
    case kF16: gz::launch_emit_heat((hipStream_t) nullptr, src, w, h, w, (gz::ingest_f16*)out, sy, sx, sc, lut, thr, hs); break;
    case kBF16: gz::launch_emit_heat((hipStream_t) nullptr, src, w, h, w, (gz::ingest_bf16*)out, sy, sx, sc, lut, thr, hs); break;
    default: gz::launch_emit_heat((hipStream_t) nullptr, src, w, h, w, (uint16_t*)out, sy, sx, sc, lut, thr, hs); break;
  }
  std::vector<uint8_t> is_image(count, 0);
  int bad_case = 0;
  for (int y = 0; y < h && !bad_case; ++y)
    for (int x = 0; x < w && !bad_case; ++x) {
      uint8_t rgb[3];
      score_to_rgb((double)src[(size_t)y * w + x], good, bad, rgb);
      for (int c = 0; c < 3; ++c) {
        const size_t i = (size_t)(lead + y * sy + x * sx + c * sc);
        is_image[i] = 1;
        if (load(mem, elem, i) != expected_bits(dtype, rgb[c])) {
          printf("MISMATCH dtype %d %s %dx%d at (%d, %d, %d): %a -> %08x, expected byte %d = %08x\n", dtype, lay.name, w, h, y, x, c,
                 (double)src[(size_t)y * w + x], load(mem, elem, i), rgb[c], expected_bits(dtype, rgb[c]));
          bad_case = 1;
          break;
        }
      }
    }
  const uint32_t sentinel = elem == 1 ? 0xEEu : elem == 2 ? 0xEEEEu : 0xEEEEEEEEu;
  for (size_t i = 0; i < count && !bad_case; ++i)
    if (!is_image[i] && load(mem, elem, i) != sentinel) {
      printf("TOUCHED dtype %d %s %dx%d: element %zu outside the image is %08x\n", dtype, lay.name, w, h, i, load(mem, elem, i));
      bad_case = 1;
    }
  free(mem);
  free(plane);
  ++*cases;
  return bad_case;
}

}  // namespace

int main() {
  const gz::HeatThresholds& t = gz::heat_thresholds();
  if (!t.ok) {
    printf("%s\n", t.why.c_str());
    return 1;
  }
  // the kernel's two tables, each malloc'ed to its exact size
  float* lut = (float*)malloc(sizeof(float) * 256);
  double* thr = (double*)malloc(sizeof(double) * 255);
  memcpy(lut, gz::emit_lut(), sizeof(float) * 256);
  memcpy(thr, t.thr, sizeof(double) * 255);
  const int widths[] = {1, 3, 4, 5, 15, 16, 17, 33, 67}, heights[] = {1, 2, 9};
  long cases = 0;
  int bad = 0;
  for (int dtype = kU8; dtype <= kU16; ++dtype)
    for (const Layout& lay : kLayouts)
      for (int w : widths)
        for (int h : heights)
          for (int src_lead = 0; src_lead < 2; ++src_lead) bad |= run_case(dtype, lay, w, h, src_lead, lut, thr, &cases);
  free(lut);
  free(thr);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all elements as expected, no access outside the buffers");
  return bad;
}
