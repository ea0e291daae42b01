// TEST ONLY (CPU, host sanitizers): the masking images' kernel k_emit_mask of gz_kernels_emitmask.h through its launch
// code, in every mode, element type and layout the tests use, from blurred planes malloc'ed to EXACTLY w * h floats (and
// one float further on, so that no row starts 16-byte aligned), a table of EXACTLY 4 * 512 doubles, into destinations
// malloc'ed to EXACTLY the last addressed element + 1.  Built with -DGZ_EMU -fsanitize=address,undefined against
// tests/emu/hip_emu.h: a 16-byte load or store, or a row's tail, that leaves its buffer is a heap-buffer-overflow report,
// a misaligned 16-byte access an alignment report, a table index outside [0, 511] an overflow report.  The elements are
// checked against mask_p0p1 / interp_lut512 / emit_map_value called pixel by pixel here, and the elements of a canvas
// that are no part of the image against the sentinel they were filled with.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_kernels_emitmask.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

// 0 HWC, 1 CHW, 2 HWC crop, 3 CHW crop, 4 WHC, 5 HWC + 1, 6 CHW crop + 1, 7 HWC with a pitch of 3 w + 1
struct Layout { const char* name; int kind; };
const Layout kLayouts[] = {{"HWC", 0}, {"CHW", 1}, {"HWC crop", 2}, {"CHW crop", 3}, {"WHC", 4}, {"HWC base+1", 5}, {"CHW crop base+1", 6},
                           {"HWC pitch+1", 7}};

struct Canvas {
  int64_t sy, sx, sc, lead;
  size_t count;
};
// planes: 3 for a mask, 1 for the quantisation field (a 2-D image: the layouts' channel stride is then not used)
Canvas canvas_of(const Layout& lay, int w, int h, int planes) {
  Canvas c;
  const int64_t cw = (w + 16 + 15) / 16 * 16, ch = h + 2;   // the canvas of a crop: rows of a multiple of 16 pixels
  c.lead = 0;
  const int64_t n = planes;
  switch (lay.kind) {
    case 0: case 5: c.sy = n * (int64_t)w; c.sx = n; c.sc = 1; break;
    case 1: c.sy = w; c.sx = 1; c.sc = (int64_t)w * h; break;
    case 2: c.sy = n * cw; c.sx = n; c.sc = 1; c.lead = (1 * cw + 16) * n; break;
    case 3: case 6: c.sy = cw; c.sx = 1; c.sc = cw * ch; c.lead = 1 * cw + 16; break;
    case 7: c.sy = n * (int64_t)w + 1; c.sx = n; c.sc = 1; break;
    default: c.sy = n; c.sx = n * (int64_t)h; c.sc = 1; break;
  }
  if (lay.kind == 5 || lay.kind == 6) c.lead += 1;
  c.count = (size_t)(c.lead + (int64_t)(h - 1) * c.sy + (int64_t)(w - 1) * c.sx + (n - 1) * c.sc + 1);
  return c;
}

template <class T>
uint32_t bits_of(T v) {
  uint32_t u = 0;
  memcpy(&u, &v, sizeof(T));
  return u;
}

// One plane of a destination against `want` (w * h floats), marking its elements.
template <class T>
int check_plane(const T* mem, const Canvas& cv, int c, int w, int h, const std::vector<float>& want, std::vector<uint8_t>* is_image, const char* what) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)(cv.lead + y * cv.sy + x * cv.sx + c * cv.sc);
      (*is_image)[i] = 1;
      T e;
      gz::emit_map_value(want[(size_t)y * w + x], &e);
      if (bits_of(mem[i]) != bits_of(e)) {
        printf("MISMATCH %s %dx%d plane %d at (%d, %d): %08x, expected %08x\n", what, w, h, c, y, x, bits_of(mem[i]), bits_of(e));
        return 1;
      }
    }
  return 0;
}

template <class T>
int check_rest(const T* mem, const Canvas& cv, const std::vector<uint8_t>& is_image, const char* what) {
  T sentinel;
  memset(&sentinel, 0xEE, sizeof(T));
  for (size_t i = 0; i < cv.count; ++i)
    if (!is_image[i] && bits_of(mem[i]) != bits_of(sentinel)) {
      printf("TOUCHED %s: element %zu outside the image is %08x\n", what, i, bits_of(mem[i]));
      return 1;
    }
  return 0;
}

template <class T>
int run_case(const Layout& lay, int w, int h, int src_lead, const double* luts, long* cases) {
  const size_t n = (size_t)w * h;
  float* planes[3];
  const float* src[3];
  uint64_t s = 88172645463325252ull + (uint64_t)w * 131 + (uint64_t)h;
  for (int k = 0; k < 3; ++k) {
    // malloc returns 16-byte aligned memory, so `lead` and `src_lead` alone decide which paths the kernel may take
    planes[k] = (float*)malloc(sizeof(float) * (n + src_lead));
    if (!planes[k]) return 2;
    for (size_t i = 0; i < n; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      // blurred sums of absolute differences: 0 .. 2.6, a few far larger, whose table position lies past the table's end
      planes[k][src_lead + i] = (s >> 60) == 0 ? 40.0f : (float)((s >> 33) % 100000) * 2.6e-5f;
    }
    src[k] = planes[k] + src_lead;
  }
  std::vector<float> want[6], wanty(n);
  for (auto& v : want) v.resize(n);
  for (size_t i = 0; i < n; ++i) {
    double p0, p1;
    gz::mask_p0p1(src[0][i], src[1][i], src[2][i], &p0, &p1);
    const double my = gz::interp_lut512(luts + 512, p1), mdcy = gz::interp_lut512(luts + 1536, p1);
    want[0][i] = (float)gz::interp_lut512(luts, p0);
    want[1][i] = (float)my;
    want[2][i] = (float)(0.086624184478 * my);
    want[3][i] = (float)gz::interp_lut512(luts + 1024, p0);
    want[4][i] = (float)mdcy;
    want[5][i] = (float)(21.6804277046 * mdcy);
  }
  int bad = 0;
  const Canvas cv = canvas_of(lay, w, h, 3), cq = canvas_of(lay, w, h, 1);
  for (int mode : {(int)gz::kEmitMask, (int)gz::kEmitMaskDc, (int)gz::kEmitMaskBoth, (int)gz::kEmitMaskY}) {
    const Canvas& c = mode == gz::kEmitMaskY ? cq : cv;
    T* m = (T*)malloc(c.count * sizeof(T));
    T* d = (T*)malloc(c.count * sizeof(T));
    if (!m || !d) return 2;
    memset(m, 0xEE, c.count * sizeof(T));
    memset(d, 0xEE, c.count * sizeof(T));
    gz::EmitMaskArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.mask_x_blur = mode == gz::kEmitMaskY ? nullptr : src[0];   // (the Y-only mode must not read it)
    a.mask_y_blur1 = src[1]; a.mask_y_blur2 = src[2];
    a.luts = luts;
    if (mode != gz::kEmitMaskDc) a.mask = {m + c.lead, c.sy, c.sx, c.sc};
    if (mode & gz::kEmitMaskDc) a.dc = {d + c.lead, c.sy, c.sx, c.sc};
    switch (mode) {
      case gz::kEmitMask: gz::launch_emit_mask<T, gz::kEmitMask>((hipStream_t) nullptr, a, w, h, w); break;
      case gz::kEmitMaskDc: gz::launch_emit_mask<T, gz::kEmitMaskDc>((hipStream_t) nullptr, a, w, h, w); break;
      case gz::kEmitMaskBoth: gz::launch_emit_mask<T, gz::kEmitMaskBoth>((hipStream_t) nullptr, a, w, h, w); break;
      default: gz::launch_emit_mask<T, gz::kEmitMaskY>((hipStream_t) nullptr, a, w, h, w); break;
    }
    std::vector<uint8_t> im(c.count, 0), id(c.count, 0);
    if (mode == gz::kEmitMaskY) {
      bad |= check_plane(m, c, 0, w, h, want[1], &im, lay.name);
    } else {
      for (int k = 0; k < 3 && !bad; ++k) {
        if (mode & gz::kEmitMask) bad |= check_plane(m, c, k, w, h, want[k], &im, lay.name);
        if (mode & gz::kEmitMaskDc) bad |= check_plane(d, c, k, w, h, want[3 + k], &id, lay.name);
      }
    }
    if (!bad) bad |= check_rest(m, c, im, lay.name) | check_rest(d, c, id, lay.name);
    free(m);
    free(d);
    ++*cases;
  }
  for (float* p : planes) free(p);
  return bad;
}

}  // namespace

int main() {
  // the kernel's table, malloc'ed to its exact size: four rising curves
  double* luts = (double*)malloc(sizeof(double) * 2048);
  for (int t = 0; t < 4; ++t)
    for (int i = 0; i < 512; ++i) luts[t * 512 + i] = (t + 1) * 0.01 + 1.0 / (1.0 + 0.37 * i + t);
  const int widths[] = {1, 3, 4, 5, 15, 16, 17, 19, 23, 33, 67}, heights[] = {1, 2, 9};
  long cases = 0;
  int bad = 0;
  for (const Layout& lay : kLayouts)
    for (int w : widths)
      for (int h : heights)
        for (int src_lead = 0; src_lead < 2; ++src_lead) {
          bad |= run_case<float>(lay, w, h, src_lead, luts, &cases);
          bad |= run_case<gz::ingest_f16>(lay, w, h, src_lead, luts, &cases);
          bad |= run_case<gz::ingest_bf16>(lay, w, h, src_lead, luts, &cases);
        }
  free(luts);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all elements as expected, no access outside the buffers");
  return bad;
}
