// TEST ONLY (CPU, host sanitizers): gz_pack_rgb_device -- the ingest kernel k_ingest_rgb of gz_kernels_ingest.h through
// its launch code -- over every layout, element type and width the tests use, on sources malloc'ed to EXACTLY the last
// addressed element + 1.  Built with -DGZ_EMU -fsanitize=address,undefined against tests/emu/hip_emu.h: a read of the
// 16-byte path or of a row's tail that leaves [0, (h-1) sy + (w-1) sx + 2 sc] is a heap-buffer-overflow report, a
// misaligned 16-byte access an alignment report.  The bytes are checked against the rule restated here as well.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_api.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 32);
  }
};

// a finite float16: (1024 + m) * 2^(e - 25), or m * 2^-24 for a subnormal -- exact in float
float widen_f16(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 0x3ff;
  const float mag = std::ldexp((float)(e ? 1024 + m : m), (e ? e : 1) - 25);
  return (h & 0x8000) ? -mag : mag;
}

// the expected byte of the element whose storage is `bits`
uint8_t expected_byte(int dtype, uint32_t bits) {
  if (dtype == GZ_DT_U8) return (uint8_t)bits;
  float x;
  if (dtype == GZ_DT_F32) {
    memcpy(&x, &bits, 4);
  } else if (dtype == GZ_DT_BF16) {
    const uint32_t u = bits << 16;
    memcpy(&x, &u, 4);
  } else {
    const uint16_t h = (uint16_t)bits;
    if (((h >> 10) & 31) == 31) {
      const uint32_t u = ((uint32_t)(h & 0x8000) << 16) | 0x7f800000u | ((uint32_t)(h & 0x3ff) << 13);
      memcpy(&x, &u, 4);
    } else {
      x = widen_f16(h);
    }
  }
  volatile float v = x * 255.0f;
  if (std::isnan(v)) return 0;
  if (v < 0.0f) return 0;
  if (v > 255.0f) return 255;
  return (uint8_t)std::nearbyint((float)v);
}

// storage bits of a random element: floats mostly in [0, 1], some bit patterns of every kind
uint32_t random_bits(int dtype, Rng* r) {
  const uint32_t u = r->next();
  if (dtype == GZ_DT_U8) return u & 0xff;
  if ((u & 7) == 0) return dtype == GZ_DT_F32 ? r->next() : r->next() & 0xffff;
  const float x = (float)(r->next() & 0xffff) / 65535.0f;
  uint32_t f;
  memcpy(&f, &x, 4);
  if (dtype == GZ_DT_F32) return f;
  if (dtype == GZ_DT_BF16) return f >> 16;
  // f32 in [0, 1] -> f16 by truncation (any f16 will do)
  const int e = (int)((f >> 23) & 0xff) - 127 + 15;
  if (e <= 0) return 0;
  return ((uint32_t)e << 10) | ((f >> 13) & 0x3ff);
}

struct Layout { const char* name; int kind; };   // 0 HWC, 1 CHW, 2 HWC crop, 3 CHW crop, 4 grey, 5 HWC + 1, 6 CHW crop + 1
const Layout kLayouts[] = {{"HWC", 0}, {"CHW", 1}, {"HWC crop", 2}, {"CHW crop", 3}, {"grey", 4}, {"HWC base+1", 5}, {"CHW crop base+1", 6}};

int run_case(int dtype, const Layout& lay, int w, int h, Rng* rng, long* cases) {
  const size_t elem = dtype == GZ_DT_U8 ? 1 : dtype == GZ_DT_F32 ? 4 : 2;
  int64_t sy, sx, sc;
  const int64_t cw = (w + 16 + 15) / 16 * 16, ch = h + 2;   // the canvas of a crop: rows of a multiple of 16 pixels
  int64_t lead = 0;                                          // elements in front of (0, 0, 0) that belong to the allocation
  switch (lay.kind) {
    case 0: case 5: sy = 3 * (int64_t)w; sx = 3; sc = 1; break;
    case 1: sy = w; sx = 1; sc = (int64_t)w * h; break;
    case 2: sy = 3 * cw; sx = 3; sc = 1; lead = (1 * cw + 16) * 3; break;
    case 3: case 6: sy = cw; sx = 1; sc = cw * ch; lead = 1 * cw + 16; break;
    default: sy = w; sx = 1; sc = 0; break;
  }
  if (lay.kind == 5 || lay.kind == 6) lead += 1;
  const int64_t last = (int64_t)(h - 1) * sy + (int64_t)(w - 1) * sx + 2 * sc;
  const size_t count = (size_t)(lead + last + 1);
  // malloc returns 16-byte aligned memory, so `lead` alone decides which read path the launch code may take
  void* mem = malloc(count * elem);
  if (!mem) return 2;
  for (size_t i = 0; i < count; ++i) {
    const uint32_t b = random_bits(dtype, rng);
    if (elem == 1) ((uint8_t*)mem)[i] = (uint8_t)b;
    else if (elem == 2) ((uint16_t*)mem)[i] = (uint16_t)b;
    else ((uint32_t*)mem)[i] = b;
  }
  gz_device_image img;
  memset(&img, 0, sizeof(img));
  img.struct_size = (int)sizeof(img);
  img.dtype = dtype;
  img.data = (const char*)mem + (size_t)lead * elem;
  img.stride_y = sy; img.stride_x = sx; img.stride_c = sc;
  std::vector<uint8_t> out((size_t)3 * w * h, 0xEE);
  const int rc = gz_pack_rgb_device(0, &img, w, h, out.data());
  int bad = rc != GZ_OK;
  for (int y = 0; y < h && !bad; ++y)
    for (int x = 0; x < w && !bad; ++x)
      for (int c = 0; c < 3; ++c) {
        const size_t i = (size_t)(lead + y * sy + x * sx + c * sc);
        const uint32_t b = elem == 1 ? ((uint8_t*)mem)[i] : elem == 2 ? ((uint16_t*)mem)[i] : ((uint32_t*)mem)[i];
        if (out[((size_t)y * w + x) * 3 + c] != expected_byte(dtype, b)) {
          printf("MISMATCH dtype %d %s %dx%d at (%d, %d, %d): bits %08x -> %d, expected %d\n", dtype, lay.name, w, h, y, x, c, b,
                 out[((size_t)y * w + x) * 3 + c], expected_byte(dtype, b));
          bad = 1;
          break;
        }
      }
  free(mem);
  ++*cases;
  return bad;
}

}  // namespace

int main() {
  const int widths[] = {1, 3, 4, 5, 15, 16, 17, 33, 61, 64, 67}, heights[] = {1, 2, 9};
  Rng rng{20261019};
  long cases = 0;
  int bad = 0;
  for (int dtype = GZ_DT_U8; dtype <= GZ_DT_BF16; ++dtype)
    for (const Layout& lay : kLayouts)
      for (int w : widths)
        for (int h : heights) bad |= run_case(dtype, lay, w, h, &rng, &cases);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all bytes as expected, no read outside the source");
  return bad;
}
