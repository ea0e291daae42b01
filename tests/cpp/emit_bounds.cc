// TEST ONLY (CPU, host sanitizers): gz_decode_coeffs_device -- the emit kernel k_emit_rgb of gz_kernels_emit.h through
// its launch code -- over every layout, element type and size the tests use, into destinations malloc'ed to EXACTLY the
// last addressed element + 1.  Built with -DGZ_EMU -fsanitize=address,undefined against tests/emu/hip_emu.h: a store of
// the 16-byte path or of a row's tail that leaves [0, (h-1) sy + (w-1) sx + 2 sc] is a heap-buffer-overflow report, a
// misaligned 16-byte access an alignment report; so is any read of the packed image outside its 3 w h bytes.  The
// elements are checked against the rule restated here, and the elements of a crop's canvas that are no part of the
// image against the sentinel they were filled with.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_api.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

// the storage bits of the element of byte b
uint32_t expected_bits(int dtype, uint8_t b) {
  if (dtype == GZ_DT_U8) return b;
  if (dtype == GZ_DT_U16) return (uint32_t)b * 257u;
  volatile float f = (float)b / 255.0f;
  const float g = f;
  uint32_t u;
  memcpy(&u, &g, 4);
  if (dtype == GZ_DT_F32) return u;
  if (dtype == GZ_DT_BF16) return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  // float16, round to nearest even, for 0 and the normal numbers [1 / 255, 1]
  if (u == 0) return 0;
  const uint32_t e = (u >> 23) - 112u, m = u & 0x7fffffu;
  uint32_t h = (e << 10) | (m >> 13);
  const uint32_t rest = m & 0x1fffu;
  if (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ++h;
  return h;
}

struct Layout { const char* name; int kind; };   // 0 HWC, 1 CHW, 2 HWC crop, 3 CHW crop, 4 WHC, 5 HWC + 1, 6 CHW crop + 1
const Layout kLayouts[] = {{"HWC", 0}, {"CHW", 1}, {"HWC crop", 2}, {"CHW crop", 3}, {"WHC", 4}, {"HWC base+1", 5}, {"CHW crop base+1", 6}};

uint32_t load(const void* mem, size_t elem, size_t i) {
  return elem == 1 ? ((const uint8_t*)mem)[i] : elem == 2 ? ((const uint16_t*)mem)[i] : ((const uint32_t*)mem)[i];
}

int run_case(int dtype, const Layout& lay, int w, int h, int factor, long* cases) {
  const size_t elem = dtype == GZ_DT_U8 ? 1 : dtype == GZ_DT_F32 ? 4 : 2;
  int64_t sy, sx, sc;
  const int64_t cw = (w + 16 + 15) / 16 * 16, ch = h + 2;   // the canvas of a crop: rows of a multiple of 16 pixels
  int64_t lead = 0;                                          // elements in front of (0, 0, 0) that belong to the allocation
  switch (lay.kind) {
    case 0: case 5: sy = 3 * (int64_t)w; sx = 3; sc = 1; break;
    case 1: sy = w; sx = 1; sc = (int64_t)w * h; break;
    case 2: sy = 3 * cw; sx = 3; sc = 1; lead = (1 * cw + 16) * 3; break;
    case 3: case 6: sy = cw; sx = 1; sc = cw * ch; lead = 1 * cw + 16; break;
    default: sy = 3; sx = 3 * (int64_t)h; sc = 1; break;
  }
  if (lay.kind == 5 || lay.kind == 6) lead += 1;
  const int64_t last = (int64_t)(h - 1) * sy + (int64_t)(w - 1) * sx + 2 * sc;
  const size_t count = (size_t)(lead + last + 1);
  // malloc returns 16-byte aligned memory, so `lead` alone decides which store path the launch code may take
  void* mem = malloc(count * elem);
  if (!mem) return 2;
  memset(mem, 0xEE, count * elem);
  std::vector<uint8_t> is_image(count, 0);
  const int bw = (w + 7) / 8, bh = (h + 7) / 8, nb = bw * bh;
  const int nbc = ((w + 8 * factor - 1) / (8 * factor)) * ((h + 8 * factor - 1) / (8 * factor));
  std::vector<int16_t> co(((size_t)nb + 2 * (size_t)nbc) * 64, 0);
  uint64_t s = 88172645463325252ull + (uint64_t)w * 131 + (uint64_t)h;
  for (size_t i = 0; i < co.size(); ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const int k = (int)(i & 63);
    co[i] = (k == 0 || (s >> 60) == 0) ? (int16_t)((int)((s >> 33) % 2049) - 1024) : (int16_t)0;
  }
  std::vector<uint8_t> rgb((size_t)3 * w * h, 0);
  gz_device_output out;
  memset(&out, 0, sizeof(out));
  out.struct_size = (int)sizeof(out);
  out.dtype = dtype;
  out.data = (char*)mem + (size_t)lead * elem;
  out.stride_y = sy; out.stride_x = sx; out.stride_c = sc;
  int bad = gz_decode_coeffs(0, co.data(), w, h, factor, rgb.data()) != GZ_OK;
  bad |= gz_decode_coeffs_device(0, co.data(), w, h, factor, &out) != GZ_OK;
  for (int y = 0; y < h && !bad; ++y)
    for (int x = 0; x < w && !bad; ++x)
      for (int c = 0; c < 3; ++c) {
        const size_t i = (size_t)(lead + y * sy + x * sx + c * sc);
        is_image[i] = 1;
        const uint8_t b = rgb[((size_t)y * w + x) * 3 + c];
        if (load(mem, elem, i) != expected_bits(dtype, b)) {
          printf("MISMATCH dtype %d %s %dx%d at (%d, %d, %d): byte %d -> %08x, expected %08x\n", dtype, lay.name, w, h, y, x, c, b,
                 load(mem, elem, i), expected_bits(dtype, b));
          bad = 1;
          break;
        }
      }
  const uint32_t sentinel = elem == 1 ? 0xEEu : elem == 2 ? 0xEEEEu : 0xEEEEEEEEu;
  for (size_t i = 0; i < count && !bad; ++i)
    if (!is_image[i] && load(mem, elem, i) != sentinel) {
      printf("TOUCHED dtype %d %s %dx%d: element %zu outside the image is %08x\n", dtype, lay.name, w, h, i, load(mem, elem, i));
      bad = 1;
    }
  free(mem);
  ++*cases;
  return bad;
}

}  // namespace

int main() {
  const int widths[] = {1, 3, 4, 5, 15, 16, 17, 33, 61, 64, 67}, heights[] = {1, 2, 9};
  long cases = 0;
  int bad = 0;
  for (int dtype = GZ_DT_U8; dtype <= GZ_DT_U16; ++dtype)
    for (const Layout& lay : kLayouts)
      for (int w : widths)
        for (int h : heights) bad |= run_case(dtype, lay, w, h, (w + h) % 2 ? 2 : 1, &cases);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all elements as expected, no store outside the destination");
  return bad;
}
