// TEST ONLY (CPU, host sanitizers): the arithmetic of guetzli_amd/csrc/api/tensor.h -- the extent rule, the
// distinct-addresses rule, the last offset -- and the adapters of the six ABI structs, compiled ALONE: this file includes
// tensor.h and the public header, no HIP, no emulation, no gz_ctx.
//   1. every view of 2, 3 and 4 dimensions with counts in {1, 2, 3} and strides in 0..13, against brute force over its
//      element addresses;  2. the 62-bit boundary at the grid's limits, without an overflow UBSan could see;
//   3. each struct's own rules, one case each.
// Built by tests/test_abi.py with -fsanitize=address,undefined -fno-sanitize-recover=all; its own process.
#include "../../guetzli_amd/csrc/api/tensor.h"
#include "../../include/guetzli_amd.h"

#include <stdio.h>
#include <stdlib.h>

#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

static TensorView make_view(int nd, const int64_t* stride, const int64_t* count) {
  TensorView v;
  static int anchor;
  v.data = &anchor;
  v.dtype = GZ_DT_F32;
  v.nd = nd;
  for (int i = 0; i < nd; ++i) v.dim[i] = {stride[i], count[i]};
  return v;
}

// Every element address of a small view: the largest one, and whether two elements share one.
struct Brute {
  uint64_t last;
  bool duplicate;
};
static Brute brute_force(const TensorView& v) {
  bool seen[256] = {false};
  Brute b = {0, false};
  int64_t idx[4] = {0, 0, 0, 0};
  for (;;) {
    uint64_t at = 0;
    for (int i = 0; i < v.nd; ++i) at += (uint64_t)(idx[i] * v.dim[i].stride);
    EXPECT(at < 256);
    if (seen[at]) b.duplicate = true;
    seen[at] = true;
    if (at > b.last) b.last = at;
    int i = v.nd - 1;
    while (i >= 0 && ++idx[i] == v.dim[i].count) idx[i--] = 0;
    if (i < 0) return b;
  }
}

static long long exhaustive(int nd, long long* refused_without_duplicate) {
  long long views = 0;
  int64_t stride[4] = {0, 0, 0, 0}, count[4] = {1, 1, 1, 1};
  int combos = 1, strides = 1;
  for (int i = 0; i < nd; ++i) { combos *= 3; strides *= 14; }
  for (int cc = 0; cc < combos; ++cc) {
    for (int i = 0, r = cc; i < nd; ++i, r /= 3) count[i] = 1 + r % 3;
    for (int ss = 0; ss < strides; ++ss) {
      for (int i = 0, r = ss; i < nd; ++i, r /= 14) stride[i] = r % 14;
      const TensorView v = make_view(nd, stride, count);
      const Brute b = brute_force(v);
      EXPECT(tensor_extent_ok(v));
      EXPECT(tensor_last(v, nd) == b.last);
      const bool accepted = tensor_distinct(v);
      if (accepted) EXPECT(!b.duplicate);
      if (b.duplicate) EXPECT(!accepted);
      if (!accepted && !b.duplicate) ++*refused_without_duplicate;
      ++views;
    }
  }
  return views;
}

// Every dense layout of nd dimensions with counts in {1, 2, 3} -- each order of the dimensions in memory: HWC, CHW, NHWC,
// NCHW and the rest -- with 0..3 elements of padding behind the innermost rows (a crop of a larger tensor): accepted.
static long long dense_layouts(int nd) {
  long long layouts = 0;
  int order[4] = {0, 1, 2, 3};
  int combos = 1;
  for (int i = 0; i < nd; ++i) combos *= 3;
  do {
    for (int cc = 0; cc < combos; ++cc) {
      int64_t stride[4] = {0, 0, 0, 0}, count[4] = {1, 1, 1, 1};
      for (int i = 0, r = cc; i < nd; ++i, r /= 3) count[i] = 1 + r % 3;
      for (int pad = 0; pad <= 3; ++pad) {
        int64_t step = 1;
        for (int k = 0; k < nd; ++k) {   // order[0] is the innermost dimension
          stride[order[k]] = step;
          step = step * count[order[k]] + (k == 0 ? pad : 0);
        }
        const TensorView v = make_view(nd, stride, count);
        EXPECT(tensor_extent_ok(v));
        EXPECT(tensor_distinct(v));
        const Brute b = brute_force(v);
        EXPECT(!b.duplicate && tensor_last(v, nd) == b.last);
        ++layouts;
      }
    }
  } while (std::next_permutation(order, order + nd));
  return layouts;
}

static void boundary() {
  const uint64_t lim = kTensorLimit;
  EXPECT(lim == 4611686018427387903ull);
  // the grid's limits: n = 21845 images of 65535 x 65535 x 3; per dimension the largest stride whose term fits, all other
  // terms 0 -- and with a count of 4, the stride whose term is the limit itself (3 divides 2^62 - 1)
  const int64_t grid[4] = {21845, 65535, 65535, 3};
  for (int d = 0; d < 4; ++d) {
    for (int exact = 0; exact < 2; ++exact) {
      int64_t count[4] = {grid[0], grid[1], grid[2], grid[3]}, stride[4] = {0, 0, 0, 0};
      if (exact) count[d] = 4;
      const uint64_t steps = (uint64_t)count[d] - 1;
      stride[d] = (int64_t)(lim / steps);
      if (exact) EXPECT((uint64_t)stride[d] * steps == lim);
      TensorView v = make_view(4, stride, count);
      EXPECT(tensor_extent_ok(v));
      EXPECT(tensor_last(v, 4) == (uint64_t)stride[d] * steps && tensor_last(v, 4) <= lim);
      EXPECT(tensor_distinct(v) == true || tensor_distinct(v) == false);   // (no overflow: UBSan would stop here)
      ++stride[d];
      v = make_view(4, stride, count);
      EXPECT(!tensor_extent_ok(v));
      // one more element anywhere else is one too many for the exact stride
      if (exact) {
        --stride[d];
        stride[(d + 1) % 4] = 1;
        EXPECT(!tensor_extent_ok(make_view(4, stride, count)));
      }
    }
  }
  // two terms that each fit: 2^61 + (2^61 - 1) is the limit, 2^61 + 2^61 is beyond it
  for (int a = 0; a < 4; ++a) {
    for (int b = 0; b < 4; ++b) {
      if (a == b) continue;
      int64_t count[4] = {1, 1, 1, 1}, stride[4] = {7, 7, 7, 7};
      count[a] = count[b] = 2;
      stride[a] = (int64_t)1 << 61;
      stride[b] = ((int64_t)1 << 61) - 1;
      EXPECT(tensor_extent_ok(make_view(4, stride, count)));
      EXPECT(tensor_last(make_view(4, stride, count), 4) == lim);
      stride[b] = (int64_t)1 << 61;
      EXPECT(!tensor_extent_ok(make_view(4, stride, count)));
    }
  }
  // INT64_MAX in every position: as a stride (at the grid's counts and at a count of 2), as a count
  for (int d = 0; d < 4; ++d) {
    int64_t count[4] = {grid[0], grid[1], grid[2], grid[3]}, stride[4] = {1, 1, 1, 1};
    stride[d] = INT64_MAX;
    EXPECT(!tensor_extent_ok(make_view(4, stride, count)));
    count[d] = 2;
    EXPECT(!tensor_extent_ok(make_view(4, stride, count)));
    stride[d] = 1;
    count[d] = INT64_MAX;
    EXPECT(!tensor_extent_ok(make_view(4, stride, count)));
  }
  int64_t all_stride[4] = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX}, all_count[4] = {grid[0], grid[1], grid[2], grid[3]};
  EXPECT(!tensor_extent_ok(make_view(4, all_stride, all_count)));
  // a stride below 0 and a dimension without an element are no extent at all
  int64_t s1[2] = {-1, 1}, c1[2] = {4, 4}, s2[2] = {4, 1}, c2[2] = {4, 0};
  EXPECT(!tensor_extent_ok(make_view(2, s1, c1)) && !tensor_extent_ok(make_view(2, s2, c2)));
}

// ---- the adapters ----
static const int W = 5, H = 4, N = 3;
static float g_mem[1024];

static gz_device_pixels good_pixels() {
  gz_device_pixels p;
  memset(&p, 0, sizeof(p));
  p.struct_size = (int)sizeof(p);
  p.dtype = GZ_DT_U8;
  p.data = g_mem;
  p.stride_y = 3 * W; p.stride_x = 3; p.stride_c = 1;
  return p;
}
static gz_device_output good_output() {
  gz_device_output o;
  memset(&o, 0, sizeof(o));
  o.struct_size = (int)sizeof(o);
  o.dtype = GZ_DT_U8;
  o.data = g_mem;
  o.stride_y = 3 * W; o.stride_x = 3; o.stride_c = 1;
  return o;
}
static gz_device_map good_map() {
  gz_device_map m;
  memset(&m, 0, sizeof(m));
  m.struct_size = (int)sizeof(m);
  m.dtype = GZ_DT_F32;
  m.data = g_mem;
  m.stride_y = W; m.stride_x = 1;
  return m;
}
static gz_device_batch good_batch() {
  gz_device_batch b;
  memset(&b, 0, sizeof(b));
  b.struct_size = (int)sizeof(b);
  b.dtype = GZ_DT_U8;
  b.data = g_mem;
  b.stride_n = 3 * W * H; b.stride_y = 3 * W; b.stride_x = 3; b.stride_c = 1;
  return b;
}
static gz_device_map_batch good_map_batch() {
  gz_device_map_batch m;
  memset(&m, 0, sizeof(m));
  m.struct_size = (int)sizeof(m);
  m.dtype = GZ_DT_F32;
  m.data = g_mem;
  m.stride_n = W * H; m.stride_y = W; m.stride_x = 1;
  return m;
}
static gz_device_image good_image() {
  gz_device_image i;
  memset(&i, 0, sizeof(i));
  i.struct_size = (int)sizeof(i);
  i.dtype = GZ_DT_U8;
  i.data = g_mem;
  i.stride_y = 3 * W; i.stride_x = 3; i.stride_c = 1;
  return i;
}
static int check(const gz_device_pixels& p) { return check_device_pixels(&p, W, H); }
static int check(const gz_device_output& p) { return check_device_output(&p, W, H); }
static int check(const gz_device_map& p) { return check_device_map(&p, W, H); }
static int check(const gz_device_batch& p) { return check_device_batch(&p, W, H, N); }
static int check(const gz_device_map_batch& p) { return check_device_map_batch(&p, W, H, N); }
static int check(const gz_device_image& i) {
  gz_device_pixels px;
  if (const int rc = pixels_of_image(&i, &px)) return rc;
  return check_device_pixels(&px, W, H);
}

// What every struct refuses, and the ends of its dtype set: first .. last are taken, the two beside them are not.
template <class S>
static void common_rules(S good, int dtype_first, int dtype_last) {
  EXPECT(check(good) == GZ_OK);
  S s = good;
  s.struct_size += 8;
  EXPECT(check(s) == GZ_E_ARG);
  s = good;
  s.data = nullptr;
  EXPECT(check(s) == GZ_E_ARG);
  s = good;
  s.stride_y = -s.stride_y;
  EXPECT(check(s) == GZ_E_ARG);
  s = good;
  s.stride_x = -1;
  EXPECT(check(s) == GZ_E_ARG);
  for (int dtype = -1; dtype <= 6; ++dtype) {
    s = good;
    s.dtype = dtype;
    EXPECT(check(s) == (dtype >= dtype_first && dtype <= dtype_last ? GZ_OK : GZ_E_ARG));
  }
}

static void adapters() {
  common_rules(good_image(), GZ_DT_U8, GZ_DT_BF16);      // (no GZ_DT_U16: pixels_of_image)
  common_rules(good_pixels(), GZ_DT_U8, GZ_DT_U16);
  common_rules(good_output(), GZ_DT_U8, GZ_DT_U16);
  common_rules(good_map(), GZ_DT_F32, GZ_DT_BF16);
  common_rules(good_batch(), GZ_DT_U8, GZ_DT_BF16);
  common_rules(good_map_batch(), GZ_DT_F32, GZ_DT_BF16);
  EXPECT(check_device_pixels(nullptr, W, H) == GZ_E_ARG && check_device_output(nullptr, W, H) == GZ_E_ARG);
  EXPECT(check_device_map(nullptr, W, H) == GZ_E_ARG && check_device_batch(nullptr, W, H, N) == GZ_E_ARG);
  EXPECT(check_device_map_batch(nullptr, W, H, N) == GZ_E_ARG);
  gz_device_pixels px;
  EXPECT(pixels_of_image(nullptr, &px) == GZ_E_ARG);
  // a stride of 0: an input repeats an element (grey pixels, one image n times), an output may not
  {
    gz_device_pixels p = good_pixels();
    p.stride_c = 0;
    EXPECT(check(p) == GZ_OK);
    gz_device_image i = good_image();
    i.stride_c = 0;
    EXPECT(check(i) == GZ_OK);
    gz_device_batch b = good_batch();
    b.stride_n = 0;
    EXPECT(check(b) == GZ_OK);
    b.stride_c = 0;
    EXPECT(check(b) == GZ_OK);
    gz_device_output o = good_output();
    o.stride_c = 0;
    EXPECT(check(o) == GZ_E_ARG);
    gz_device_map m = good_map();
    m.stride_x = 0;
    EXPECT(check(m) == GZ_E_ARG);
    gz_device_map_batch mb = good_map_batch();
    mb.stride_n = 0;
    EXPECT(check(mb) == GZ_E_ARG);
    EXPECT(check_device_map_batch(&mb, W, H, 1) == GZ_OK);   // (one map: its stride addresses nothing)
    mb = good_map_batch();
    mb.stride_n = W * H - 1;   // the second map's first element on the first one's last
    EXPECT(check(mb) == GZ_E_ARG);
  }
  // the plane sizes the adapters bound themselves (a map batch's are the entry's)
  {
    const gz_device_pixels p = good_pixels();
    const gz_device_output o = good_output();
    const gz_device_map m = good_map();
    const gz_device_batch b = good_batch();
    for (const int bad : {0, -1, 1 << 16}) {
      EXPECT(check_device_pixels(&p, bad, H) == GZ_E_ARG && check_device_pixels(&p, W, bad) == GZ_E_ARG);
      EXPECT(check_device_output(&o, bad, H) == GZ_E_ARG && check_device_output(&o, W, bad) == GZ_E_ARG);
      EXPECT(check_device_map(&m, bad, H) == GZ_E_ARG && check_device_map(&m, W, bad) == GZ_E_ARG);
      EXPECT(check_device_batch(&b, bad, H, N) == GZ_E_ARG && check_device_batch(&b, W, bad, N) == GZ_E_ARG);
    }
    EXPECT(check_device_pixels(&p, 65535, 1) == GZ_OK);
  }
  // alpha: data's extent without the channel term, whatever the channel stride
  {
    gz_device_pixels p = good_pixels();
    p.stride_y = 1000; p.stride_x = 4; p.stride_c = 100000;
    p.alpha = g_mem + 3;
    const TensorView v = tensor_view(&p, W, H);
    EXPECT(v.alpha == p.alpha && v.alpha_nd == 2 && v.nd == 3);
    EXPECT(tensor_last(v, v.alpha_nd) == (uint64_t)(1000 * (H - 1) + 4 * (W - 1)));
    EXPECT(tensor_last(v, v.nd) == tensor_last(v, v.alpha_nd) + 200000);
    // ... and both in 62 bits: a channel term that does not fit is refused although alpha's extent would
    p.stride_c = (int64_t)1 << 61;
    EXPECT(check(p) == GZ_E_ARG);
    p.stride_c = ((int64_t)1 << 61) - 1 - (1000 * (H - 1) + 4 * (W - 1) + 1) / 2;
    EXPECT(check(p) == GZ_OK);
  }
  // one image of a batch, one plane of an output: an offset and a dimension less
  {
    gz_device_batch b = good_batch();
    b.dtype = GZ_DT_F16;
    const TensorView one = tensor_select(tensor_view(&b, W, H, N), 0, 2);
    EXPECT(one.nd == 3 && one.data == (const char*)g_mem + 2 * b.stride_n * 2 && one.stream == b.producer_stream);
    EXPECT(one.dim[0].stride == b.stride_y && one.dim[0].count == H && one.dim[1].stride == b.stride_x && one.dim[1].count == W);
    EXPECT(one.dim[2].stride == b.stride_c && one.dim[2].count == 3);
    gz_device_output o = good_output();
    o.dtype = GZ_DT_F32;
    o.stride_c = 7;
    const TensorView plane = tensor_select(tensor_view(&o, W, H), 2, 2);
    EXPECT(plane.nd == 2 && plane.data == (const char*)g_mem + 2 * 7 * 4);
    EXPECT(plane.dim[0].stride == o.stride_y && plane.dim[0].count == H && plane.dim[1].stride == o.stride_x && plane.dim[1].count == W);
    gz_device_pixels p = good_pixels();
    p.alpha = g_mem + 3;
    const TensorView row = tensor_select(tensor_view(&p, W, H), 0, 1);
    EXPECT(row.nd == 2 && row.alpha_nd == 1 && row.alpha == (const char*)p.alpha + 3 * W && row.data == (const char*)g_mem + 3 * W);
  }
}

int main() {
  long long refused = 0, views = 0, layouts = 0;
  for (int nd = 2; nd <= 4; ++nd) {
    views += exhaustive(nd, &refused);
    layouts += dense_layouts(nd);
  }
  boundary();
  adapters();
  printf("%lld views against brute force; %lld of them without a duplicate address are refused (the rule is sufficient, not necessary)\n",
         views, refused);
  printf("%lld dense and padded layouts accepted\n", layouts);
  printf("tensor arguments: all as expected\n");
  return 0;
}
