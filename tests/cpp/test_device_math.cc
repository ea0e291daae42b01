// TEST INFRASTRUCTURE.  The per-pixel functions of guetzli_amd/csrc/gz_math.h (and quant_div of the
// entropy kernels) evaluated ON THE DEVICE through gz_probe_math, against the plain statement
// sequences of the reference evaluated here on the host: malta_diff_plain, the Clenshaw recursion
// with real divisions, C++'s / on ints.  What is proven on the host alone elsewhere
// (verify_malta_diff.cc, verify_opsin_divisions.cc, verify_quant_div.cc: the cheaper forms equal the
// plain ones given an emulated reciprocal) is checked here with the device's own v_rcp_f32, fused
// multiply-adds, denormal mode and wavefront-uniform branch.
//
//   test_device_math <libguetzli_amd*.so> [sweep stride, default 1]
//
// Build: g++ -O2 -std=c++17 -ffp-contract=off -DGZ_EMU -I guetzli_amd/csrc -I tests/emu
//        tests/cpp/test_device_math.cc -o test_device_math -ldl
//
// Inputs per function: uniform random values; values within +-2 ulp of every threshold (0.55 |a|,
// 1.05 |a|, 0.4 |a|, |a|, the clamps, the cutoffs, the ends of the table); +-0, denormals, 2^+-100,
// +-inf and NaN.  Consecutive groups of 64 elements (a wavefront) mix elements of malta_diff's rare
// path (|a| + |b| == 0 or outside [2^-100, 2^100]) with ordinary ones.  Results are compared bit for
// bit; two NaNs count as equal whatever their sign and payload (x86 and gfx950 differ in the NaN an
// invalid operation produces, and nothing in the chain looks at it).
// interp_lut512 indexes a table with its argument: it gets finite arguments below 2^31 only.
//
// The sweep: gz_probe_div2_sweep compares div2_shared with the device's IEEE division for the twelve
// production numerators and every stride-th float denominator of [2^-40, 2^40); a sample of its
// quotients is compared here with the host's division.
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "gz_common.h"
#include "gz_math.h"
#include "../../include/guetzli_amd.h"

using gz::MaltaNorm;

static uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float float_of(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
static uint64_t bits_of(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static float nudge(float x, int ulps) { return float_of(bits_of(x) + (uint32_t)ulps); }
static bool same(float a, float b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }
static bool same(double a, double b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }

static decltype(&gz_probe_math) g_probe;
static int g_failures = 0;
static std::mt19937_64 g_rng(20261017);

static double urand() { return (double)(g_rng() >> 11) / 9007199254740992.0; }          // [0, 1)
static float frand(double lo, double hi) { return (float)(lo + (hi - lo) * urand()); }
static float logrand(int e_lo, int e_hi) {   // +-2^[e_lo, e_hi), log-uniform
  const double m = ldexp(1.0 + urand(), e_lo + (int)(g_rng() % (uint64_t)(e_hi - e_lo)));
  return (float)((g_rng() & 1) ? -m : m);
}

static const float kInf = __builtin_inff();
static const float kSpecials[] = {0.0f,     -0.0f,     1e-45f,   -1e-45f,        1e-39f,         -1e-40f,
                                  0x1p-126f, 0x1p-100f, -0x1p-100f, 0x1p100f,     -0x1p100f,      0x1.fffffep127f,
                                  kInf,      -kInf,     __builtin_nanf(""), 1.0f, -1.0f,          0x1p-101f,
                                  0x1p101f,  0x1p41f,   85.7047444518f,     78.8223237675f, 5.8907152736f};
static const int kNumSpecials = (int)(sizeof(kSpecials) / sizeof(kSpecials[0]));

// ---------------------------------------------------------------- the plain forms --
// MaltaNorm as api/plans.h builds it (MaltaDiffMapImpl, butteraugli.cc:1468-1476)
static MaltaNorm norm_of(bool lf, double w_0gt1, double w_0lt1, double norm1) {
  const double len = 3.75;
  const double mulli = lf ? 0.405371989604 : 0.354191303559;
  const float kWeight0 = 0.5;
  const float kWeight1 = 0.33;
  const double w_pre0gt1 = mulli * sqrt(kWeight0 * w_0gt1) / (len * 2 + 1);
  const double w_pre0lt1 = mulli * sqrt(kWeight1 * w_0lt1) / (len * 2 + 1);
  MaltaNorm n;
  n.norm2_0gt1 = w_pre0gt1 * norm1;
  n.norm2_0lt1 = w_pre0lt1 * norm1;
  n.norm1f = static_cast<float>(norm1);
  auto mid = [](float x) { return x >= 0x1p-40f && x <= 0x1p40f; };
  n.fast_div = mid(n.norm2_0gt1) && mid(n.norm2_0lt1) && n.norm1f >= 0x1p-40f && n.norm1f <= 0x1p39f ? 1 : 0;
  return n;
}
// GammaPolynomial (butteraugli.h:548-615) as written: real divisions, the full recursion
static double gamma_plain(double v) {
  const double kMin = 0.971783, kMax = 590.188894;
  const double x01 = (v - kMin) / (kMax - kMin);
  const double xc = 2.0 * x01 - 1.0;
  const double yp = gz::clenshaw6_plain(xc, 98.7821300963361, 164.273222212631, 92.948112871376,
                                        33.8165311212688, 6.91626704983562, 0.556380877028234);
  const double yq = gz::clenshaw6_plain(xc, 1, 1.64339473427892, 0.89392405219969, 0.298947051776379,
                                        0.0507146002577288, 0.00226495093949756);
  if (yq == 0.0) return 0.0;
  return static_cast<float>(yp / yq);
}
// The remaining per-pixel statements as the reference writes them (butteraugli.cc), restated here so
// that the expected values do not come from the header under test.
static float plain_remove_range(float w, float x) { return x > w ? x - w : x < -w ? x + w : 0; }      // :369
static float plain_amplify_range(float w, float x) { return x > w ? x + w : x < -w ? x - w : 2.0f * x; }   // :374
static float plain_maximum_clamp(float v, float maxval) {   // :432-444
  static const double kMul = 0.688059627878;
  if (v >= maxval) {
    v -= maxval;
    v *= kMul;
    v += maxval;
  } else if (v < -maxval) {
    v += maxval;
    v *= kMul;
    v -= maxval;
  }
  return v;
}
static float plain_suppress_bright(float hf, float brightness, float mul, float reg) {   // :420-430
  float scaler = mul * reg / (reg + brightness);
  return scaler * hf;
}
static float plain_suppress_x_by_y(float xv, float yv) {   // :470-487
  static const double suppress = 2.96534974403, s = 0.745954517135;
  const double xval = xv, yval = yv;
  const double scaler = s + (suppress * (1.0 - s)) / (suppress + yval * yval);
  return scaler * xval;
}
static void plain_lf_to_vals(float x, float y, float b_arg, float* o) {   // :382-399
  const float xmul = 5.57547552483, ymul = 1.20828034498, bmul = 6.08319517575;
  const float y_to_b_mul = -0.628811683685;
  const float b = b_arg + y_to_b_mul * y;
  o[2] = b * bmul;
  o[0] = x * xmul;
  o[1] = y * ymul;
}
static float plain_l2diff(float acc, float a, float b, double w) {   // :654-668
  double diff = a - b;
  acc += w * diff * diff;
  return acc;
}
static float plain_l2diff_asym(float out, float a, float b, double w_0gt1, double w_0lt1) {   // :672-714
  double diff = a - b;
  out += w_0gt1 * diff * diff;
  const double fabs0 = fabs(a);
  const double too_small = 0.4 * fabs0;
  const double too_big = 1.0 * fabs0;
  if (a < 0) {
    if (b > -too_small) {
      double v = b + too_small;
      out += w_0lt1 * v * v;
    } else if (b < -too_big) {
      double v = -b - too_big;
      out += w_0lt1 * v * v;
    }
  } else {
    if (b < too_small) {
      double v = too_small - b;
      out += w_0lt1 * v * v;
    } else if (b > too_big) {
      double v = b - too_big;
      out += w_0lt1 * v * v;
    }
  }
  return out;
}
static float plain_same_noise_pre(float a, float b) {   // :631-641
  const double maxclamp = 85.7047444518;
  double v0 = fabs(a);
  double v1 = fabs(b);
  if (v0 > maxclamp) v0 = maxclamp;
  if (v1 > maxclamp) v1 = maxclamp;
  return v0 - v1;
}
static float plain_diff_from_sups(float s0, float s1) {   // DiffPrecompute, :1723-1733
  double sup0 = s0, sup1 = s1;
  static const double mul0 = 0.918416534734;
  float v = mul0 * std::min(sup0, sup1);
  static const double cutoff = 55.0184555849;
  if (v >= cutoff) v = cutoff;
  return v;
}
static double plain_interp(const double* a, int size, double ix) {   // InterpolateClampNegative, :236-251
  if (ix < 0) ix = 0;
  const int baseix = static_cast<int>(ix);
  if (baseix >= size - 1) return a[size - 1];
  const double mix = ix - baseix;
  return a[baseix] + mix * (a[baseix + 1] - a[baseix]);
}
// OpsinAbsorbance<float> (butteraugli.h:498-534)
static void plain_absorbance(float r, float g, float b, float* out) {
  const float m0 = 0.254462330846, m1 = 0.488238255095, m2 = 0.0635278003854, m3 = 1.01681026909;
  const float m4 = 0.195214015766, m5 = 0.568019861857, m6 = 0.0860755536007, m7 = 1.1510118369;
  const float m8 = 0.07374607900105684, m9 = 0.06142425304154509, m10 = 0.24416850520714256, m11 = 1.20481945273;
  out[0] = m0 * r + m1 * g + m2 * b + m3;
  out[1] = m4 * r + m5 * g + m6 * b + m7;
  out[2] = m8 * r + m9 * g + m10 * b + m11;
}

// OpsinDynamicsImage's pixel (butteraugli.cc:337-363): the sensitivity as a double quotient
static void opsin_plain(const float* bl, const float* px, float* out) {
  float pre[3], cur[3];
  plain_absorbance(bl[0], bl[1], bl[2], pre);
  plain_absorbance(px[0], px[1], px[2], cur);
  for (int c = 0; c < 3; ++c) {
    const float sens = (float)(gamma_plain((double)pre[c]) / (double)pre[c]);
    cur[c] *= sens;
  }
  out[0] = cur[0] - cur[1];
  out[1] = cur[0] + cur[1];
  out[2] = cur[2];
}

// ------------------------------------------------------------------------ inputs --
struct Pairs { std::vector<float> a, b; void add(float x, float y) { a.push_back(x); b.push_back(y); } };

// (a, b) pairs for the two-sample functions: thresholds are ratios b / a
static Pairs sample_pairs(const std::vector<double>& ratios, int nrandom) {
  Pairs p;
  for (int i = 0; i < nrandom; ++i) {   // band-like: both within a few decades
    const float a = logrand(-14, 14);
    p.add(a, (float)(a * (1.0 + (2.0 * urand() - 1.0) * 1.2)));
  }
  for (int i = 0; i < nrandom / 4; ++i) p.add(logrand(-30, 30), logrand(-30, 30));
  for (int rep = 0; rep < 40; ++rep)    // b = a * ratio, nudged
    for (double r : ratios)
      for (int u = -2; u <= 2; ++u) {
        const float a = rep < 4 ? kSpecials[4 * rep + 3] : logrand(-20, 20);
        if (a != a || a * 0.0f != 0.0f) continue;
        p.add(a, nudge((float)((double)a * r), u));
      }
  for (int i = 0; i < kNumSpecials; ++i)
    for (int j = 0; j < kNumSpecials; ++j) p.add(kSpecials[i], kSpecials[j]);
  // wavefronts that mix the rare path with ordinary elements: a second copy with every fourth
  // element one of the zero / out-of-range pairs, and a third with every second
  const float rare[][2] = {{0.0f, 0.0f}, {-0.0f, 0.0f}, {0.0f, -0.0f}, {-0.0f, -0.0f}, {0x1p-101f, 0.0f},
                           {0x1p100f, 0x1p100f}, {0x1p-110f, -0x1p-120f}, {-0x1p101f, 1.0f}};
  const size_t n = p.a.size();
  for (int every : {4, 2})
    for (size_t i = 0; i < n; ++i) {
      if (i % every == 1) p.add(rare[(i / every) % 8][0], rare[(i / every) % 8][1]);
      else p.add(p.a[i], p.b[i]);
    }
  while (p.a.size() % 64) p.add(0.0f, 0.0f);
  return p;
}
// single values around +-t for every threshold t, random values and the specials
static std::vector<float> sample_values(const std::vector<float>& thresholds, int nrandom, double lo, double hi) {
  std::vector<float> v;
  for (int i = 0; i < nrandom; ++i) v.push_back(frand(lo, hi));
  for (int i = 0; i < nrandom / 4; ++i) v.push_back(logrand(-30, 30));
  for (float t : thresholds)
    for (int u = -2; u <= 2; ++u) { v.push_back(nudge(t, u)); v.push_back(-nudge(t, u)); }
  for (int i = 0; i < kNumSpecials; ++i) v.push_back(kSpecials[i]);
  return v;
}

// ---------------------------------------------------------------------- checking --
static void report(const char* what, size_t n, size_t bad, const std::string& first) {
  printf("%-28s %9zu elements, %zu mismatches\n", what, n, bad);
  if (bad) {
    fprintf(stderr, "%s: first mismatches:\n%s", what, first.c_str());
    ++g_failures;
  }
}
static void run(int op, int n, const void* a, const void* b, const void* c, const std::vector<double>& p, void* out) {
  const int rc = g_probe(0, op, n, a, b, c, p.empty() ? nullptr : p.data(), (int)p.size(), out);
  if (rc != GZ_OK) { fprintf(stderr, "gz_probe_math(op %d): %d\n", op, rc); exit(2); }
}
// device floats against expected floats, `outs` outputs per element
static void check(const char* what, int n, int outs, const std::vector<float>& got, const std::vector<float>& want,
                  const float* a, const float* b, const float* c) {
  size_t bad = 0;
  std::string first;
  for (int k = 0; k < outs; ++k)
    for (int i = 0; i < n; ++i)
      if (!same(got[(size_t)k * n + i], want[(size_t)k * n + i])) {
        if (bad++ < 5) {
          char buf[400];
          snprintf(buf, sizeof(buf), "  [%d] output %d: a=%a b=%a c=%a (group of 64: %d): device %a (%08x), host %a (%08x)\n", i, k,
                   a ? a[i] : 0.0f, b ? b[i] : 0.0f, c ? c[i] : 0.0f, i / 64, got[(size_t)k * n + i],
                   bits_of(got[(size_t)k * n + i]), want[(size_t)k * n + i], bits_of(want[(size_t)k * n + i]));
          first += buf;
        }
      }
  report(what, (size_t)n * outs, bad, first);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: test_device_math <library> [sweep stride]\n"); return 2; }
  const unsigned stride = argc > 2 ? (unsigned)strtoul(argv[2], nullptr, 10) : 1u;
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 2; }
  g_probe = (decltype(&gz_probe_math))dlsym(lib, "gz_probe_math");
  auto sweep = (decltype(&gz_probe_div2_sweep))dlsym(lib, "gz_probe_div2_sweep");
  if (!g_probe || !sweep) { fprintf(stderr, "gz_probe_math / gz_probe_div2_sweep missing\n"); return 2; }

  const float asym = 0.8f, sq = sqrtf(asym);
  std::vector<MaltaNorm> norms = {
      norm_of(false, 5.1409625726 * asym, 5.1409625726 / asym, 58.5001247061),
      norm_of(true, 153.671655716 * sq, 153.671655716 / sq, 83150785.9592),
      norm_of(true, 6841.81248144, 6841.81248144, 0.0135134962487),
      norm_of(false, 4.91743441556 * asym, 4.91743441556 / asym, 687196.39002),
      norm_of(true, 668.358918152 * sq, 668.358918152 / sq, 0.882954368025),
      norm_of(true, 813.901703816, 813.901703816, 16792.9322251)};
  for (int k = 0; k < 6; ++k)
    if (!norms[k].fast_div) { fprintf(stderr, "production norm %d without fast_div\n", k); return 1; }
  norms.push_back(norms[0]);
  norms.back().fast_div = 0;                                             // the plain divisions by choice ...
  norms.push_back(norm_of(true, 813.901703816, 813.901703816, 0x1p45));  // ... and by the host's rule
  if (norms.back().fast_div) { fprintf(stderr, "norm1 = 2^45 should not allow the shared reciprocal\n"); return 1; }

  // ---- malta_diff: the device's fast form and its plain form against the host's plain form ----
  {
    const Pairs p = sample_pairs({0.55, 1.05, -0.55, -1.05, 1.0, -1.0, 0.0}, 60000);
    const int n = (int)p.a.size();
    size_t rare = 0, mixed_groups = 0;
    for (int g = 0; g < n / 64; ++g) {
      int r = 0;
      for (int i = 64 * g; i < 64 * g + 64; ++i) {
        const float s = fabsf(p.a[i]) + fabsf(p.b[i]);
        r += !(s >= 0x1p-100f && s <= 0x1p100f);
      }
      rare += r;
      mixed_groups += r > 0 && r < 64;
    }
    printf("malta_diff inputs: %d pairs, %zu on the rare path, %zu of %d groups of 64 mix both\n", n, rare,
           mixed_groups, n / 64);
    if (mixed_groups < 100) { fprintf(stderr, "too few mixed wavefronts\n"); return 1; }
    for (size_t k = 0; k < norms.size(); ++k) {
      const MaltaNorm& nm = norms[k];
      std::vector<float> want(n), got(n), host_fast(n);
      for (int i = 0; i < n; ++i) {
        want[i] = gz::malta_diff_plain(p.a[i], p.b[i], nm);
        host_fast[i] = gz::malta_diff(p.a[i], p.b[i], nm);
      }
      const std::vector<double> pp = {nm.norm2_0gt1, nm.norm2_0lt1, nm.norm1f, (double)nm.fast_div};
      char what[64];
      snprintf(what, sizeof(what), "malta_diff norm %zu (host)", k);
      check(what, n, 1, host_fast, want, p.a.data(), p.b.data(), nullptr);
      run(GZ_MATH_MALTA_DIFF, n, p.a.data(), p.b.data(), nullptr, pp, got.data());
      snprintf(what, sizeof(what), "malta_diff norm %zu", k);
      check(what, n, 1, got, want, p.a.data(), p.b.data(), nullptr);
      run(GZ_MATH_MALTA_DIFF_PLAIN, n, p.a.data(), p.b.data(), nullptr, pp, got.data());
      snprintf(what, sizeof(what), "malta_diff_plain norm %zu", k);
      check(what, n, 1, got, want, p.a.data(), p.b.data(), nullptr);
    }
  }
  // An emulation build's reciprocal is 1.0f / d, correctly rounded, where v_rcp_f32 is accurate to 1 ulp: there the
  // division checks run with the estimate off by -1, 0 and +1 ulp (gz_emu_set_rcp_ulps; a gfx950 library has no such
  // hook and runs them once, on its own reciprocal).
  auto set_ulps = (void (*)(int))dlsym(lib, "gz_emu_set_rcp_ulps");
  for (int ulps = set_ulps ? -1 : 0; ulps <= (set_ulps ? 1 : 0); ++ulps) {
  if (set_ulps) { set_ulps(ulps); printf("emulated reciprocal off by %d ulp:\n", ulps); }
  // ---- div2_shared on arrays: the production numerators, denominators over the allowed range ----
  {
    std::vector<float> n0, n1, d;
    for (int k = 0; k < 6; ++k)
      for (int i = 0; i < 20000; ++i) {
        n0.push_back(norms[k].norm2_0gt1);
        n1.push_back(norms[k].norm2_0lt1);
        const float edge[] = {0x1p-40f, nudge(0x1p-40f, 1), nudge(0x1p40f, -1), 1.0f, nudge(1.0f, -1), nudge(2.0f, -1)};
        d.push_back(i < 6 ? edge[i] : fabsf(logrand(-40, 40)));
      }
    const int n = (int)d.size();
    std::vector<float> got(2 * (size_t)n), want(2 * (size_t)n);
    for (int i = 0; i < n; ++i) { want[i] = n0[i] / d[i]; want[n + i] = n1[i] / d[i]; }
    run(GZ_MATH_DIV2_SHARED, n, n0.data(), n1.data(), d.data(), {}, got.data());
    check("div2_shared", n, 2, got, want, n0.data(), n1.data(), d.data());
  }
  // ---- the sweep: every stride-th denominator of [2^-40, 2^40), the twelve production numerators ----
  {
    float num[12];
    for (int k = 0; k < 6; ++k) { num[2 * k] = norms[k].norm2_0gt1; num[2 * k + 1] = norms[k].norm2_0lt1; }
    const unsigned long long total = 80ull << 23, count = (total + stride - 1) / stride;
    const unsigned sample_every = (unsigned)(count / 60000 + 1) | 1u;
    const unsigned long long nsample = (count + sample_every - 1) / sample_every;
    std::vector<float> sample((size_t)nsample * 12, -1.0f);
    uint64_t bad = ~0ull;
    const int rc = sweep(0, num, 12, stride, sample_every, &bad, sample.data(), sample.size());
    if (rc != GZ_OK) { fprintf(stderr, "gz_probe_div2_sweep: %d\n", rc); return 2; }
    printf("div2_shared sweep (stride %u): %llu quotients, %llu mismatches with the device's division\n", stride,
           count * 12, (unsigned long long)bad);
    if (bad) ++g_failures;
    size_t hbad = 0;
    for (unsigned long long s = 0; s < nsample; ++s) {
      const unsigned idx = (unsigned)(s * sample_every * stride);
      const float d = float_of((((idx >> 23) + 127u - 40u) << 23) | (idx & 0x7fffffu));
      for (int k = 0; k < 12; ++k)
        if (!same(sample[(size_t)s * 12 + k], num[k] / d) && hbad++ < 5)
          fprintf(stderr, "  sweep sample %llu: %a / %a: device %a, host %a\n", s, num[k], d, sample[(size_t)s * 12 + k], num[k] / d);
    }
    printf("div2_shared sweep sample: %llu quotients, %zu mismatches with the host's division\n", nsample * 12, hbad);
    if (hbad) ++g_failures;
  }
  }
  if (set_ulps) set_ulps(0);
  // ---- gamma_poly_f and opsin_pixel ----
  {
    std::vector<float> v = sample_values({0.971783f, 590.188894f, 1.01681026909f, 217.72491f}, 200000, 0.9, 300.0);
    for (int i = 0; i < 50000; ++i) v.push_back(frand(-50.0, 1000.0));
    const int n = (int)v.size();
    std::vector<float> got(n), want(n);
    for (int i = 0; i < n; ++i) want[i] = (float)gamma_plain((double)v[i]);
    run(GZ_MATH_GAMMA_POLY, n, v.data(), nullptr, nullptr, {}, got.data());
    check("gamma_poly_f", n, 1, got, want, v.data(), nullptr, nullptr);
  }
  {
    const int n = 120000;
    std::vector<float> bl(3 * (size_t)n), px(3 * (size_t)n), got(3 * (size_t)n), want(3 * (size_t)n);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) {
        const int kind = i % 8;
        float b = frand(0.0, 255.0), s = frand(0.0, 255.0);
        if (kind == 1) b = s;
        if (kind == 2) { b = (float)(g_rng() % 256); s = (float)(g_rng() % 256); }
        if (kind == 3) { b = fabsf(logrand(-20, 8)); s = fabsf(logrand(-20, 8)); }
        if (kind == 4 && i % 64 == 4) { b = kSpecials[(i / 64 + c) % kNumSpecials]; s = kSpecials[(i / 64 + 2 * c) % kNumSpecials]; }
        bl[(size_t)c * n + i] = b;
        px[(size_t)c * n + i] = s;
      }
    for (int i = 0; i < n; ++i) {
      const float b3[3] = {bl[i], bl[n + i], bl[2 * (size_t)n + i]}, p3[3] = {px[i], px[n + i], px[2 * (size_t)n + i]};
      float o[3];
      opsin_plain(b3, p3, o);
      for (int c = 0; c < 3; ++c) want[(size_t)c * n + i] = o[c];
    }
    run(GZ_MATH_OPSIN_PIXEL, n, bl.data(), px.data(), nullptr, {}, got.data());
    check("opsin_pixel", n, 3, got, want, bl.data(), px.data(), nullptr);
  }
  // ---- the range helpers of SeparateFrequencies ----
  {
    struct { int op; const char* name; double p; } ops[] = {
        {GZ_MATH_MAXIMUM_CLAMP, "maximum_clamp 78.8", 78.8223237675}, {GZ_MATH_MAXIMUM_CLAMP, "maximum_clamp 5.89", 5.8907152736},
        {GZ_MATH_REMOVE_RANGE, "remove_range 0.12", 0.120079806822},  {GZ_MATH_REMOVE_RANGE, "remove_range 0.029", 0.0287615200377},
        {GZ_MATH_AMPLIFY_RANGE, "amplify_range 0.034", 0.03430529365}};
    for (const auto& o : ops) {
      const float t = (float)o.p;
      const std::vector<float> v = sample_values({t}, 100000, -3.0 * o.p, 3.0 * o.p);
      const int n = (int)v.size();
      std::vector<float> got(n), want(n);
      for (int i = 0; i < n; ++i)
        want[i] = o.op == GZ_MATH_MAXIMUM_CLAMP ? plain_maximum_clamp(v[i], t)
                  : o.op == GZ_MATH_REMOVE_RANGE ? plain_remove_range(t, v[i]) : plain_amplify_range(t, v[i]);
      run(o.op, n, v.data(), nullptr, nullptr, {o.p}, got.data());
      check(o.name, n, 1, got, want, v.data(), nullptr, nullptr);
    }
  }
  // ---- two- and three-operand functions on the pair samples ----
  {
    const Pairs p = sample_pairs({0.4, 1.0, -0.4, -1.0, 0.0}, 60000);
    const int n = (int)p.a.size();
    std::vector<float> acc(n), got(3 * (size_t)n), want(3 * (size_t)n);
    for (int i = 0; i < n; ++i) acc[i] = i % 5 == 0 ? 0.0f : fabsf(logrand(-20, 20));
    for (int i = 0; i < n; ++i) want[i] = plain_suppress_x_by_y(p.a[i], p.b[i]);
    run(GZ_MATH_SUPPRESS_X_BY_Y, n, p.a.data(), p.b.data(), nullptr, {}, got.data());
    check("suppress_x_by_y", n, 1, got, want, p.a.data(), p.b.data(), nullptr);
    const float kMulSuppressHf = 1.10684769012, kRegHf = 2000 * (float)0.478741530298;
    const float kMulSuppressUhf = 1.76905001176, kRegUhf = 2000 * (float)0.310148420674;
    for (int k = 0; k < 2; ++k) {
      const float mul = k ? kMulSuppressUhf : kMulSuppressHf, reg = k ? kRegUhf : kRegHf;
      std::vector<float> br(n);
      for (int i = 0; i < n; ++i) br[i] = i % 97 == 0 ? -reg : i % 3 ? frand(0.0, 700.0) : p.b[i];
      for (int i = 0; i < n; ++i) want[i] = plain_suppress_bright(p.a[i], br[i], mul, reg);
      run(GZ_MATH_SUPPRESS_BRIGHT, n, p.a.data(), br.data(), nullptr, {mul, reg}, got.data());
      check(k ? "suppress_bright uhf" : "suppress_bright hf", n, 1, got, want, p.a.data(), br.data(), nullptr);
    }
    for (int i = 0; i < n; ++i) {
      float o[3];
      plain_lf_to_vals(p.a[i], p.b[i], acc[i], o);
      for (int c = 0; c < 3; ++c) want[(size_t)c * n + i] = o[c];
    }
    run(GZ_MATH_LF_TO_VALS, n, p.a.data(), p.b.data(), acc.data(), {}, got.data());
    check("lf_to_vals", n, 3, got, want, p.a.data(), p.b.data(), acc.data());
    for (double w : {1.01370836411, 1.74566011615}) {
      for (int i = 0; i < n; ++i) want[i] = plain_l2diff(acc[i], p.a[i], p.b[i], w);
      run(GZ_MATH_L2DIFF, n, acc.data(), p.a.data(), p.b.data(), {w}, got.data());
      check("l2diff_acc", n, 1, got, want, acc.data(), p.a.data(), p.b.data());
    }
    {
      double w_0gt1 = 32.4449876135 * asym, w_0lt1 = 32.4449876135 / asym;   // DiffmapPsychoImage, then L2DiffAsymmetric's
      w_0gt1 *= 0.8;                                                           // own factor (butteraugli.cc:680-681)
      w_0lt1 *= 0.8;
      for (int i = 0; i < n; ++i) want[i] = plain_l2diff_asym(acc[i], p.a[i], p.b[i], w_0gt1, w_0lt1);
      run(GZ_MATH_L2DIFF_ASYM, n, acc.data(), p.a.data(), p.b.data(), {w_0gt1, w_0lt1}, got.data());
      check("l2diff_asym_acc", n, 1, got, want, acc.data(), p.a.data(), p.b.data());
    }
  }
  {
    const float t = (float)85.7047444518;
    std::vector<float> a = sample_values({t, (float)(55.0184555849 / 0.918416534734), 55.0184555849f}, 100000, -200.0, 200.0);
    std::vector<float> b(a.size());
    for (size_t i = 0; i < a.size(); ++i) b[i] = i % 3 == 0 ? a[(i * 7 + 1) % a.size()] : i % 3 == 1 ? nudge(a[i], (int)(i % 5) - 2) : frand(0.0, 200.0);
    const int n = (int)a.size();
    std::vector<float> got(n), want(n);
    for (int i = 0; i < n; ++i) want[i] = plain_same_noise_pre(a[i], b[i]);
    run(GZ_MATH_SAME_NOISE_PRE, n, a.data(), b.data(), nullptr, {}, got.data());
    check("same_noise_pre", n, 1, got, want, a.data(), b.data(), nullptr);
    for (int i = 0; i < n; ++i) want[i] = plain_diff_from_sups(a[i], b[i]);
    run(GZ_MATH_DIFF_FROM_SUPS, n, a.data(), b.data(), nullptr, {}, got.data());
    check("diff_from_sups", n, 1, got, want, a.data(), b.data(), nullptr);
  }
  // ---- interp_lut512: finite arguments below 2^31 only (the argument becomes an index) ----
  {
    std::vector<double> table(512), ix;
    for (int i = 0; i < 512; ++i) table[i] = 1.0 / (0.01 * 16.2770141832 * i + 0.315424196682) + 1e-3 * (i % 7);
    for (int i = 0; i < 100000; ++i) ix.push_back(-20.0 + 560.0 * urand());
    for (double t : {0.0, 1.0, 510.0, 511.0, 512.0})
      for (int u = -2; u <= 2; ++u) ix.push_back(t == 0.0 ? u * 4.9e-324 : t + u * ldexp(1.0, -44));
    for (double t : {-0.0, -1e-300, 1e-300, -1e9, 1e9, 2147483000.0, 510.99999999999994, 0.99999999999999989}) ix.push_back(t);
    const int n = (int)ix.size();
    std::vector<double> got(n), want(n);
    for (int i = 0; i < n; ++i) want[i] = plain_interp(table.data(), 512, ix[i]);
    run(GZ_MATH_INTERP_LUT512, n, ix.data(), nullptr, nullptr, table, got.data());
    size_t bad = 0;
    std::string first;
    for (int i = 0; i < n; ++i)
      if (!same(got[i], want[i]) && bad++ < 5) {
        char buf[200];
        snprintf(buf, sizeof(buf), "  [%d] ix=%a: device %a, host %a\n", i, ix[i], got[i], want[i]);
        first += buf;
      }
    report("interp_lut512", n, bad, first);
  }
  // ---- quant_div against C++'s / and % ----
  {
    std::vector<int32_t> a, q;
    for (int i = 0; i < 400000; ++i) { a.push_back((int)(g_rng() % 65537) - 32768); q.push_back(1 + (int)(g_rng() % (i % 2 ? 65535 : 255))); }
    for (int qq : {1, 2, 3, 7, 255, 256, 257, 32767, 32768, 65535})
      for (int m = -40; m <= 40; ++m)
        for (int d = -1; d <= 1; ++d) {
          const long v = (long)m * qq + d;
          if (v >= -32768 && v <= 32768) { a.push_back((int)v); q.push_back(qq); }
        }
    const int n = (int)a.size();
    std::vector<int32_t> got(n);
    run(GZ_MATH_QUANT_DIV, n, a.data(), q.data(), nullptr, {}, got.data());
    size_t bad = 0;
    std::string first;
    for (int i = 0; i < n; ++i)
      if ((got[i] != a[i] / q[i] || a[i] - got[i] * q[i] != a[i] % q[i]) && bad++ < 5) {
        char buf[200];
        snprintf(buf, sizeof(buf), "  [%d] %d / %d: device %d, host %d\n", i, a[i], q[i], got[i], a[i] / q[i]);
        first += buf;
      }
    report("quant_div", n, bad, first);
  }
  if (g_failures) { fprintf(stderr, "device_math: %d checks FAILED\n", g_failures); return 1; }
  printf("device_math: ok\n");
  return 0;
}
