// Times gz::malta_diff (gz_math.h: no if-ladder, two quotients from one v_rcp_f32) against
// malta_diff_plain on band-like data.  Timing only: that the two give the same bits on the device
// -- for every float denominator of [2^-40, 2^40] -- is checked by the suite (gz_probe_div2_sweep,
// gz_probe_math: tests/cpp/test_device_math.cc, run by tests/test_gpu_parity.py).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I../../guetzli_amd/csrc divcheck.hip -o divcheck
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "gz_common.h"
#include "gz_math.h"
using gz::MaltaNorm;

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
  n.fast_div = 1;
  return n;
}
struct Norms { MaltaNorm n[6]; };

template <bool FAST>
__global__ void k_time_only(const float* a, const float* b, float* o, MaltaNorm nm, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  o[i] = FAST ? gz::malta_diff(a[i], b[i], nm) : gz::malta_diff_plain(a[i], b[i], nm);
}
template <bool FAST, int REP>
__global__ void k_valu(const float* a, const float* b, float* o, Norms nn, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  const float x = a[i], y = b[i];
#pragma unroll 1
  for (int r = 0; r < REP; ++r)
#pragma unroll
    for (int k = 0; k < 6; ++k)
      acc += FAST ? gz::malta_diff(x + (float)r, y, nn.n[k]) : gz::malta_diff_plain(x + (float)r, y, nn.n[k]);
  o[i] = acc;
}
int main() {
  const float asym = 0.8f, sq = sqrtf(asym);
  Norms nn;
  nn.n[0] = norm_of(false, 5.1409625726 * asym, 5.1409625726 / asym, 58.5001247061);
  nn.n[1] = norm_of(true, 153.671655716 * sq, 153.671655716 / sq, 83150785.9592);
  nn.n[2] = norm_of(true, 6841.81248144, 6841.81248144, 0.0135134962487);
  nn.n[3] = norm_of(false, 4.91743441556 * asym, 4.91743441556 / asym, 687196.39002);
  nn.n[4] = norm_of(true, 668.358918152 * sq, 668.358918152 / sq, 0.882954368025);
  nn.n[5] = norm_of(true, 813.901703816, 813.901703816, 16792.9322251);
  const int n = 1 << 24;
  float *a, *b, *o; hipMalloc(&a, n * 4); hipMalloc(&b, n * 4); hipMalloc(&o, n * 4);
  float* h = (float*)malloc(n * 4);
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
  for (int i = 0; i < n; ++i) h[i] = (rnd() - 0.5f) * 20.0f;
  hipMemcpy(a, h, n * 4, hipMemcpyHostToDevice);
  for (int i = 0; i < n; ++i) h[i] = h[i] * (0.3f + 1.2f * rnd()) * (rnd() < 0.05f ? -1.0f : 1.0f);
  hipMemcpy(b, h, n * 4, hipMemcpyHostToDevice);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int fast = 0; fast < 2; ++fast) {
    hipEventRecord(e0);
    for (int r = 0; r < 20; ++r) {
      if (fast) hipLaunchKernelGGL(k_time_only<true>, dim3(n / 256), dim3(256), 0, 0, a, b, o, nn.n[r % 6], n);
      else hipLaunchKernelGGL(k_time_only<false>, dim3(n / 256), dim3(256), 0, 0, a, b, o, nn.n[r % 6], n);
    }
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%s: %.1f us per 16.8 M values (3 plane passes = 201 MB)\n", fast ? "malta_diff      " : "malta_diff_plain", ms / 20 * 1000);
  }
  for (int fast = 0; fast < 2; ++fast) {
    hipEventRecord(e0);
    for (int r = 0; r < 5; ++r) {
      if (fast) hipLaunchKernelGGL((k_valu<true, 8>), dim3(n / 256), dim3(256), 0, 0, a, b, o, nn, n);
      else hipLaunchKernelGGL((k_valu<false, 8>), dim3(n / 256), dim3(256), 0, 0, a, b, o, nn, n);
    }
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%s, 48 evaluations per loaded pair: %.1f us per 16.8 M pairs = %.3f ns per evaluation chip-wide\n",
           fast ? "malta_diff      " : "malta_diff_plain", ms / 5 * 1000, ms / 5 * 1e6 / (48.0 * n));
  }
  return 0;
}
