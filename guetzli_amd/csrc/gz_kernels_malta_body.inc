// The body of k_malta_rolled and of its batched sibling k_malta_rolled_batch (gz_kernels_diff.h includes this file once
// in either, with GZ_MALTA_BATCHED 0 and 1).  Not a function: a kernel's two LDS arrays are named after the kernel, a
// shared function template (or a parameter pack on the kernel, as the blur kernels have) renames them, the compiler
// then lays them out the other way round, and the kernel of one image no longer compiles to what it compiled to.  With
// GZ_MALTA_BATCHED 0 the text is the kernel's as it was.  In scope: a0, a1, w, h, pitch and, batched, `batch` (BatchIdx).
  const GzTile bid = gz_xcd_tile();
#if GZ_MALTA_BATCHED   // grid z = image x 2 + channel
  const int img = bid.z >> 1;
  const MaltaArgs<NPASS>& a = (bid.z & 1) ? a1 : a0;
#else
  const MaltaArgs<NPASS>& a = bid.z ? a1 : a0;
#endif
  __shared__ __attribute__((aligned(16))) float tile[MH + 8][MW + 8];
  const int tx = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const int x0 = bid.x * MW, y0 = bid.y * MH;
  __shared__ float accs[MPT][256];
#pragma unroll
  for (int i = 0; i < MPT; ++i) accs[i][threadIdx.x] = 0.0f;   // (own slots: no barrier needed)
  // the haloed tile starts at x0 - 4: rows can be staged with aligned 16-byte loads when the
  // tile lies inside the image horizontally and the pitch allows it
  const bool vec = x0 >= 4 && x0 + MW + 4 <= w && (pitch & 3) == 0;
  for (int ps = 0; ps < NPASS; ++ps) {
#if GZ_MALTA_BATCHED   // (the arguments stay where they are -- a pass is picked with a run-time index: its copy moves)
    MaltaPass P = a.pass[ps];
    P.p0 += img * batch.ref_stride;
    P.p1 += img * batch.stride;
#else
    const MaltaPass P = a.pass[ps];
#endif
    // the pass's three constants in vector registers: malta_diff adds / multiplies them into every
    // staged sample, and a scalar-register operand makes those 4-cycle instructions (GZ_IN_VGPR)
    MaltaNorm nm = P.nm;
    nm.norm1f = GZ_IN_VGPR(nm.norm1f);
    nm.norm2_0gt1 = GZ_IN_VGPR(nm.norm2_0gt1);
    nm.norm2_0lt1 = GZ_IN_VGPR(nm.norm2_0lt1);
    if (ps > 0) __syncthreads();
    if (vec) {
      constexpr int NV = (MH + 8) * ((MW + 8) / 4);   // 16-byte vectors in the tile
#pragma unroll 1
      for (int k = 0; k < (NV + 255) / 256; ++k) {
        const int i = 256 * k + (int)threadIdx.x;
        if (i < NV) {
          const int ry = i / ((MW + 8) / 4), q = i - ry * ((MW + 8) / 4);
          const int y = y0 - 4 + ry;
          gz_f4 v;
          v.v[0] = v.v[1] = v.v[2] = v.v[3] = 0.0f;
          if (y >= 0 && y < h) {
            const size_t idx = (size_t)y * pitch + (x0 - 4 + 4 * q);
            const gz_f4 u0 = GZ_LDG4(P.p0, idx), u1 = GZ_LDG4(P.p1, idx);
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = malta_diff(u0.v[e], u1.v[e], nm);
          }
          *reinterpret_cast<gz_f4*>(&tile[ry][4 * q]) = v;
        }
      }
    } else {
      for (int i = threadIdx.x; i < (MH + 8) * (MW + 8); i += 256) {
        const int ry = i / (MW + 8), rx = i - ry * (MW + 8);
        const int x = x0 - 4 + rx, y = y0 - 4 + ry;
        float v = 0.0f;
        if (x >= 0 && x < w && y >= 0 && y < h) {
          const size_t idx = (size_t)y * pitch + x;
          v = malta_diff(GZ_LDG(P.p0, idx), GZ_LDG(P.p1, idx), nm);
        }
        tile[ry][rx] = v;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < MPT; ++i) {
      const int ly = tg * MPT + i;
      const float r = P.lf ? malta_unit<true>(tile, ly + 4, tx + 4)
                           : malta_unit<false>(tile, ly + 4, tx + 4);
      accs[i][threadIdx.x] += r;
    }
  }
  const int x = x0 + tx;
  if (x >= w) return;
#pragma unroll
  for (int i = 0; i < MPT; ++i) {
    const int y = y0 + tg * MPT + i;
    if (y >= h) break;
    const size_t idx = (size_t)y * pitch + x;
    const float v = accs[i][threadIdx.x];
#if GZ_MALTA_BATCHED
    GZ_STG(a.out + img * batch.stride, idx, v);
#else
    GZ_STG(a.out, idx, v);
#endif
  }
