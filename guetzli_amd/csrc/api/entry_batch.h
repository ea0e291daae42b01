// C ABI: gz_butteraugli_batch -- n image pairs of one size through ONE Compare chain.  A context without an original lives
// for the call; its arena is a chunk's image arenas back to back with the result words behind them, its plane pointers
// are the first arena's, and while gz_ctx::batch.n > 0 every launch of the chain's dispatchers (chain.h) covers batch.n
// images: the stages that run are the ones a pair comparison runs, enqueued on ONE stream in the order enqueue_compare
// uses when it is not forked.  The tensors' ends are k_ingest_rgb's and k_emit_map's batched forms.
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

namespace {

constexpr size_t kBatchDefaultScratch = (size_t)2 << 30;   // scratch_cap_bytes == 0
constexpr int kBatchMaxGridImages = 65535 / 3;              // gridDim.z = images x planes of the launch, 3 at the most
constexpr uint64_t kBatchMaxPixels = 1500000;               // (chain.h: below it a lone image gets the configuration the batch has)

// (the arguments alone -- check_device_batch, check_device_map_batch: tensor.h)

// k_ingest_rgb's batched form on `stream`: images first .. first + count - 1 of b -> the linear planes of `count` arenas.
// The 16-byte reads need every image's base aligned: the first one's, and stride_n a multiple of the vector's elements.
void launch_ingest_batch(hipStream_t stream, const gz_device_batch* b, int first, int count, int w, int h, const float* lut, float* lin,
                         int pitch, size_t pstride, size_t arena_stride) {
  const long long sn = b->stride_n, sy = b->stride_y, sx = b->stride_x, sc = b->stride_c;
  with_sample_type(b->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if constexpr (!std::is_same<T, uint16_t>::value) {   // (a batch holds no GZ_DT_U16, and the kernel has no batched form of it)
      const T* data = (const T*)b->data + (long long)first * sn;
      constexpr int P = 16 / (int)sizeof(T);
      const int wide = sn % P == 0 ? ingest_wide_mode(data, sizeof(T), sy, sx, sc) : (int)kIngestElementwise;
      const dim3 grid((unsigned)(((size_t)gz_div_up(w, P) * h + 255) / 256), (unsigned)count), block(256);
      const BatchTensor bt = {sn, arena_stride};
      uint8_t* const no_bytes = nullptr;
      GZ_LAUNCH((k_ingest_rgb<T, BatchTensor>), grid, block, stream, data, sy, sx, sc, w, h, wide, no_bytes, lut, lin, pitch, pstride, bt);
    }
  });
}

// k_emit_map's batched form: the `count` arenas' map planes -> maps first .. first + count - 1 of m.
void launch_emit_map_batch(hipStream_t stream, const float* plane, size_t arena_stride, int w, int h, int pitch, const gz_device_map_batch* m,
                           int first, int count) {
  const long long sn = m->stride_n, sy = m->stride_y, sx = m->stride_x;
  with_float_type(m->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    T* out = (T*)m->data + (long long)first * sn;
    constexpr int P = 16 / (int)sizeof(T);
    const dim3 grid((unsigned)(((size_t)((w + P - 1) / P) * h + 255) / 256), (unsigned)count), block(256);
    const BatchTensor bt = {sn, arena_stride};
    if (sn % P == 0 && emit_map_wide(out, sizeof(T), sy, sx)) {
      GZ_LAUNCH((k_emit_map<T, true, BatchTensor>), grid, block, stream, plane, w, h, pitch, out, sy, sx, bt);
    } else {
      GZ_LAUNCH((k_emit_map<T, false, BatchTensor>), grid, block, stream, plane, w, h, pitch, out, sy, sx, bt);
    }
  });
}

// The batch's own state in the context: on for the launches of a chunk, off again on every path out.
struct BatchScope {
  gz_ctx* c;
  BatchScope(gz_ctx* c_, int n, size_t stride, size_t ref_stride) : c(c_) {
    c->batch.n = n;
    c->batch.idx = BatchIdx{stride, ref_stride};
  }
  ~BatchScope() { c->batch.n = 0; }
  BatchScope(const BatchScope&) = delete;
  BatchScope& operator=(const BatchScope&) = delete;
};

// (the context's device is current, every argument is checked; c has `per_chunk` arenas)
int butteraugli_batch(gz_ctx* c, int n, const gz_device_batch* ref, int n_ref, const gz_device_batch* other, float* distances,
                      float* host_distances, const gz_device_map_batch* maps, int per_chunk) {
  const int w = c->w, h = c->h;
  const size_t stride = batch_arena_stride(c->plane);
  const hipStream_t stream = c->stream;
  const ChainStreams cs = chain_streams(c, false);   // ONE stream: the batch supplies the parallelism
  c->batch.max_bits = (unsigned*)(c->arena + stride * (size_t)per_chunk);
  TRY(wait_for_producer(c, ref->producer_stream));
  if (other->producer_stream != ref->producer_stream) TRY(wait_for_producer(c, other->producer_stream));
  if (n_ref == 1) {
    // one reference for all: its planes once, in the first arena, by the kernels of a lone image (batch.n == 0)
    launch_ingest(stream, tensor_select(tensor_view(ref, w, h, 1), 0, 0), nullptr, w, h, c->d_rgb, c->d_srgb_lut, c->lin[0], c->pitch, c->plane);
    KCHK(c);
    TRY(stage_opsin(c, stream));
    TRY(stage_separate(c, cs, &c->pi0));
    MaskIn in0[2];
    mask_in_psycho(c->pi0, in0);
    TRY(stage_mask_sup(c, stream, in0, c->sup0));
  }
  if (maps && maps->consumer_stream && !c->ev_emit) TRY(own_event(c, &c->ev_emit));   // (in front of the chunks: outputs_after_consumers finds it)
  for (int first = 0; first < n; first += per_chunk) {
    const int m = std::min(per_chunk, n - first);
    BatchScope scope(c, m, stride, n_ref == 1 ? 0 : stride);
    if (n_ref != 1) {   // the references of this chunk: pi0 and sup0 of every arena
      launch_ingest_batch(stream, ref, first, m, w, h, c->d_srgb_lut, c->lin[0], c->pitch, c->plane, stride);
      KCHK(c);
      TRY(stage_opsin(c, stream));
      TRY(stage_separate(c, cs, &c->pi0));
      MaskIn in0[2];
      mask_in_psycho(c->pi0, in0);
      TRY(stage_mask_sup(c, stream, in0, c->sup0));
    }
    launch_ingest_batch(stream, other, first, m, w, h, c->d_srgb_lut, c->lin[0], c->pitch, c->plane, stride);
    KCHK(c);
    TRY(stage_opsin(c, stream));
    TRY(stage_separate(c, cs, &c->pi1));
    TRY(stage_diffmap(c, cs, c->pi0, c->pi1, maps ? kWantDistmap : 0u, ClearMax::kMemset));
    if (maps) {
      // the consumer's stream: waited for in front of the first emit kernel, and it waits behind the last one
      if (first == 0) TRY(outputs_after_consumers(c, stream, &c->ev_emit, {maps->consumer_stream}));
      launch_emit_map_batch(stream, c->distmap, stride, w, h, c->pitch, maps, first, m);
      KCHK(c);
    }
    HIPCHK(c, hipMemcpyAsync(distances + first, c->batch.max_bits, sizeof(float) * (size_t)m, hipMemcpyDeviceToDevice, stream));
  }
  if (maps) TRY(consumers_after_outputs(c, stream, c->ev_emit, {maps->consumer_stream}));
  if (host_distances) HIPCHK(c, hipMemcpyAsync(host_distances, distances, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));   // (the arenas go back to the pool behind this; the tensors are read and written)
  return GZ_OK;
}

}  // namespace

extern "C" {

int gz_butteraugli_batch(int device, int w, int h, int n, const gz_device_batch* ref, int n_ref, const gz_device_batch* other,
                         float* distances, float* host_distances, const gz_device_map_batch* maps, size_t scratch_cap_bytes) {
  // all of these before any device call
  if (!ref || !other || !distances || n < 1 || (n_ref != 1 && n_ref != n)) return GZ_E_ARG;
  if (w < 8 || h < 8 || w >= (1 << 16) || h >= (1 << 16) || (uint64_t)w * (uint64_t)h >= kBatchMaxPixels) return GZ_E_ARG;
  if (check_device_batch(ref, w, h, n_ref) != GZ_OK || check_device_batch(other, w, h, n) != GZ_OK) return GZ_E_ARG;
  if (maps && check_device_map_batch(maps, w, h, n) != GZ_OK) return GZ_E_ARG;
  if (((uintptr_t)distances & 3u) != 0) return GZ_E_ARG;
  // chunks: as many arenas as the cap holds and the grid can index, one at the least
  const size_t cap = scratch_cap_bytes ? scratch_cap_bytes : kBatchDefaultScratch;
  const size_t per_image = sizeof(float) * batch_arena_stride((size_t)w * h) + sizeof(unsigned);
  const int per_chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, cap / per_image, (size_t)kBatchMaxGridImages}));
  CallerDevice keep(device);
  TRY(probe_device(device));
  TRY(check_tensor_memory(device, tensor_view(ref, w, h, n_ref), "reference batch", nullptr));
  TRY(check_tensor_memory(device, tensor_view(other, w, h, n), "batch", nullptr));
  TRY(check_device_range(device, distances, (uint64_t)(n - 1), sizeof(float), "distances", nullptr));
  if (maps) TRY(check_tensor_memory(device, tensor_view(maps, w, h, n), "maps", nullptr));
  int rc = GZ_OK;
  const CallContext ctx(create_context(device, w, h, nullptr, nullptr, 1.0f, &rc, nullptr, per_chunk));
  return ctx.c ? butteraugli_batch(ctx.c, n, ref, n_ref, other, distances, host_distances, maps, per_chunk) : rc;
}

}  // extern "C"
