/* guetzli_amd.h -- C ABI of the MI355X (gfx950) implementation of Guetzli's
 * block-parallel hot path: per-8x8-block FDCT / quantise / IDCT / colour transform and
 * the butteraugli distance map evaluated for every candidate by
 * Processor::TryQuantMatrix and Processor::SelectFrequencyMasking.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no C++,
 * HIP or torch types.  A maintainer of the reference binds it from a
 * `guetzli::Comparator` subclass (INTEGRATION.md shows the stub); every entry point
 * cites the reference interface it replaces as path:line under /root/reference.
 *
 * Conventions
 *   - one gz_ctx per (image, GPU); calls on one context are serialised by the caller
 *     (the reference objects are single-threaded too: comparator.h:29-96); contexts are
 *     independent of each other.
 *   - every function returns GZ_OK (0) or a negative GZ_E_* code; nothing throws, nothing
 *     prints.  gz_last_error(ctx) gives a static description of the last failure.
 *   - host pointers are ordinary pageable memory unless named `dev_*`.
 *   - layouts
 *       rgb     : uint8 packed, rgb[(y*w + x)*3 + c]                (guetzli.cc ReadPNG)
 *       coeffs  : int16 DEQUANTISED DCT coefficients, component-major then block-major
 *                 (= OutputImageComponent::coeffs_, output_image.h:33-40, one after the
 *                 other for c = 0,1,2).  4:4:4 frame: coeffs[(c*nb + by*bw + bx)*64 + k],
 *                 bw=ceil(w/8), bh=ceil(h/8), nb=bw*bh.  4:2:0 frame (the two chroma
 *                 components Reset(2, 2), output_image.cc:40-49): nb luma blocks, then
 *                 nbc = ceil(w/16)*ceil(h/16) blocks of Cb, then nbc of Cr -- no MCU padding
 *                 (SaveToJpegData's padding blocks, :386-404, are implied).  A context starts
 *                 in 4:4:4; gz_downsample / gz_set_orig_coeffs_420 switch it to 4:2:0,
 *                 gz_encode_rgb / gz_set_orig_coeffs back; gz_frame_layout tells.
 *       q       : int[3][64] quantisation matrices in natural (row-major) order
 *       planes  : float, plane[y*w + x] (no row padding on the host side)
 */
#ifndef GUETZLI_AMD_H_
#define GUETZLI_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GZ_OK 0
#define GZ_E_ARG (-1)        /* bad argument (null, size out of range, w/h < 8 ...) */
#define GZ_E_NO_DEVICE (-2)  /* no usable gfx950 device / HIP runtime failure at init */
#define GZ_E_HIP (-3)        /* a HIP call failed; see gz_last_error */
#define GZ_E_STATE (-4)      /* call sequence violated (e.g. compare before coefficients) */
#define GZ_E_NOMEM (-5)      /* out of device or page-locked memory: the context stays valid and holds nothing of the
                                failed call's half-made buffers; the call may be repeated (after freeing memory) */

typedef struct gz_ctx gz_ctx;

/* Library / device ------------------------------------------------------------ */
int gz_abi_version(void);                 /* currently 6 (5 without the two experiment fields of gz_config); the
                                             device-input entries (gz_device_image, gz_create_from_device,
                                             gz_set_rgb_device, gz_pack_rgb_device) were ADDED to version 6: no
                                             existing declaration, struct or call sequence changed, so the number stays;
                                             so were gz_device_pixels and its three entries, and gz_device_output and
                                             its three (gz_decode_coeffs_device, gz_decode_coeffs,
                                             gz_reconstruct_device), and gz_device_map and its entries
                                             (gz_compare_device_pixels, gz_compare_rgb, gz_distmap_device), and the heat
                                             map's entries (gz_heatmap_device, gz_compare_device_pixels_heat,
                                             gz_heatmap_from_map_device, gz_butteraugli_fuzzy_*), the linear float
                                             entries (gz_create_from_device_linear, gz_set_linear_device,
                                             gz_compare_device_linear, gz_butteraugli_linear) and the masking entries
                                             (gz_opsin_device, gz_mask_device, gz_adaptive_quantization), by the same rule */
/* Device and pinned host memory of destroyed contexts is kept (per device, exact sizes, at
 * most GZ_POOL_MB megabytes of device memory, default 16384) for the next context of the same
 * image size: a batch of same-sized images allocates once.  gz_trim_pool releases everything
 * that is cached; GZ_POOL_MB=0 turns the caching off. */
int gz_trim_pool(void);
int gz_device_count(void);                /* number of visible HIP devices, <0 on error */
const char* gz_strerror(int code);
const char* gz_last_error(const gz_ctx* ctx);
/* A caller that runs several images at once in this process (one thread + one context each) says so before it starts
 * them: n = images in flight (<= 1: lone images again).  Only a hint, process-wide, no result depends on it: a context
 * created while the device is empty takes a highest-priority main stream (worth 2 % of a lone 4K chain) unless the hint
 * says that company is coming -- a priority stream is one more hardware queue for the runtime to multiplex and costs a
 * batch 1-4 %; with n > 1 the idle priority stream sets of the pool are destroyed as well. */
void gz_hint_images_in_flight(int n);
/* PCI bus id of a HIP device ("0000:05:00.0"; hipDeviceGetPCIBusId) -- for NUMA-aware placement of the
 * process that feeds it (bench.py / guetzli_amd/affinity.py); out needs >= 16 bytes. */
int gz_device_pci_bus_id(int device, char* out, int cap);

/* Run-time configuration of a context -------------------------------------------
 * What used to be read from GZ_* environment variables on every call (rounds 1-5) is a struct of the context:
 * gz_create fills it ONCE from the environment (gz_config_from_environment: the variable behind every field is
 * named below), gz_get_config / gz_set_config read and replace it (between calls, never while work of the
 * context is in flight).  None of the fields changes a result bit: they choose kernel instantiations and
 * stream use, and exist for the tests (every instantiation on small images) and for A/B measurements.
 * Process-wide settings stay in the environment, read once: GZ_POOL_MB (cache of freed device memory). */
typedef struct gz_config {
  int struct_size;      /* sizeof(gz_config) as the caller compiled it (checked by gz_set_config) */
  int blur_packed;      /* GZ_BLUR_PK      -1: by image size (row / column pairs from 1.5 MPix on); 0, 1: forced */
  int tile_rows;        /* GZ_TILE_ROWS     0: by image size (16-row blur tiles below 7 MPix); 16, 32: forced */
  int single_stream;    /* GZ_SINGLE_STREAM -1: one stream when other contexts are alive on the device (a batch's images in
                                            flight), three for a lone context; 0: always three; 1: always one */
  int store_distmap;    /* GZ_STORE_DISTMAP 1: every Compare stores the distance map (default: only gz_compare with
                                            distmap != NULL and the stage probes do) */
  int patch_reconstruct;/* GZ_PATCH_RECON   1 (default): gz_apply_candidate_steps / gz_apply_coeff_edits transform the block
                                            positions they change again (4:4:4 frames of half a megapixel and more, while
                                            fewer than half of the blocks change) and the Compare behind them skips its
                                            full reconstruction; 0: every Compare reconstructs the whole image; 2: as 1 at
                                            every image size, and every such Compare checks the patched planes against a
                                            full reconstruction first (GZ_E_STATE on a difference; tests).
                                            gz_time_compare / gz_compare_enqueue always run the whole chain. */
  int opsin_ahead;      /* GZ_OPSIN_AHEAD   1 (default): with patch_reconstruct, a context that has the device to itself runs
                                            the opsin blur of the next Compare right behind gz_apply_candidate_steps'
                                            patches -- while the host takes its serial steps -- and gz_apply_coeff_edits
                                            recomputes the opsin tiles around the blocks it edits; 0: every Compare runs it */
} gz_config;
int gz_config_from_environment(gz_config* out);
int gz_get_config(const gz_ctx* ctx, gz_config* out);
int gz_set_config(gz_ctx* ctx, const gz_config* in);

/* Context ---------------------------------------------------------------------
 * gz_create: replaces guetzli::ButteraugliComparator::ButteraugliComparator
 * (butteraugli_comparator.cc:51-61) -- uploads the original sRGB image, converts it to
 * linear RGB (LinearRgb, :33-47) and precomputes the original's PsychoImage pi0_
 * (butteraugli.cc:784-791).  `target` is Params::butteraugli_target
 * (processor.h:30).  Requires w,h >= 8 (butteraugli) -- Process() itself only builds a
 * comparator when w,h >= 32 (processor.cc:940) -- and w,h < 65536 (JPEG) with at most
 * 11.18 M 8x8 blocks (715 MPix: coefficient positions are 32-bit), else GZ_E_ARG.  Returns
 * NULL on failure, *err set.
 * Every entry point that takes a context runs on the context's device and leaves the calling
 * thread's current HIP device as it found it (a thread may own contexts on several GPUs). */
gz_ctx* gz_create(int device, int w, int h, const uint8_t* rgb, float target, int* err);
void gz_destroy(gz_ctx* ctx);
/* Replace the original image of an existing context (same w, h): what constructing a new
 * ButteraugliComparator on other pixels does.  Used by the JPEG-input path, whose original is
 * DecodeJpegToRGB(jpg) (jpeg_data_decoder.cc:45-54) -- an IDCT of the input's coefficients
 * that the context itself computes (gz_set_orig_coeffs, gz_quantize(NULL), gz_reconstruct). */
int gz_set_rgb(gz_ctx* ctx, const uint8_t* rgb);

/* Device-resident input ----------------------------------------------------------
 * The original as a strided image that already lives in DEVICE memory (a decoder's, a resize's or a model's
 * output): element (y, x, c) of the w x h x 3 image is data[y*stride_y + x*stride_x + c*stride_c], strides in
 * ELEMENTS, each >= 0 -- HWC, CHW, cropped views (a row pitch larger than the row), grey broadcast over the
 * channels (stride_c = 0), any element alignment of the base.  One kernel converts it to the context's packed 8-bit
 * image and its linear planes; nothing goes through host memory.
 * Byte of an element: integers pass through.  A float x becomes rint(clamp(float32(x) * 255.0f, 0, 255)) -- one f32
 * multiplication, NaN -> 0, below 0 (and -inf) -> 0, above 255 (and +inf) -> 255, round to nearest with ties to
 * even -- so k/255 stored in any of the three float types comes back as k.
 * Stream contract: producer_stream is the hipStream_t whose already enqueued work writes the data; the call records
 * an event there and makes the context's stream wait for it (no host synchronisation of the producer).  NULL: there
 * is nothing to wait for -- the data is complete, or its producer is the legacy default stream, with which the
 * context's (blocking) streams synchronise by themselves.  The source is fully read when the call returns.
 * The memory must be readable by the context's device (device memory of that device, managed memory, or page-locked
 * host memory mapped at the same address): anything else -- an ordinary host pointer -- is GZ_E_ARG, not a fault. */
#define GZ_DT_U8 0
#define GZ_DT_F32 1
#define GZ_DT_F16 2
#define GZ_DT_BF16 3
typedef struct gz_device_image {
  int struct_size;            /* sizeof(gz_device_image) */
  int dtype;                  /* GZ_DT_U8 / GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 */
  const void* data;           /* device address of element (0,0,0) */
  int64_t stride_y, stride_x, stride_c;   /* elements, >= 0 */
  void* producer_stream;      /* hipStream_t whose work produced the data; NULL = none to wait for */
} gz_device_image;
/* gz_create with the ingest kernel in place of the upload: same limits on w and h, same ownership (all or nothing).
 * GZ_E_ARG (before any device call): NULL img or data, a wrong struct_size, an unknown dtype, a negative stride, an
 * extent whose last element offset does not fit 62 bits. */
gz_ctx* gz_create_from_device(int device, int w, int h, const gz_device_image* img, float target, int* err);
/* gz_set_rgb from such an image (the context's w and h). */
int gz_set_rgb_device(gz_ctx* ctx, const gz_device_image* img);
/* The conversion alone, without a context: img (w x h, 0 < w, h < 65536) -> host_rgb_out, packed uint8 w*h*3.  For
 * images too small for a context (w or h < 32: gz_encode_rgb_only takes the bytes from there). */
int gz_pack_rgb_device(int device, const gz_device_image* img, int w, int h, uint8_t* host_rgb_out);

/* Device-resident input with alpha and 16-bit samples: the pixel forms a PNG can hold (grey, grey + alpha, RGB, RGBA;
 * 8 or 16 bits), under the arithmetic of the PNG front end (host/png_reader.cc, the reference's ReadPNG) -- the raw
 * samples of a PNG handed over as device memory encode to the bytes `guetzli in.png out.jpg` writes.
 * gz_device_pixels is gz_device_image (same addressing, same stream contract, same memory rules) and
 *   dtype GZ_DT_U16: the byte of a sample v is v >> 8, the HIGH byte (libpng's STRIP_16), not a rounding;
 *   alpha: the device address of the alpha sample of pixel (0, 0), of the colours' dtype; the alpha of pixel (y, x) is
 *     alpha[y*stride_y + x*stride_x] -- data + 3 of HWC RGBA, the fourth plane of CHW, data + 1 of interleaved
 *     grey + alpha (stride_c = 0, stride_x = 2), or a mask in an allocation of its own.  NULL: the image is opaque.
 *   background: the bytes r, g, b (and 0) the pixels are blended over.
 * With a the byte of the alpha sample (floats by the float rule above: NaN is transparent), v the byte of a colour
 * sample and bg the background's byte of that channel:
 *   out = (v * a + bg * (255 - a) + 128) / 255     integer (floor) division
 * which is BlendOnBlack (guetzli.cc:42-44) at bg = 0; a = 255 gives v, a = 0 gives bg.  Nothing is premultiplied.
 * The three entries are the three above for such pixels (those forward here with alpha = NULL), with the same
 * contract: GZ_E_ARG before any device call for NULL img or data, a wrong struct_size, an unknown dtype, a negative
 * stride, an extent -- the alpha extent (h-1) stride_y + (w-1) stride_x included -- beyond 62 bits; alpha gets data's
 * pointer checks (readable by the context's device, its extent inside its allocation; a host pointer is GZ_E_ARG and
 * gz_last_error names alpha). */
#define GZ_DT_U16 4                      /* gz_device_pixels and gz_device_output only */
typedef struct gz_device_pixels {
  int struct_size;            /* sizeof(gz_device_pixels) */
  int dtype;                  /* GZ_DT_U8 / GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 / GZ_DT_U16 */
  const void* data;           /* device address of element (0,0,0) */
  int64_t stride_y, stride_x, stride_c;   /* elements, >= 0 */
  void* producer_stream;      /* hipStream_t whose work produced the data; NULL = none to wait for */
  const void* alpha;          /* device address of the alpha sample of pixel (0,0); NULL = opaque */
  uint8_t background[4];      /* r, g, b, 0 */
} gz_device_pixels;
gz_ctx* gz_create_from_device_pixels(int device, int w, int h, const gz_device_pixels* img, float target, int* err);
int gz_set_rgb_device_pixels(gz_ctx* ctx, const gz_device_pixels* img);
int gz_pack_rgb_device_pixels(int device, const gz_device_pixels* img, int w, int h, uint8_t* host_rgb_out);

int gz_synchronize(gz_ctx* ctx);
/* Run subsequent work of this context on an externally owned hipStream_t (e.g. torch's
 * current stream, so that torch.cuda.Event timing sees the kernels).  NULL restores the
 * context's own stream. */
int gz_set_stream(gz_ctx* ctx, void* hip_stream);

/* Block path ------------------------------------------------------------------
 * gz_encode_rgb: replaces EncodeRGBToJpeg (jpeg_data_encoder.cc:66-117) for the
 * all-ones quantisation: RGBToYUV16 (:40-48, edge-clamped gather :88-98) ->
 * ComputeBlockDCT (fdct.cc:230) -> (v*65537 + 0x80000) >> 20 (:33-35).  The result is
 * kept on the device as the context's ORIGINAL coefficients and, if coeffs_out != NULL,
 * copied to the host. */
int gz_encode_rgb(gz_ctx* ctx, int16_t* coeffs_out);

/* The same transform without a context, for images too small for butteraugli (w or h < 32:
 * Process() emits the unquantised JPEG, processor.cc:832-838, and gz_create needs >= 8):
 * rgb w*h*3 -> coeffs [3][nb][64].  0 < w, h < 65536. */
int gz_encode_rgb_only(int device, const uint8_t* rgb, int w, int h, int16_t* coeffs_out);

/* Upload original (unquantised) coefficients computed elsewhere (JPEG input path:
 * JPEGData after RemoveOriginalQuantization, processor.cc:84-97). */
int gz_set_orig_coeffs(gz_ctx* ctx, const int16_t* coeffs);
/* The same for a YUV 4:2:0 input (jpg.Is420(), processor.cc:814-815): luma blocks on the
 * 8x8 grid, then the two chroma components on the 16x16 grid (the input's MCU padding left
 * out, as OutputImageComponent::CopyFromJpegComponent does, output_image.cc:211-230).  The
 * context's frame becomes 4:2:0. */
int gz_set_orig_coeffs_420(gz_ctx* ctx, const int16_t* coeffs);
/* OutputImage::Downsample (output_image.cc:304-340) as Processor::DownsampleImage calls it
 * (processor.cc:97-104; use_silver_screen == false) on the ORIGINAL coefficients of a 4:4:4
 * frame: ToFloatPixels (:99-121) of the three components, PreProcessChannel
 * (preprocess_downsample.cc:157-279) on V, then on U -- sharpen the channel where the image
 * is red and dark, blur it where it is smooth -- and SetDownsampledCoefficients (:265-300) of
 * U and V by 2 x 2.  Luma is kept.  The context's frame becomes 4:2:0; coeffs_out (may be NULL)
 * receives the new original, nb + 2*nbc blocks.  The caller skips the call for a greyscale
 * image, as the reference does (:305-308). */
int gz_downsample(gz_ctx* ctx, int16_t* coeffs_out);
/* The use_silver_screen branch of OutputImage::Downsample (output_image.cc:309-318) for a caller that
 * has RGBToYUV420's planes already: y, u, v are the three w x h planes it returned
 * (preprocess_downsample.cc:452-476) for OutputImage::ToSRGB() = gz_quantize(NULL) + gz_reconstruct of
 * the 4:4:4 original -- from the reference's own function, or from guetzli_amd/host/silver_screen.cc,
 * the host restatement (twenty rounds of libm pow()) the tests keep as their yardstick.  The encoder
 * itself calls gz_downsample_silver below, which computes the planes on the device.  All three
 * components become SetDownsampledCoefficients of their plane -- luma by 1 x 1, chroma by
 * 2 x 2 -- and the context's frame 4:2:0, as after gz_downsample. */
int gz_downsample_planes(gz_ctx* ctx, const float* y, const float* u, const float* v,
                         int16_t* coeffs_out);
/* The whole use_silver_screen branch on the device: the candidate's pixels are those of the unquantised original
 * (ToSRGB of CopyFromJpegData's image), RGBToYUV420 runs as kernels (csrc/gz_kernels_silver.h: an init pass and twenty
 * rounds, one thread per 2 x 2 cell), and the three components become SetDownsampledCoefficients of its planes, as
 * above.  Bit-identical to the host form: every float(pow()) of the reference is evaluated by the device's pow
 * together with a proof that glibc's pow rounds to the same float (gz_pow_to_float, csrc/gz_math.h); the cells that
 * hold an evaluation without that proof -- about 5 in 10^4 per pass -- are redone by this library's host code with
 * libm and patched in before the next pass.  Preconditions, frame and error behaviour as gz_downsample_planes: a
 * failed call leaves the 4:4:4 frame without an original.  counters (may be NULL): [0] = cell-passes evaluated
 * (cells x 21), [1] = cell-passes redone on the host. */
int gz_downsample_silver(gz_ctx* ctx, int16_t* coeffs_out, uint64_t counters[2]);
/* Current frame: chroma subsampling factor (1 or 2), luma blocks, blocks per chroma
 * component.  Any pointer may be NULL. */
int gz_frame_layout(gz_ctx* ctx, int* chroma_factor, int* luma_blocks, int* chroma_blocks);

/* Candidate := original, then OutputImage::ApplyGlobalQuantization(q)
 * (output_image.cc:232-243,342-346; Quantize quantize.h:24-29).  This is the coefficient
 * side of Processor::TryQuantMatrix (processor.cc:298-307).  q == NULL means all ones
 * (plain CopyFromJpegData).  coeffs_out (may be NULL) receives the candidate's
 * coefficients for the host JPEG writer. */
int gz_quantize(gz_ctx* ctx, const int* q, int16_t* coeffs_out);

/* Replace the whole candidate / individual candidate blocks with host data
 * (OutputImageComponent::SetCoeffBlock, output_image.cc:123-132).  block_index[i] =
 * by*bw + bx, all distinct; blocks holds n * 3 * 64 int16 (component-major per block:
 * Y,Cb,Cr). */
int gz_set_coeffs(gz_ctx* ctx, const int16_t* coeffs);
/* (4:4:4 frames only) */
int gz_set_coeff_blocks(gz_ctx* ctx, const int32_t* block_index, int n,
                        const int16_t* blocks);
int gz_get_coeffs(gz_ctx* ctx, int16_t* coeffs_out);
/* Single-coefficient form of SetCoeffBlock: candidate[pos[i]] = val[i] for n distinct
 * positions in the frame's coefficient array: pos = (first block of component c + block)*64 + k
 * (what one phase-B iteration changes). */
int gz_apply_coeff_edits(gz_ctx* ctx, const int32_t* pos, const int16_t* val, int n);

/* Candidate -> pixels, for parity checks and for callers that want the decoded image:
 * OutputImage::ToSRGB (output_image.cc:411-425) and ToLinearRGB (:427-440).
 * srgb: w*h*3 uint8 or NULL; linear: 3 planes of w*h float or NULL. */
int gz_reconstruct(gz_ctx* ctx, uint8_t* srgb, float* linear);

/* Device-resident output ----------------------------------------------------------
 * The decoded pixels as a strided image in DEVICE memory of the caller's (a tensor a model, a metric or the next
 * stage reads): element (y, x, c) of the w x h x 3 image is data[y*stride_y + x*stride_x + c*stride_c], strides in
 * ELEMENTS -- HWC, CHW, cropped views inside a larger tensor, any element alignment of the base.  One kernel
 * (k_emit_rgb, the mirror of the ingest kernel) converts the packed bytes of OutputImage::ToSRGB
 * (output_image.cc:411-425) and writes exactly the w*h*3 elements of the image: what lies between them stays as it is.
 * Element of a byte b: GZ_DT_U8 b; GZ_DT_U16 b * 257 (its high byte is b: the input rule gives b back); GZ_DT_F32
 * (float)b / 255.0f, the IEEE quotient (not b * (1/255.f)); GZ_DT_F16 / GZ_DT_BF16 that float rounded to nearest, ties to
 * even.  Under the input side's byte rule every such element is b again.
 * GZ_E_ARG (before any device call): NULL out or data, a wrong struct_size, an unknown dtype, a negative stride, an
 * extent whose last element offset does not fit 62 bits, and strides under which two of the w*h*3 elements would share
 * an address: with the three (stride, count) pairs ordered by stride, every stride must be at least the stride times
 * the count of the pair before it, and at least 1 -- a stride of 0 is an input convenience and an output error.  (A
 * dimension of one element -- h or w of 1 -- addresses nothing: its stride is not looked at.)
 * The memory must be device memory of that device that a kernel may write (or managed / mapped page-locked memory),
 * its extent inside its allocation: an ordinary host pointer is GZ_E_ARG, not a fault.
 * Stream contract, both directions: consumer_stream is the hipStream_t that used the memory before the call and
 * reads it afterwards.  The library's stream first waits for an event recorded there (a caching allocator may have
 * handed the memory out while earlier work of that stream still uses it), and behind the kernel that stream waits for
 * an event recorded on the library's: work enqueued on it after the call sees the pixels, with no host
 * synchronisation of the consumer.  NULL: the call synchronises its own stream before it returns, and the memory must
 * not be in use when it starts.  (The context-free entries wait for their own work in either case -- their temporaries
 * go back to the pool -- gz_reconstruct_device with a consumer stream returns behind the enqueue.) */
typedef struct gz_device_output {
  int struct_size;            /* sizeof(gz_device_output) */
  int dtype;                  /* GZ_DT_U8 / GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 / GZ_DT_U16 */
  void* data;                 /* device address of element (0,0,0) */
  int64_t stride_y, stride_x, stride_c;   /* elements */
  void* consumer_stream;      /* hipStream_t that used the memory before and reads it after; NULL = none */
} gz_device_output;
/* guetzli::DecodeJpegToRGB's arithmetic (jpeg_data_decoder.cc:45-54: OutputImage::ToSRGB of CopyFromJpegData's image)
 * without a context: coeffs = DEQUANTISED coefficients in host memory, in the frame layout of this header
 * ([3][nb][64] for chroma_factor 1; nb + 2*nbc blocks for chroma_factor 2), written into out.  0 < w, h < 65536 and
 * gz_create's block limit; no lower bound: a 1 x 1 image decodes.  Temporaries (the coefficients, the chroma samples,
 * 3*w*h bytes) come from the device pool, all of them or none: GZ_E_NOMEM leaves nothing behind. */
int gz_decode_coeffs_device(int device, const int16_t* coeffs, int w, int h, int chroma_factor,
                            const gz_device_output* out);
/* The same into packed host bytes w*h*3: what gz_reconstruct returns as srgb, without a context. */
int gz_decode_coeffs(int device, const int16_t* coeffs, int w, int h, int chroma_factor, uint8_t* host_rgb_out);
/* The candidate of a context, as gz_reconstruct's srgb, into out (the context's w and h). */
int gz_reconstruct_device(gz_ctx* ctx, const gz_device_output* out);

/* A baseline scan read on the device ----------------------------------------------------
 * The entropy-coded segment of a sequential 8-bit JPEG whose ONE scan names all components in frame order -- one
 * component, or three sampled 4:4:4 or 4:2:0 -- with no restart interval, decoded by a self-synchronising parallel
 * Huffman decoder (gz_kernels_scandec.h) into DEQUANTISED coefficients in the frame layout of this
 * header: what the host reader's block loop, its range checks and DecodedCoeffs' dequantisation produce, or a status
 * that says the host must read the scan itself.
 *   data / len: from the first byte behind the SOS header to the END OF THE FILE (the reader's view of where the
 *     entropy-coded data end depends on it: the first 0xff that no 0x00 follows, or two bytes before the end);
 *     3 <= len < 2^28.
 *   dc[c] / ac[c]: component c's tables as a DHT holds them, 16 counts and the values; quant[c]: its quantisers in
 *     natural (row-major) order, 1 .. 65535.  Only the first ncomp entries are read.
 *   subseq_bytes: bytes of the stream per lane, a multiple of 4 in [16, 1024], 0 = 64; max_sync_rounds: launches of the
 *     inter-workgroup synchronisation at the most, > 0, 0 = 16.
 * A status other than GZ_SCAN_DECODED is not an error: the call returns GZ_OK, has written nothing, and the caller
 * falls back.  GZ_E_ARG (before any device call): a wrong struct_size, NULL data, len, subseq_bytes or max_sync_rounds
 * out of range, ncomp other than 1 or 3, chroma_factor other than 1 or 2 (2 with one component), w or h outside
 * 1 .. 65535 or more than 2^21 blocks in a component, a quantiser outside 1 .. 65535, table counts the reader's
 * ProcessDHT would refuse. */
#define GZ_SCAN_DECODED 0
#define GZ_SCAN_NOT_CONVERGED 1   /* the lanes' states still changed after max_sync_rounds launches */
#define GZ_SCAN_BAD_SYMBOL 2      /* a code that does not exist, a DC category above 11, an end-of-band run */
#define GZ_SCAN_RUN_PAST_BAND 3   /* an AC run past position 63 */
#define GZ_SCAN_DC_RANGE 4        /* a DC value that is no int16 */
#define GZ_SCAN_COEFF_RANGE 5     /* an AC category above 11, or a dequantised coefficient that is no int16 */
#define GZ_SCAN_ENDS_EARLY 6      /* a bit consumed that the stream does not have */
typedef struct gz_huffman_spec {
  uint8_t counts[16];         /* codes of length 1 .. 16 */
  uint8_t values[256];
} gz_huffman_spec;
typedef struct gz_scan {
  int struct_size;            /* sizeof(gz_scan) */
  int w, h, ncomp, chroma_factor;
  const uint8_t* data;        /* host memory */
  uint64_t len;
  gz_huffman_spec dc[3], ac[3];
  int quant[3][64];
  int subseq_bytes, max_sync_rounds;
} gz_scan;
typedef struct gz_scan_result {
  int status;                 /* GZ_SCAN_* */
  int subsequences;           /* lanes */
  int sync_rounds;            /* launches of the inter-workgroup synchronisation */
  int reserved;
  uint64_t end_offset;        /* GZ_SCAN_DECODED: where BitReader::Finish would leave the parser, from `data` (but see
                                 below: data ending ff 00 xx) */
} gz_scan_result;
/* One exception to end_offset: where the third- and second-last bytes of `data` are ff 00 -- a stuffed pair across the
 * reader's first stop, two bytes before the end of the file -- BitReader::Finish does not undo its NextByte and leaves the
 * parser one byte further on than the data it consumed, or refuses a scan that consumed the ff.  The coefficients are
 * right, end_offset is the end of the data consumed: a caller that needs the reader's own position reads such a stream
 * on the host, as the library's own driver does (OfferScan, host/jpeg_reader.cc).
 * host_coeffs: (nb + 2 * nbc) * 64 int16 on the host, written only on GZ_SCAN_DECODED (a one-component scan leaves the
 * two chroma components zero). */
int gz_decode_scan(int device, const gz_scan* scan, int16_t* host_coeffs, gz_scan_result* result);
/* ... and on GZ_SCAN_DECODED the pixels of those coefficients into `out`, the coefficients never leaving the device:
 * gz_decode_coeffs_device's arithmetic, ownership, stream contract and argument checks. */
int gz_decode_scan_device(int device, const gz_scan* scan, const gz_device_output* out, gz_scan_result* result);
/* The reader's own result, for an encode of JPEG input (host/processor.h: Process(..., EntropyOptions)): the same
 * decoder with its last two passes in their INPUT mode.  The values are QUANTISED, as coded -- no multiplication, so
 * GZ_SCAN_COEFF_RANGE is left for an AC category above 11 -- and EVERY block of the scan is stored, the MCU padding
 * included.  total = mcu_cols * mcu_rows * (1, 3 or 6 blocks an MCU); the components lie one after the other, each
 * [height_in_blocks][width_in_blocks][64] in natural order on its grid padded to whole MCUs: of a 4:2:0 scan
 * (2 mcu_cols) x (2 mcu_rows) blocks for component 0 and mcu_cols x mcu_rows for the other two, otherwise mcu_cols x
 * mcu_rows for each (mcu_cols = ceil(w / (8 chroma_factor)), mcu_rows likewise).  A one-component scan stores one
 * component.
 * host_coeffs: total * 64 int16 on the host, written only on GZ_SCAN_DECODED; *large_coeff = 1 if CheckJpegSanity would
 * refuse the stream -- |value * quant[c][k]| > 4096 for any stored coefficient, the padding's included; 4096 passes --
 * else 0, written only on GZ_SCAN_DECODED.  Arguments, statuses, end_offset, ownership and stream contract are
 * gz_decode_scan's; GZ_E_ARG also for a NULL host_coeffs or large_coeff. */
int gz_decode_scan_input(int device, const gz_scan* scan, int16_t* host_coeffs, int* large_coeff, gz_scan_result* result);

/* Image pairs: the butteraugli distance of two images, and its map on the device --------
 * A context compares its original with JPEG candidates of it (gz_compare, below).  These entries compare it with ANY
 * image of its size: the context's original is the reference (butteraugli's rgb0), `other` the distorted image (rgb1).
 * The metric is not symmetric.  The chain is gz_compare's from its second kernel on -- OpsinDynamicsImage,
 * SeparateFrequencies, DiffmapPsychoImage against the original's psycho image, which gz_create computed once -- so
 * distance and map are, bit for bit, ButteraugliComparator's of the two images' 8-bit samples.
 *
 * gz_device_map: where a distance map goes, a strided w x h image in DEVICE memory: element (y, x) is
 * data[y*stride_y + x*stride_x], strides in ELEMENTS, of float32, float16 or bfloat16.  One kernel (k_emit_map)
 * converts the context's float plane and writes exactly the w*h elements: what lies between them stays as it is.
 * GZ_DT_F32 is the map bit for bit; GZ_DT_F16 / GZ_DT_BF16 round to nearest, ties to even, over the whole float32
 * domain (subnormal results, overflow to infinity, NaN stays NaN).
 * GZ_E_ARG (before any device call): NULL data, a wrong struct_size, a dtype other than those three, a negative stride,
 * an extent whose last offset does not fit 62 bits, strides under which two elements share an address
 * (gz_device_output's rule: a stride of 0 is an error; the stride of a dimension of one element is not looked at).
 * The memory must be device memory of the context's device (or managed / mapped page-locked memory), its extent
 * inside its allocation: an ordinary host pointer is GZ_E_ARG, not a fault.
 * consumer_stream: as gz_device_output's, in both directions.  With one, a call does not wait for the map on the
 * host: work enqueued on that stream after the call sees it. */
typedef struct gz_device_map {
  int struct_size;            /* sizeof(gz_device_map) */
  int dtype;                  /* GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 */
  void* data;                 /* device address of element (0,0) */
  int64_t stride_y, stride_x; /* elements, >= 0, no two elements at one address */
  void* consumer_stream;      /* hipStream_t that used the memory before and reads it after; NULL = none */
} gz_device_map;
/* gz_compare_device_pixels: `other` is a device-resident image of the context's w x h, described and checked as
 * gz_set_rgb_device_pixels' (every dtype, alpha over a background, the producer's stream is waited for on the device);
 * its bytes are those the ingest kernel makes of it -- what an encode of `other` would read.  *distance receives the
 * image maximum, as gz_compare returns it; map (may be NULL) receives the distance map.  The call synchronises for the
 * distance in every case; with map->consumer_stream it does not wait for the map on the host.
 * Afterwards gz_block_weights (use_distmap) speaks of THIS comparison.  The candidate, the original, its coefficients
 * and the frame (4:4:4 or 4:2:0) stay as they were: the next gz_compare of the candidate returns what it would have
 * returned.  GZ_E_STATE between gz_compare_begin and gz_compare_end, and while an order or a descent of phase B is in
 * flight.  A failed call leaves the context valid; no later call trusts what it may have half written.
 * gz_compare_rgb: the same for packed host bytes w*h*3; host_distmap (may be NULL) receives the map, w*h floats.
 * gz_distmap_device: the map of the LAST comparison that stored one -- gz_compare with distmap != NULL, the two entries
 * above called with a map, any comparison under gz_config.store_distmap -- written into map; a coefficient
 * candidate's map stays on the device this way.  GZ_E_STATE if the last comparison stored none. */
int gz_compare_device_pixels(gz_ctx* ctx, const gz_device_pixels* other, float* distance, const gz_device_map* map);
int gz_compare_rgb(gz_ctx* ctx, const uint8_t* host_rgb, float* distance, float* host_distmap);
int gz_distmap_device(gz_ctx* ctx, const gz_device_map* map);

/* Heat maps: butteraugli's colour picture of a distance map, on the device -------------
 * CreateHeatMapImage (butteraugli.cc:1979-1992): every distance through ScoreToRgb (:1938-1975) with the thresholds
 * good and bad, written by one kernel (k_emit_heat) into a gz_device_output -- a strided w x h x 3 image of any of its
 * five element types, described, checked and ordered on streams exactly as for the decoded pixels above; the element
 * of a byte is the same.  The bytes are the reference's for every finite distance, both zeros, negatives (black) and
 * +infinity (white); for NaN, where the reference is undefined, they are unspecified.  ScoreToRgb's arithmetic runs in
 * FP64 in the reference's order; its (uint8_t)(255 * pow(v, 0.5) + 0.5) is answered from 255 thresholds that the HOST's
 * libm yields once per process.  Should that libm's pow fail the table's monotonicity check, every
 * entry here returns GZ_E_STATE (gz_last_error says why) and nothing else is affected.
 * GZ_E_ARG (before any device call): gz_device_output's, and thresholds that are not 0 < good < bad < infinity.
 * gz_butteraugli_fuzzy_class / _inverse: ButteraugliFuzzyClass / ButteraugliFuzzyInverse (butteraugli.cc:1903-1934) with
 * the host's exp; no device call.  The reference's tool draws its heat maps with good = inverse(1.5), bad = inverse(0.5).
 * gz_heatmap_device: the heat map of the map gz_distmap_device would write.  GZ_E_STATE if the last comparison stored
 * none, and while a Compare or phase-B work of the context is in flight.  No claim of the context changes.
 * gz_compare_device_pixels_heat: gz_compare_device_pixels with a heat map of the comparison into `heat` (may be NULL:
 * then it IS gz_compare_device_pixels).  Asking for a heat map stores the distance map, with or without `map`.
 * gz_heatmap_from_map_device: without a context, the heat map of a float32 plane in the caller's device memory,
 * element (y, x) at map[y*pitch + x], pitch >= w in floats, 0 < w, h < 65536.  The plane must be complete on
 * out->consumer_stream (without one: when the call starts).  Temporaries come from the device pool, all or none; the
 * call waits for its own work. */
double gz_butteraugli_fuzzy_class(double score);
double gz_butteraugli_fuzzy_inverse(double seek);
int gz_heatmap_device(gz_ctx* ctx, double good, double bad, const gz_device_output* out);
int gz_compare_device_pixels_heat(gz_ctx* ctx, const gz_device_pixels* other, float* distance, const gz_device_map* map,
                                  const gz_device_output* heat, double good, double bad);
int gz_heatmap_from_map_device(int device, const float* map, int w, int h, int pitch, double good, double bad,
                               const gz_device_output* out);

/* Linear float images: ButteraugliInterface on the device -------------------------------
 * The entries above compare 8-bit sRGB samples: every element is rounded to the byte an encode would read.  These take
 * what the reference's documented entry takes -- ButteraugliInterface(rgb0, rgb1, diffmap, diffvalue), butteraugli.h:44-79
 * and butteraugli.cc:1819-1878: three planes of LINEAR light, raw intensity 0..255, as floats -- from device memory, with
 * nothing rounded and nothing gamma-decoded.  Two images that differ by less than a byte step have a distance.
 * The images are gz_device_pixels: dtype GZ_DT_F32, GZ_DT_F16 or GZ_DT_BF16, alpha NULL, background ignored; strides, the
 * producer's stream and where the memory must live as for gz_set_rgb_device_pixels.  One kernel (k_ingest_linear) writes
 * the planes.  The value of an element x is  v = (float)x * scale  -- one float32 multiplication; scale = 1 for data in
 * 0..255, 255 for data in [0, 1] -- and then: NaN and everything below 0 become 0, everything above 255 (+infinity too)
 * becomes 255.  Inside [0, 255] nothing is altered and distance and map are the reference's bit for bit; outside it the
 * reference is outside its documented domain (butteraugli.h:52-56) and this clamp is a deliberate difference (DESIGN.md
 * 3.10).  `clamped` (may be NULL) receives the number of elements the clamp altered.
 * GZ_E_ARG (before any device call): gz_device_pixels' own, any other dtype, alpha != NULL, a scale that is not finite
 * and > 0; for map and heat what gz_compare_device_pixels_heat refuses.
 * gz_create_from_device_linear: gz_create_from_device_pixels for such an original, w, h >= 8, with the target 1 (which
 *   only scales gz_block_weights).  The context is a LINEAR
 *   one: it has no 8-bit pixels and no coefficients of its original, so the entries that read them -- gz_encode_rgb,
 *   gz_quantize, gz_downsample*, gz_apply_candidate_steps, gz_block_zeroing_orders*, gz_compare_blocks,
 *   gz_compare_block_pixels -- return GZ_E_STATE (gz_last_error says why).  Every pair entry works on it:
 *   gz_compare_device_pixels of an 8-bit image against a linear original compares that image's table-linearised bytes
 *   with it.  gz_set_rgb* give the context an 8-bit original again.
 * gz_set_linear_device: replaces the original of ANY context by a linear image of its size; the context is a linear
 *   one from then on (from the call's first write: after a failed call too).  GZ_E_STATE while work is in flight.
 * gz_compare_device_linear: gz_compare_device_pixels_heat for a linear `other` (rgb1), on every context, under the
 *   same state rules and stream contracts; map, heat and clamped may be NULL.
 * gz_butteraugli_linear: ButteraugliInterface itself, without a context: ref is rgb0, other rgb1, any 1 <= w, h < 65536
 *   within a context's limits.  Under 8 pixels in a dimension both images are extended to 8 by replicating their border,
 *   xborder = (8 - w) / 2 in integers (ButteraugliDiffmap, :1825-1855); map and heat are of the images' own w x h, and
 *   *distance is the maximum over that window (ButteraugliScoreFromDiffmap of the cropped map).  *clamped counts both
 *   images.  The caller's current device stays current; the temporaries come from the pools and go back to them. */
gz_ctx* gz_create_from_device_linear(int device, int w, int h, const gz_device_pixels* img, float scale, int* err);
int gz_set_linear_device(gz_ctx* ctx, const gz_device_pixels* img, float scale);
int gz_compare_device_linear(gz_ctx* ctx, const gz_device_pixels* other, float scale, float* distance,
                             const gz_device_map* map, const gz_device_output* heat, double good, double bad,
                             uint64_t* clamped);
int gz_butteraugli_linear(int device, int w, int h, const gz_device_pixels* ref, const gz_device_pixels* other,
                          float scale, float* distance, const gz_device_map* map, const gz_device_output* heat,
                          double good, double bad, uint64_t* clamped);

/* Batches: N image pairs of one size through ONE Compare chain --------------------------
 * gz_compare_device_pixels answers one pair per call and enqueues the chain's ~18 launches for it; below 0.25 MPix
 * those launches cost more than their work.  gz_butteraugli_batch compares n pairs of w x h images with the launches of
 * one: every kernel of the chain has a batched form whose grid carries the image index.  Context-free,
 * as gz_butteraugli_linear: a context lives for the call, temporaries come from the pools and go back to them, the
 * caller's current device stays current, and the call waits for its own work before it returns.
 * gz_device_batch: n strided images in device memory, element (i, y, x, c) at data[i*stride_n + y*stride_y + x*stride_x
 * + c*stride_c], strides in ELEMENTS and >= 0 (stride_n = 0: the same image n times; stride_c = 0: grey).  The byte of an
 * element is gz_device_image's (integers pass, floats x 255 rounded to nearest even and clamped): the bytes compared
 * are the bytes an encode would read.  producer_stream is waited for on the device.
 * gz_device_map_batch: n strided maps, element (i, y, x) at data[i*stride_n + y*stride_y + x*stride_x], gz_device_map's
 * value rule; exactly the n*h*w elements are written.  consumer_stream as gz_device_map's, in both directions.
 * ref holds n_ref images: n (pair i is ref i against other i), or 1 -- ONE reference for all, whose planes are computed
 * once.  distances: n contiguous float32 in DEVICE memory, 4-byte aligned; host_distances (may be NULL) receives them too.
 * maps may be NULL.  Distance and map of pair i are, bit for bit, what gz_create_from_device(ref i) followed by
 * gz_compare_device_pixels(other i, map i) gives.
 * scratch_cap_bytes (0: 2 GiB): the most device memory the call's image arenas may take -- 43 float planes per image,
 * 172 bytes per pixel.  More images than fit (or than 21845, the grid's limit) run as chunks of as many as fit, one at
 * the least; no result depends on the chunking.
 * GZ_E_ARG (before any device call): a NULL ref, other or distances, a wrong struct_size, n < 1, n_ref not 1 or n, w or
 * h < 8 or >= 65536, w*h >= 1500000 (larger images gain nothing: use a context per reference), an unknown dtype, a
 * negative stride, an extent beyond 62 bits, a misaligned distances; for maps, strides under which two of the n*h*w
 * elements share an address (stride_n = 0 with n > 1 among them).  Memory the device cannot reach: GZ_E_ARG, as for the
 * other entries.  After a failed call the caller's tensors hold unspecified values in their elements, and what lies
 * between their elements is untouched. */
typedef struct gz_device_batch {
  int struct_size;            /* sizeof(gz_device_batch) */
  int dtype;                  /* GZ_DT_U8 / GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 */
  const void* data;           /* device address of element (0,0,0,0) */
  int64_t stride_n, stride_y, stride_x, stride_c;   /* elements, >= 0 */
  void* producer_stream;      /* hipStream_t that wrote the data; NULL = it is complete when the call starts */
} gz_device_batch;
typedef struct gz_device_map_batch {
  int struct_size;            /* sizeof(gz_device_map_batch) */
  int dtype;                  /* GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 */
  void* data;                 /* device address of element (0,0,0) */
  int64_t stride_n, stride_y, stride_x;   /* elements, >= 0, no two elements at one address */
  void* consumer_stream;      /* hipStream_t that used the memory before and reads it after; NULL = none */
} gz_device_map_batch;
int gz_butteraugli_batch(int device, int w, int h, int n, const gz_device_batch* ref, int n_ref,
                         const gz_device_batch* other, float* distances, float* host_distances,
                         const gz_device_map_batch* maps, size_t scratch_cap_bytes);

/* Batches: N baseline scans of one frame size through the launches of ONE device decode -
 * gz_decode_scan_device costs per call, not per byte: its kernels are latency-bound, and the host reads a word per
 * synchronisation round and the verdict at the end.  gz_decode_scan_batch_device decodes n scans of ONE w, h, ncomp and
 * chroma_factor with one launch of every kernel for all of them: the streams lie in one buffer, every
 * stream's lanes are padded to whole workgroups, the host reads n words per round and n verdicts at the end, and the
 * pixels of the scans that decoded leave through batched forms of the reconstruction and emit kernels.
 * gz_device_output_batch: n strided images in device memory that are WRITTEN -- gz_device_batch's fields, the number of
 * images, and gz_device_output's rules: element (i, y, x, c) at data[i*stride_n + y*stride_y + x*stride_x + c*stride_c], strides in
 * ELEMENTS and >= 0, no two elements of the n * h * w * 3 at one address; every gz_device_output dtype;
 * consumer_stream as gz_device_output's, in both directions.
 * scans[i] (tables, quantisers, data, len its own; subseq_bytes and max_sync_rounds must be the same in all of them)
 * fills image slots[i] of `out`, 0 <= slots[i] < out->n, no slot twice.  results[i] is exactly what
 * gz_decode_scan_device(device, &scans[i], image slots[i], ...) writes -- status, subsequences, sync_rounds (the rounds
 * THIS stream needed: a property of the stream, not of the batch), end_offset -- and so are the pixels; a scan whose
 * status is not GZ_SCAN_DECODED has no byte of its image written, and the other scans do not depend on it.
 * scratch_cap_bytes (0: 2 GiB): the most device memory the call's temporaries may take.  Per image: the stream's bytes,
 * 9.5 KiB of tables, 28 bytes per lane (a lane is subseq_bytes of the stream, padded to 256 lanes), 2 bytes per block of
 * the scan, and the frame: 128 bytes per coefficient block (192 B per pixel at 4:4:4, 96 at 4:2:0), 3 bytes per pixel
 * packed, at 4:2:0 another 0.5.  More scans than fit run as chunks of as many as fit, with the same results; a scan
 * that does not fit alone is GZ_E_ARG.  Temporaries come from the device pool, all of a chunk's or none.
 * GZ_E_ARG (before any device call): gz_decode_scan's per scan; n < 1, NULL scans, slots, out or results, scans that
 * differ in w, h, ncomp, chroma_factor, subseq_bytes or max_sync_rounds, a slot out of range or named twice, a wrong
 * struct_size, an unknown dtype, a negative stride, aliasing strides.  Any other error: the results of the scans that
 * had no verdict yet are left at "no verdict" (status GZ_SCAN_NOT_CONVERGED, sync_rounds 0) and their images hold
 * unspecified values in their elements; the caller reads those scans itself. */
typedef struct gz_device_output_batch {
  int struct_size;            /* sizeof(gz_device_output_batch) */
  int dtype;                  /* GZ_DT_U8 / GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 / GZ_DT_U16 */
  void* data;                 /* device address of element (0,0,0,0) */
  int64_t stride_n, stride_y, stride_x, stride_c;   /* elements, >= 0, no two elements at one address */
  void* consumer_stream;      /* hipStream_t that used the memory before and reads it after; NULL = none */
  int n;                      /* images, >= 1 */
} gz_device_output_batch;
int gz_decode_scan_batch_device(int device, int n, const gz_scan* scans, const int* slots,
                                const gz_device_output_batch* out, gz_scan_result* results,
                                size_t scratch_cap_bytes);

/* Masking: Mask, the opsin image and the quantisation field, on the device ---------------
 * What butteraugli.h offers beside the distance: OpsinDynamicsImage(rgb), the XYB image; Mask(xyb0, xyb1, &mask,
 * &mask_dc) (butteraugli.cc:1741-1817), the visual-masking images that say where an error of a given size is visible;
 * and ButteraugliAdaptiveQuantization(xsize, ysize, rgb, quant) (:1880-1901), the per-pixel field a codec multiplies
 * its step sizes with.  Context-free, as gz_butteraugli_linear: a context lives for the call, the caller's current
 * device stays current, temporaries come from the pools, all or none (GZ_E_NOMEM leaves nothing behind), and the call
 * waits for its own work.  (The context is made with the first image as its original, so that image's psycho image is
 * computed too, though nothing here reads it: DESIGN.md 3.11.)
 * samples: how the elements of a gz_device_pixels become linear planes --
 *   GZ_SAMPLES_SRGB8   as gz_set_rgb_device_pixels reads them: the ingest kernel's bytes (every dtype, alpha over a
 *                      background), linearised by the sRGB table -- what the 8-bit pair entries compare; scale is ignored;
 *   GZ_SAMPLES_LINEAR  as gz_set_linear_device reads them: (float)x * scale, NaN and < 0 -> 0, > 255 -> 255, counted in
 *                      *clamped (may be NULL; 0 for 8-bit samples); float32 / float16 / bfloat16 only.  The clamp is the
 *                      deliberate difference of the linear entries above.
 * gz_opsin_device: OpsinDynamicsImage of the image's linear planes into xyb, a gz_device_output used as a w x h x 3
 *   image of FLOATS: GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16 (GZ_DT_U8 / GZ_DT_U16: GZ_E_ARG).
 * gz_mask_device: Mask(OpsinDynamicsImage(lin0), OpsinDynamicsImage(lin1)); img1 == NULL is the mask of img0 with
 *   itself, what StartBlockComparisons computes for the block search.  mask and mask_dc are float gz_device_outputs as
 *   xyb, each optional, one at least; *clamped counts both images.
 * gz_adaptive_quantization: ButteraugliAdaptiveQuantization to the letter -- Mask applied to the LINEAR planes
 *   themselves (no opsin step: the reference passes rgb as xyb0 and xyb1), plane 1 of `mask` into quant, a gz_device_map.
 *   The image is read as GZ_SAMPLES_LINEAR.  w < 16 or h < 16: GZ_E_ARG (the reference returns false).  Only the Y
 *   plane's half of Mask's first stage runs: half the blurs of gz_mask_device.
 * Sizes: gz_opsin_device and gz_mask_device need w, h >= 8, a context's minimum (GZ_E_ARG below): a limit of this
 *   library, not of the reference.
 * Elements of the outputs: gz_device_map's rule -- GZ_DT_F32 the reference's float bit for bit, GZ_DT_F16 / GZ_DT_BF16
 *   rounded to nearest, ties to even, over the whole float32 domain.  Exactly the image's elements are written: a crop
 *   view's surroundings stay as they are.
 * GZ_E_ARG (before any device call): what gz_set_rgb_device_pixels / gz_set_linear_device refuse of an image, what
 *   gz_device_output / gz_device_map refuse of a destination, an unknown `samples`, an output dtype that is no float,
 *   both mask outputs NULL.  Memory that is not device memory of `device` -- an ordinary host pointer -- is GZ_E_ARG too,
 *   not a fault.
 * Streams: every input's producer_stream is waited for on the device; with an output's consumer_stream, that stream
 *   waits for the output on the device (the call still waits for its own work: its temporaries go back to the pool). */
#define GZ_SAMPLES_SRGB8 0
#define GZ_SAMPLES_LINEAR 1
int gz_opsin_device(int device, int w, int h, const gz_device_pixels* img, int samples, float scale,
                    const gz_device_output* xyb, uint64_t* clamped);
int gz_mask_device(int device, int w, int h, const gz_device_pixels* img0, const gz_device_pixels* img1 /* NULL: img0 */,
                   int samples, float scale, const gz_device_output* mask, const gz_device_output* mask_dc,
                   uint64_t* clamped);
int gz_adaptive_quantization(int device, int w, int h, const gz_device_pixels* img, float scale,
                             const gz_device_map* quant, uint64_t* clamped);

/* Double-precision DCT -----------------------------------------
 * gz_dct_double_blocks: ComputeBlockDCTDouble (inverse == 0) / ComputeBlockIDCTDouble
 * (inverse != 0), dct_double.cc:76-85, on n bare blocks of 64 doubles, in place.
 * gz_component_to_float_pixels: OutputImageComponent::ToFloatPixels with stride 1
 * (output_image.cc:99-121): one 4:4:4 component's coefficients [ceil(w/8)*ceil(h/8)][64]
 * -> out[y*w + x] = float(IDCTDouble + 128).
 * gz_component_set_downsampled: SetDownsampledCoefficients (output_image.cc:265-300):
 * pixels (w*h floats of the full-resolution component) averaged fx x fy, forward
 * DCTDouble, DC - 1024, round() -> int16 coefficients of the subsampled component,
 * ceil(w/(8 fx)) * ceil(h/(8 fy)) blocks (OutputImageComponent::Reset, :40-49).
 * These are the two consumers of dct_double.cc on the reference's YUV420 path
 * (OutputImage::Downsample, :304-340); all three are bit-exact (FP64, no contraction).
 * Context-free: they take a device ordinal. */
int gz_dct_double_blocks(int device, double* blocks, int n, int inverse);
int gz_component_to_float_pixels(int device, const int16_t* coeffs, int w, int h,
                                 float* out);
int gz_component_set_downsampled(int device, const float* pixels, int w, int h, int fx,
                                 int fy, int16_t* coeffs_out);

/* Whole-image distance -----------------------------------------------------------
 * gz_compare: replaces guetzli::ButteraugliComparator::Compare
 * (butteraugli_comparator.cc:63-75) on the current candidate: IDCT + colour + linear
 * (ToLinearRGB), OpsinDynamicsImage, SeparateFrequencies, Malta x6, L2Diff*,
 * SameNoiseLevels, Mask, CombineChannels, CalculateDiffmap, max
 * (butteraugli.cc:799-908,1623-1633).
 *   distance  : distmap_aggregate() (butteraugli_comparator.h:56)          [required]
 *   distmap   : distmap() (h:55), w*h floats                               [may be NULL]
 *   block_max : per-8x8-block maximum of the distance map, nb floats = the first loop
 *               of ComputeBlockErrorAdjustmentWeights (:505-520)           [may be NULL]
 * With distmap == block_max == NULL only 4 bytes cross PCIe. */
int gz_compare(gz_ctx* ctx, float* distance, float* distmap, float* block_max);

/* gz_compare in two halves, so that the caller can do host work (e.g. build the Huffman
 * codes of the same candidate) while the evaluation runs: _begin enqueues it and returns,
 * _end waits and returns distmap_aggregate().  Between them only calls that leave the
 * candidate unchanged are allowed: gz_jpeg_scan (which runs on the context's entropy stream,
 * beside the evaluation), gz_jpeg_scan_keep / _bytes, gz_get_coeffs. */
int gz_compare_begin(gz_ctx* ctx);
int gz_compare_end(gz_ctx* ctx, float* distance);

/* Enqueue `iters` back-to-back Compare evaluations of the current candidate on the
 * context's stream without any host transfer or synchronisation (for HIP-event timing
 * of the resident-in-HBM rate).  The distance of the last one is readable with
 * gz_last_distance after gz_synchronize.  Every one of them is the whole chain, reconstruction included
 * (gz_config.patch_reconstruct does not apply: nothing changes the candidate between them). */
int gz_compare_enqueue(gz_ctx* ctx, int iters);
int gz_last_distance(gz_ctx* ctx, float* distance);
/* Convenience: time `iters` enqueued Compare evaluations with hipEvents recorded on the
 * context's stream; returns total milliseconds. */
int gz_time_compare(gz_ctx* ctx, int iters, float* total_ms);

/* ComputeBlockErrorAdjustmentWeights (butteraugli_comparator.cc:494-558) from the
 * block maxima of the LAST gz_compare (or all-zero if use_distmap == 0, which is what
 * SelectFrequencyMasking does on its first "up" iteration, processor.cc:625-629).
 * block_weight: nb floats, in/out exactly like the reference's vector. */
int gz_block_weights(gz_ctx* ctx, int direction, int max_block_dist, double target_mul,
                     int use_distmap, float* block_weight);
/* The same for blocks of 8*factor x 8*factor pixels (factor_x = factor_y = factor, 1 or 2:
 * the chroma grid of a 4:2:0 frame); block_weight has ceil(w/(8 factor))*ceil(h/(8 factor))
 * entries. */
int gz_block_weights_factor(gz_ctx* ctx, int direction, int max_block_dist, double target_mul,
                            int use_distmap, int factor, float* block_weight);

/* Per-block zeroing search ---------------------------------------------------------
 * gz_block_zeroing_orders: phase A of Processor::SelectFrequencyMasking
 * (processor.cc:554-590) for comp_mask 7 on a 4:4:4 image: for every block,
 * ComputeBlockZeroingOrder (processor.cc:364-467) with CompareBlock
 * (butteraugli_comparator.cc:457-488) evaluated on the device, between the reference's
 * StartBlockComparisons / FinishBlockComparisons (:415-425).  Operates on the current
 * candidate (e.g. after gz_quantize(best_q)) and the original coefficients.
 *   lookahead = Params::zeroing_greedy_lookahead (3), new_model =
 *   Params::new_zeroing_model (processor.h:35-36).
 * Outputs are the reference's CSR arrays: candidate_coeff_offsets[nb+1],
 * candidate_coeffs[], candidate_coeff_errors[] (processor.cc:554-558).  cap = capacity of
 * idx/err in elements (nb*189 always suffices); if too small, GZ_E_ARG is returned and
 * offsets[nb] holds the required size.  err may be NULL: the errors then stay on the device
 * only, where gz_order_build reads them. */
int gz_block_zeroing_orders(gz_ctx* ctx, int lookahead, int new_model, int32_t* offsets,
                            uint8_t* idx, float* err, int cap);
/* The same for any comp_mask of SelectFrequencyMasking (processor.cc:539-590): candidates come
 * from the components in the mask only, and the grid is that of the mask's last component
 * (:546-552).  4:4:4 frame: any mask, the 8x8 grid.  4:2:0 frame: mask 1 (luma; 8x8 grid,
 * chroma pixels fixed) or mask 6 (chroma; ceil(w/16) x ceil(h/16) grid -- every candidate is
 * compared on the up to four 8x8 blocks of its 16x16 area and scored by the largest error,
 * processor.cc:420-430, with the 2x2-subsampled pixel model of
 * OutputImageComponent::UpdatePixelsForBlock, output_image.cc:146-203).  offsets has one
 * entry per block of that grid plus one.  Phase B's order functions below then work on the
 * same grid and mask. */
int gz_block_zeroing_orders_masked(gz_ctx* ctx, int comp_mask, int lookahead, int new_model,
                                   int32_t* offsets, uint8_t* idx, float* err, int cap);
/* Number of CompareBlock evaluations (butteraugli_comparator.cc:457-488) the last
 * gz_block_zeroing_orders* call made -- the unit the search's throughput is reported in
 * (bench.py: evaluations per second). */
int gz_search_evaluations(gz_ctx* ctx, uint64_t* evaluations);
/* Process-wide, since the library was loaded (tests, bench.py): out[0] = Compares whose candidate planes were kept
 * current by the calls that changed the candidate and that skipped the full reconstruction (gz_config.patch_reconstruct),
 * out[1] = those of them that were checked against a full reconstruction (patch_reconstruct == 2), out[2] = Compares in all,
 * out[3] = Compares that also found their opsin image in place (gz_config.opsin_ahead), out[4] = those of them checked. */
int gz_compare_counters(uint64_t out[5]);
/* The per-block form of the seam: Comparator::SwitchBlock + CompareBlock
 * (butteraugli_comparator.cc:427-488; factor_x = factor_y = 1) for n independent pairs of a
 * block position block_xy[i] = {block_x, block_y} and that block's candidate coefficients
 * coeffs[i][3][64] (Y, Cb, Cr; dequantised): out[i] = the distance CompareBlock returns.
 * StartBlockComparisons' mask (:415-421) is computed on first use.  This is what a
 * `guetzli::Comparator` subclass calls from its CompareBlock (tests/integration/ drives the
 * UNMODIFIED reference Processor through it); a search that wants speed batches whole blocks'
 * searches with gz_block_zeroing_orders instead -- one call per block costs a round trip. */
int gz_compare_blocks(gz_ctx* ctx, int n, const int32_t* block_xy, const int16_t* coeffs,
                      double* out);
/* The same for 8x8 windows given by their YCbCr PIXELS -- what CompareBlock reads of the image:
 * OutputImage::ToLinearRGB(xmin, ymin, 8, 8) (butteraugli_comparator.cc:467), i.e.
 * OutputImageComponent::ToPixels (output_image.cc:69-96, edge replication included) of the three
 * components.  This form serves every frame (comparator.h:50-52: SwitchBlock carries
 * factor_x, factor_y): the pixels of a 2x2-subsampled component depend on its neighbours' blocks,
 * which the caller's OutputImage holds.  block_xy: the window's position on the 8x8 luma grid
 * (block_x * factor_x + off_x, block_y * factor_y + off_y); ycc: n x 3 x 64 bytes. */
int gz_compare_block_pixels(gz_ctx* ctx, int n, const int32_t* block_xy, const uint8_t* ycc, double* out);
/* OutputImageComponent::Reset(factor, factor) of the two chroma components (output_image.cc:
 * 32-57) without touching their content: the layout gz_set_coeffs / gz_get_coeffs /
 * gz_set_orig_coeffs* use from now on (1: 4:4:4, 2: 4:2:0).  A change drops the candidate, the
 * original coefficients and the search results; the original PIXELS (gz_create) stay. */
int gz_set_frame(gz_ctx* ctx, int chroma_factor);
/* Host-only helper, exported for tests: the ranked input_order of
 * ComputeBlockZeroingOrder (processor.cc:381-400) for every block, as CSR, by std::sort
 * itself.  gz_block_zeroing_orders ranks on the device. */
int gz_rank_zeroing_candidates(const int16_t* coeffs, const int16_t* orig, int nb,
                               int new_model, int32_t* offsets, uint8_t* idx);
/* Test hook for the device-side ranking (k_rank_candidates sorts every block's candidates
 * with libstdc++'s std::sort permutation): narr arrays of cnt[a] <= 192 keys, keys[a][192];
 * perm[a][i] = index (into array a) of the element std::sort puts at position i. */
int gz_probe_rank_sort(int device, const float* keys, const int32_t* cnt, int narr, uint8_t* perm);

/* Global candidate order of phase B ------------------------------
 * Phase B of SelectFrequencyMasking builds `global_order` = (block, val) for every
 * remaining candidate of every block with a non-zero weight (processor.cc:622-663),
 * std::sort-s it by val (:675-678) and consumes a prefix.  The order lives on the device:
 *
 * gz_order_build: the construction loop (:636-663) over the CSR arrays the last
 *   gz_block_zeroing_orders left on the device.  next_cand = last_indexes (:608),
 *   max_block_error (:607), block_weight = the output of gz_block_weights, nb values each.
 *   *total = global_order.size(), *blocks_to_change as the reference counts it; if
 *   count_below, *below = number of entries with val < limit (what the partition_point of
 *   :690-696 yields on the sorted order).
 * gz_order_upload: replace the device order with n host entries instead.
 * gz_order_partition: one step of libstdc++'s introsort on [lo, hi) of the device order --
 *   std::__unguarded_partition_pivot: median of {lo+1, mid, hi-1} to lo, unguarded Hoare
 *   partition of [lo+1, hi) around it -- with exactly the arrangement and *cut the serial
 *   algorithm gives (ties across blocks are not stable under std::sort and feed the JPEG
 *   bytes).  Requires hi - lo > 3.
 * gz_order_fetch: entries [lo, hi) to the host, 8 bytes each: {int32 block; float val}
 *   (the layout of std::pair<int, float>).
 * The search driver (guetzli_amd/host/lazy_sort.h) refines the leading ranges on the
 * device until they are small, fetches them, and finishes them on the host. */
int gz_order_build(gz_ctx* ctx, int direction, const int32_t* next_cand,
                   const float* max_block_error, const float* block_weight, int count_below,
                   float limit, uint64_t* total, int32_t* blocks_to_change, uint64_t* below);
/* The same with the per-block state kept on the device across iterations:
 * gz_order_reset: max_block_error := 0 (processor.cc:607).
 * gz_order_build_auto: block_weight = ComputeBlockErrorAdjustmentWeights(direction,
 *   max_block_dist, target_mul) of the last gz_compare (all-zero distance map if
 *   use_distmap == 0) computed on the device (butteraugli_comparator.cc:494-558), then the
 *   construction loop as gz_order_build with the device-resident max_block_error.
 * gz_order_advance: max_block_error[i] += block_weight[i] * val_threshold * direction
 *   (processor.cc:754-756) with the weights of the last gz_order_build_auto. */
int gz_order_reset(gz_ctx* ctx);
int gz_order_build_auto(gz_ctx* ctx, int direction, int max_block_dist, double target_mul,
                        int use_distmap, const int32_t* next_cand, int count_below, float limit,
                        uint64_t* total, int32_t* blocks_to_change, uint64_t* below);
/* gz_order_build_auto in two halves, so that the order of the NEXT iteration is constructed on
 * the device right behind the evaluation of the candidate it depends on (gz_compare_begin on
 * the same context: use_distmap is then allowed before gz_compare_end), with no host round
 * trip in between -- processor.cc:607-663 run back to back with :767.  _begin enqueues and
 * returns (next_cand is copied); _end waits and reports what gz_order_build_auto reports.
 * Any other gz_order_build* call drops a pending _begin. */
int gz_order_build_auto_begin(gz_ctx* ctx, int direction, int max_block_dist, double target_mul,
                              int use_distmap, const int32_t* next_cand, int count_below, float limit);
int gz_order_build_auto_end(gz_ctx* ctx, uint64_t* total, int32_t* blocks_to_change, uint64_t* below);
int gz_order_advance(gz_ctx* ctx, float val_threshold, int direction);
/* gz_apply_candidate_steps: the coefficient side of the global loop's steps
 * (processor.cc:704-736) for whole blocks: block blocks[i] advances by counts[i] steps in
 * `direction` from the next_cand the last gz_order_build* call uploaded -- each step zeroes
 * ("up") or restores ("down") the block's next candidate coefficient unless it is
 * "precious" (:722-733).  blocks distinct; the device copy of next_cand is left as uploaded
 * (the next gz_order_build* call brings the caller's). */
int gz_apply_candidate_steps(gz_ctx* ctx, int direction, const int32_t* blocks,
                             const int32_t* counts, int n);
/* What the last gz_apply_candidate_steps did to the AC symbol statistics: ac_delta[3][256] =
 * BuildACHistograms (jpeg_data_writer.cc:255-275) of the image after the steps minus before,
 * raw occurrence counts under the quantiser of the last gz_jpeg_histograms (which must have
 * been called before the steps).  Computed from the touched blocks only, so that the caller's
 * size model (processor.cc:471-525) does not need a recount of the whole image. */
int gz_steps_histogram_delta(gz_ctx* ctx, int32_t* ac_delta);
int gz_order_upload(gz_ctx* ctx, const void* entries, uint64_t n);
int gz_order_partition(gz_ctx* ctx, uint64_t lo, uint64_t hi, uint64_t* cut);
int gz_order_fetch(gz_ctx* ctx, uint64_t lo, uint64_t hi, void* out);
/* A host array of at least `entries` order entries (8 bytes each), page-locked and owned by the
 * context: gz_order_fetch into it (at any offset) is one DMA transfer without the landing copy a
 * pageable destination needs.  The search driver keeps its host copy of the order there.  A call
 * that has to grow the array invalidates the pointer of the call before; gz_destroy frees it. */
int gz_order_host_mirror(gz_ctx* ctx, uint64_t entries, void** out);
/* After gz_order_build_auto_descend_begin ... gz_order_descend_end: the number of leading entries
 * of the order that the device has already written into the host mirror behind the descent (the
 * prefix up to the end of the range the descent ended in, when that range is within `threshold`
 * and the prefix within 2^19 entries; else 0).  They are what gz_order_fetch(ctx, 0, n, mirror)
 * would deliver at that moment: the driver skips that fetch. */
int gz_order_exported(gz_ctx* ctx, uint64_t* entries);
/* The quick-select descent of that sort, decided on the device.  What the global loop needs
 * before its stopping rule can fire (processor.cc:743-746: not before min_coeffs_to_change
 * steps) is the SET of the leading entries of the sorted order; std::sort's introsort reaches
 * it by partitioning the whole order, then the part that holds position `last`, and so on.
 * gz_order_descend runs up to max_levels of exactly those gz_order_partition steps back to back
 * -- on the range [0, n), then on whichever side of the cut holds `last`, while the range has
 * more than `threshold` entries and introsort's depth budget (2 floor(lg n)) lasts -- without
 * the host in between, and reports them: log[3*i] = lo, log[3*i+1] = hi, log[3*i+2] = cut of
 * step i, *levels of them.  Same arrangement, same cuts as the same sequence of
 * gz_order_partition calls.
 * gz_order_descend_begin: the same enqueued behind gz_order_build_auto_begin, before the order's
 *   size is known to the host: `last` is derived on the device as the search driver derives it,
 *   min_coeffs = (int)(per_block * blocks_to_change) (:685-687), capped at n - 1, rounded down
 *   to the entropy-code refresh interval of 10 (:739-741), minus one (0 if that is 0).
 * gz_order_descend_end: its log, after gz_order_build_auto_end, and the `last` it was made
 *   for (meaningful when *levels > 0): a caller that derives another position must not replay it. */
int gz_order_descend(gz_ctx* ctx, uint64_t last, uint64_t threshold, int max_levels,
                     uint64_t* log, int* levels);
int gz_order_descend_begin(gz_ctx* ctx, float per_block, uint64_t threshold, int max_levels);
/* gz_order_build_auto_begin followed by gz_order_descend_begin as ONE call: the same kernels, and
 * one device-to-host transfer for everything the caller waits for afterwards -- the order's size
 * and counters (gz_order_build_auto_end), the descent's log (gz_order_descend_end) and, when the
 * call is made between gz_compare_begin and gz_compare_end, that evaluation's distance
 * (gz_compare_end then only waits): three small copies less on the stream, each a dispatch of its
 * own between the evaluation and the host. */
int gz_order_build_auto_descend_begin(gz_ctx* ctx, int direction, int max_block_dist, double target_mul,
                                      int use_distmap, const int32_t* next_cand, int count_below,
                                      float limit, float per_block, uint64_t threshold, int max_levels);
int gz_order_descend_end(gz_ctx* ctx, uint64_t* log, int cap_levels, int* levels, uint64_t* last);

/* Entropy coding of the candidate -----------------------------------------------------
 * The search needs the exact size of every candidate's JPEG (ScoreJPEG) and the bytes of the
 * winner only.  The candidate's coefficients are resident, so the symbol statistics and the
 * scan are produced on the device; Huffman code construction (ClusterHistograms,
 * BuildHuffmanCode, jpeg_data_writer.cc:158-342) and the marker segments stay on the host.
 *
 * gz_jpeg_histograms: BuildDCHistograms + BuildACHistograms (jpeg_data_writer.cc:241-275)
 * of the candidate quantised by q (int[3][64]; value = coeff / q as in
 * OutputImage::SaveToJpegData, output_image.cc:348-409).  counts: uint32 [2][3][256] =
 * (DC, AC) x component x symbol, raw occurrence counts.  Remembers q for gz_jpeg_scan.
 *
 * gz_jpeg_scan: EncodeScan (:499-536) of the same frame with ncomp (1 or 3) components
 * under the codes depth / code ([2][3][256] each, per component, already resolved through
 * the DC/AC table indexes).  The bit stream stays on the device; *scan_bytes receives its
 * exact length in bytes including the 0x00 stuffed after every 0xFF and the final
 * 1-padding (jpeg_bit_writer.h:31-108).  Codes of used symbols longer than 16 bits can overflow the scan's bound: GZ_E_ARG.  The
 * kernels run on the context's entropy stream, ordered behind whatever put the candidate in
 * place; the call returns after its single synchronisation of that stream.
 *
 * gz_jpeg_scan_begin / _end are the same call in two halves: _begin enqueues the scan on the
 * entropy stream and returns, _end waits for it and returns the length.  Between them the
 * caller may enqueue what gz_compare_begin's contract allows (the evaluation itself, the next
 * order's construction: gz_order_build_auto_begin / gz_order_descend_begin) -- the entropy
 * coder then runs beside the evaluation instead of behind the host code that enqueues it.
 *
 * gz_jpeg_scan_keep snapshots the last scan on the device (the caller's "best so far",
 * processor.cc:139-148); gz_jpeg_scan_bytes downloads the last (kept = 0) or the kept
 * (kept = 1) scan as stuffed bytes. */
int gz_jpeg_histograms(gz_ctx* ctx, const int* q, uint32_t* counts);
/* In a 4:2:0 frame the luma DC statistics depend on whether the chroma components are
 * written (MCU order and padding blocks, output_image.cc:357-404) or not (ncomp == 1: luma
 * alone in raster order): this variant says which.  gz_jpeg_histograms == ncomp 3. */
int gz_jpeg_histograms_ncomp(gz_ctx* ctx, const int* q, int ncomp, uint32_t* counts);
int gz_jpeg_scan(gz_ctx* ctx, int ncomp, const uint8_t* depth, const uint16_t* code,
                 uint64_t* scan_bytes);
int gz_jpeg_scan_begin(gz_ctx* ctx, int ncomp, const uint8_t* depth, const uint16_t* code);
int gz_jpeg_scan_end(gz_ctx* ctx, uint64_t* scan_bytes);
int gz_jpeg_scan_keep(gz_ctx* ctx);
/* Of the last scan: its length in bits (before byte stuffing and padding) and the number of 0xFF
 * bytes it holds, i.e. of 0x00 bytes stuffed: scan_bytes = ceil(bits / 8) + stuffed.  The bit
 * count is a function of the symbol statistics and the code lengths alone (every occurrence costs
 * its code plus its extra bits, jpeg_data_writer.cc:446-497); the host driver derives it that way
 * to bound a candidate's size without coding it, and checks itself against this. */
int gz_jpeg_scan_bits(gz_ctx* ctx, uint64_t* bits, uint64_t* stuffed);
int gz_jpeg_scan_bytes(gz_ctx* ctx, int kept, uint8_t* out, size_t cap, size_t* n);

/* Stage probes (parity tests) -----------------------------------------------------
 * Each runs ONE stage of the pipeline on host-provided input through the same kernels
 * gz_compare uses.  They exist so that tests can localise a divergence; they are not on
 * the hot path.  All planes are w*h floats of a context created for that w,h. */
int gz_probe_blur(gz_ctx* ctx, const float* in, float sigma, float border_ratio,
                  float* out);                                  /* Blur, butteraugli.cc:229 */
int gz_probe_opsin(gz_ctx* ctx, const float* rgb3, float* xyb3); /* :324-366 */
int gz_probe_separate_frequencies(gz_ctx* ctx, const float* xyb3,
                                  float* out10);                /* :489-622; lf3,mf3,hf2,uhf2 */
/* PRECONDITION of gz_probe_diffmap: rgb0_3 must be the linear image (sRGB table of the 8-bit
 * samples) of the context's CURRENT original -- the one given to gz_create or to the last
 * gz_set_rgb.  The probe computes rgb0's band planes itself, but its mask branch is the production
 * one, which reads the original's half of DiffPrecompute that gz_set_rgb computed once per image.
 * With any other rgb0 the call succeeds and the map is wrong (by factors, on every pixel).  To
 * probe another pair, gz_set_rgb its original first. */
int gz_probe_diffmap(gz_ctx* ctx, const float* rgb0_3, const float* rgb1_3,
                     float* diffmap, float* score);             /* :784-908 both sides */
int gz_probe_mask(gz_ctx* ctx, const float* xyb0_3, const float* xyb1_3, float* mask3,
                  float* mask_dc3);                             /* Mask, :1741-1817 */
/* k_emit_map alone, without a context: host_plane (w*h floats of the caller's choosing, 0 < w, h < 65536; any bit
 * pattern) is uploaded to a plane from the device pool and written into map as gz_distmap_device writes a distance
 * map.  The call waits for its own work. */
int gz_probe_emit_map(int device, const float* host_plane, int w, int h, const gz_device_map* map);
/* k_emit_heat alone: host_plane as above, written into out as gz_heatmap_from_map_device writes a device plane.
 * gz_probe_heat_thresholds: the table the kernel searches, thr255[k - 1] = the least double v for which the host's
 * (uint8_t)(255 * pow(v, 0.5) + 0.5) is >= k; GZ_E_STATE where the host's pow fails the table's check.  No device call. */
int gz_probe_emit_heat(int device, const float* host_plane, int w, int h, double good, double bad,
                       const gz_device_output* out);
int gz_probe_heat_thresholds(double* thr255);
/* The context's three linear planes as they are now, [3][h][w] floats: after gz_create_from_device_linear /
 * gz_set_linear_device (and gz_set_rgb*) the original's, after a pair comparison the other image's. */
int gz_probe_linear_planes(gz_ctx* ctx, float* planes3);
/* Block kernels on bare 64-element blocks (n blocks each). */
int gz_probe_idct_blocks(int device, const int16_t* blocks, int n, uint8_t* out);
int gz_probe_fdct_blocks(int device, int16_t* blocks, int n);
/* Arithmetic self-check of the device: IEEE float/double divide & sqrt, conversions and
 * the absence of FMA contraction, on host-supplied operands.  op: 0 a/b (f32),
 * 1 sqrt(a) (f32), 2 a/b (f64), 3 sqrt(a) (f64), 4 a*b+c unfused (f32), 5 a*b+c unfused
 * (f64), 6 (float)a for double a.  Arrays hold n elements of the operand type
 * (out of (float)a is float). */
int gz_probe_arith(int device, int op, const void* a, const void* b, const void* c,
                   void* out, int n);

/* The per-pixel functions of the butteraugli chain (csrc/gz_math.h, quant_div of the entropy
 * kernels) evaluated element-wise on the device, on host-supplied operands: the device-only forms
 * (two quotients from one hardware reciprocal, Malta's branch-free "diffs" value with its
 * wavefront-uniform rare path, the division by a constant through two fused multiply-adds) and
 * every value branch can be compared with the plain C++ statement sequences at values no image
 * produces.  a, b, c: n floats each unless stated; p: the op's np constants; out: n floats per
 * output, output-major (out[k * n + i]).  256 consecutive elements share a workgroup, 64 a
 * wavefront.
 *   op                         inputs                          p                             outputs
 *   GZ_MATH_DIV2_SHARED        a = n0, b = n1, c = d           -                             n0/d, n1/d
 *   GZ_MATH_MALTA_DIFF         a, b                            norm2_0gt1, norm2_0lt1,       1
 *   GZ_MATH_MALTA_DIFF_PLAIN   a, b                              norm1f, fast_div            1
 *   GZ_MATH_GAMMA_POLY         a                               -                             1
 *   GZ_MATH_OPSIN_PIXEL        a = blurred rgb [3][n],         -                             x, y, b
 *                              b = sharp rgb [3][n]
 *   GZ_MATH_MAXIMUM_CLAMP      a                               maxval                        1
 *   GZ_MATH_REMOVE_RANGE       a                               w                             1
 *   GZ_MATH_AMPLIFY_RANGE      a                               w                             1
 *   GZ_MATH_SUPPRESS_X_BY_Y    a = x, b = y                    -                             1
 *   GZ_MATH_SUPPRESS_BRIGHT    a = hf, b = brightness          mul, reg                      1
 *   GZ_MATH_LF_TO_VALS         a = x, b = y, c = b             -                             3
 *   GZ_MATH_L2DIFF             a = acc, b, c                   w                             1
 *   GZ_MATH_L2DIFF_ASYM        a = acc, b, c                   w_0gt1, w_0lt1 (times 0.8)    1
 *   GZ_MATH_SAME_NOISE_PRE     a, b                            -                             1
 *   GZ_MATH_DIFF_FROM_SUPS     a = sup0, b = sup1              -                             1
 *   GZ_MATH_INTERP_LUT512      a = ix (n DOUBLES)              the table, 512 doubles        1 (double)
 *   GZ_MATH_QUANT_DIV          a, b = q >= 1 (n int32 each)    -                             1 (int32)
 *   GZ_MATH_POW_TO_FLOAT       a = base (n DOUBLES)            expo, scale                   3 (double): the device's
 *                              pow(base, expo); gz_pow_to_float's float(scale * pow) as a double; 1.0 where that float
 *                              is not proven to be libm's (G = 2^-40)  */
enum {
  GZ_MATH_DIV2_SHARED = 0, GZ_MATH_MALTA_DIFF, GZ_MATH_MALTA_DIFF_PLAIN, GZ_MATH_GAMMA_POLY,
  GZ_MATH_OPSIN_PIXEL, GZ_MATH_MAXIMUM_CLAMP, GZ_MATH_REMOVE_RANGE, GZ_MATH_AMPLIFY_RANGE,
  GZ_MATH_SUPPRESS_X_BY_Y, GZ_MATH_SUPPRESS_BRIGHT, GZ_MATH_LF_TO_VALS, GZ_MATH_L2DIFF,
  GZ_MATH_L2DIFF_ASYM, GZ_MATH_SAME_NOISE_PRE, GZ_MATH_DIFF_FROM_SUPS, GZ_MATH_INTERP_LUT512,
  GZ_MATH_QUANT_DIV, GZ_MATH_POW_TO_FLOAT, GZ_MATH_OP_COUNT
};
int gz_probe_math(int device, int op, int n, const void* a, const void* b, const void* c,
                  const double* p, int np, void* out);
/* RGBToYUV420 (preprocess_downsample.cc:452-476) of a packed sRGB image through the kernels and the host path of
 * gz_downsample_silver, without a context: y, u, v receive its three w x h planes (u, v box-upsampled).  guard_log2:
 * the guard of gz_pow_to_float is 2^-guard_log2 -- 40 in production; -1: every cell takes the host path (gather,
 * libm, patch); 64: no guard, nothing takes it (the planes then differ from the reference's wherever the device's pow
 * rounds to another float than libm's).  counters (may be NULL) as gz_downsample_silver's. */
int gz_probe_silver_yuv420(int device, const uint8_t* srgb, int w, int h, int guard_log2, float* y, float* u, float* v,
                           uint64_t counters[2]);
/* The exclusive prefix sums of the entropy coder and of phase B's order (k_scan_offsets, decoupled look-back over tiles
 * of 2048 values) without a context: one launch per entry of `lengths` (1 <= lengths[i] <= n_values, n_lengths <= 4096)
 * on the first lengths[i] of `values`, back to back on ONE scratch sized for the largest, its epochs continuing from
 * start_epoch (< 0x3fffffff) as a context's do -- 0x3ffffffd: the second launch wraps the flags' epoch field, the scratch
 * is cleared and the count starts over at 1.  out receives every launch's off[0 .. lengths[i]] (lengths[i] + 1 sums,
 * 64-bit), one launch after the other. */
int gz_probe_scan_offsets(int device, const uint32_t* values, int n_values, const int32_t* lengths, int n_lengths,
                          uint32_t start_epoch, uint64_t* out);
/* Phase B on state of the caller's choosing (tests/order_domain.py).  None of the three launches a kernel.
 * gz_probe_set_block_max: the nb per-8x8-block maxima of a distance map, as if a gz_compare had left them.
 * gz_probe_set_search: the candidates of a block search as gz_block_zeroing_orders_masked returns them (CSR: offsets of
 * the mask's search grid on the current frame, at most 192 entries per block), put where that call leaves them for the
 * orders, steps and descents that follow; a pending order or descent is void, as after a search.
 * gz_probe_order_state: the device's block weights and max_block_error (search-grid blocks each; either may be NULL);
 * an update of gz_order_advance that is still due is made first, so a test of the update that rides on the next
 * gz_order_build_auto reads AFTER that build. */
int gz_probe_set_block_max(gz_ctx* ctx, const float* block_max);
int gz_probe_set_search(gz_ctx* ctx, int comp_mask, const int32_t* offsets, const uint8_t* idx, const float* err);
int gz_probe_order_state(gz_ctx* ctx, float* weight, float* max_err);
/* div2_shared against the device's own IEEE division, on the device: for the nnum numerators (an
 * even number, at most 12: each pair shares its reciprocal) and every stride-th float denominator
 * of [2^-40, 2^40) -- 80 * 2^23 of them, stride 1: all -- the number of quotients that differ.
 * sample (may be null): the quotients of every sample_every-th CHECKED denominator,
 * sample[(k / sample_every) * nnum + j] for the k-th checked one, for the host to compare with its
 * own division; sample_cap: floats available there. */
int gz_probe_div2_sweep(int device, const float* numerators, int nnum, unsigned stride,
                        unsigned sample_every, uint64_t* mismatches, float* sample,
                        size_t sample_cap);

#ifdef __cplusplus
}
#endif
#endif /* GUETZLI_AMD_H_ */
