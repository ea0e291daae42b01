// C-ABI implementation (include/guetzli_amd.h): per-image context, device plane arena,
// blur plans, and the kernel sequences for the block path and for
// ButteraugliComparator::Compare.  Host code only orchestrates; every per-pixel /
// per-block operation is in the gz_kernels_*.h kernels.
//
// Built by hipcc for gfx950 with -ffp-contract=off (guetzli_amd/build.py).  There is no
// CPU path: without a usable HIP device gz_create fails with GZ_E_NO_DEVICE.

#include "../../include/guetzli_amd.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>
#include <string>
#include <sched.h>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "gz_common.h"
#include "gz_kernels_block.h"
#include "gz_kernels_blur.h"
#include "gz_kernels_diff.h"
#include "gz_kernels_search.h"
#include "gz_kernels_entropy.h"
#include "gz_kernels_dctd.h"
#include "gz_kernels_downsample.h"
#include "gz_kernels_silver.h"
#include "gz_kernels_order.h"
#include "gz_kernels_rank.h"
#include "gz_kernels_ingest.h"
#include "gz_kernels_ingestlin.h"
#include "gz_kernels_emit.h"
#include "gz_kernels_emitmap.h"
#include "gz_kernels_emitheat.h"
#include "gz_kernels_emitmask.h"
#include "gz_kernels_scandec.h"
#include "gz_host_weights.h"
#include "order_tables_generated.h"   // host-side csf/bias of order.inc

using namespace gz;

// The implementation by concern (one translation unit: the kernels are templates and static
// functions of the headers above, instantiated where they are launched):
#include "api/plans.h"          // blur plans, Malta normalisations, PsychoImage planes
#include "api/context.h"        // pools, gz_ctx, error macros, plane arena
#include "api/tensor.h"         // the callers' strided device tensors: one view, its checks, an adapter per ABI struct
#include "api/chain.h"          // the Compare chain's stages on three streams
#include "api/entry_context.h"  // gz_create / gz_destroy / ...
#include "api/entry_compare.h"  // block path + gz_compare*
#include "api/entry_phaseb.h"   // gz_order_* / gz_apply_*
#include "api/entry_entropy.h"  // gz_jpeg_*
#include "api/entry_frame.h"    // context-free transforms, 4:2:0 frame
#include "api/entry_decode.h"   // gz_decode_coeffs* / gz_reconstruct_device (device-resident output)
#include "api/entry_scandec.h"  // gz_decode_scan / gz_decode_scan_device (a baseline scan read on the device)
#include "api/entry_heat.h"     // gz_heatmap_device / gz_heatmap_from_map_device / gz_butteraugli_fuzzy_* (the heat map of a distance map)
#include "api/entry_pair.h"     // gz_compare_device_pixels / gz_compare_rgb / gz_distmap_device (image pairs, the map on the device)
#include "api/entry_linear.h"   // gz_create_from_device_linear / gz_set_linear_device / gz_compare_device_linear / gz_butteraugli_linear (linear float images)
#include "api/entry_batch.h"    // gz_butteraugli_batch (n image pairs through one chain: the kernels' batched forms)
#include "api/entry_scandec_batch.h"   // gz_decode_scan_batch_device (n scans through the launches of one device decode)
#include "api/entry_mask.h"     // gz_opsin_device / gz_mask_device / gz_adaptive_quantization (the masking images on the device)
#include "api/entry_search.h"   // gz_block_zeroing_orders*, gz_compare_blocks
#include "api/entry_probes.h"   // gz_probe_* (diagnostics)
