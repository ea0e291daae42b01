// Params::use_silver_screen: RGBToYUV420 of the reference (guetzli/preprocess_downsample.cc:
// 283-476) -- the YUV 4:2:0 samples whose decoded image has the luma of the original when
// averaged in LINEAR light, found by 20 fixed-point iterations through the decoder model.
// The whole conversion on the host, with the same libm as the reference uses (glibc's pow), row-parallel on the
// worker pool.  The encoder runs the conversion on the device (gz_downsample_silver, csrc/gz_kernels_silver.h), which
// gives the same floats; this form is the yardstick of the tests (gzh_silver_screen_yuv420) and what a caller of
// gz_downsample_planes may feed it.  The per-sample functions are shared with the device path: csrc/gz_silver_ref.h.
#pragma once
#include <stdint.h>

#include <vector>

namespace guetzli_amd {

// rgb: packed 8-bit sRGB (w*h*3) = OutputImage::ToSRGB() of the unquantised image.
// y, u, v: w*h floats each (u and v already box-upsampled to full resolution, as
// RGBToYUV420 returns them).
void SilverScreenYUV420(const uint8_t* rgb, int w, int h, std::vector<float>* y,
                        std::vector<float>* u, std::vector<float>* v);

}  // namespace guetzli_amd
