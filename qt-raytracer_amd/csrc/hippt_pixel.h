// hippt_pixel.h — the displayed pixel word of a linear colour, shared by the render kernels
// (hippt_kernels.hip) and the denoiser (hippt_denoise.hip).
#pragma once

#include "hippt_device.h"

namespace hippt {

__device__ __forceinline__ unsigned q8(float c) {
    return unsigned(sqrtf(fminf(fmaxf(c, 0.0f), 1.0f)) * 255.0f);
}

// The displayed pixel of an accumulated colour.  kPixelArgb: the CUDA backend's word
// (CudaPathTracerKernel.cu:171-178): 0xAARRGGBB, channel = uint(sqrt(clamp(c, 0, 1)) * 255)
// truncated.  kPixelRgba8: the GL / Vulkan backends' RGBA8 UNORM image texel
// (GpuPathTracer.cpp:284-285, pathtrace_vulkan.comp:113-114): bytes R, G, B, A in memory
// (0xAABBGGRR), channel = sqrt(clamp(c, 0, 1)) * 255 rounded to nearest, ties to even.
__device__ __forceinline__ uint32_t pack_pixel(float r, float g, float b, int format) {
    if (format == kPixelRgba8) {
        const auto u8 = [](float c) { return unsigned(rintf(sqrtf(fminf(fmaxf(c, 0.0f), 1.0f)) * 255.0f)); };
        return (255u << 24) | (u8(b) << 16) | (u8(g) << 8) | u8(r);
    }
    return (255u << 24) | (q8(r) << 16) | (q8(g) << 8) | q8(b);
}

}  // namespace hippt
