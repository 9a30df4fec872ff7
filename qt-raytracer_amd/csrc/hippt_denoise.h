// hippt_denoise.h — launch interface of the edge-avoiding À-trous denoiser (hippt_denoise.hip;
// include/hippt.h hipptDenoise).  Every pointer is device memory of the launch's
// device; every array holds width * height entries, row 0 = v = 0.
#pragma once

#include "hippt_device.h"

namespace hippt {

// Albedo channels below this are not demodulated (2^-6: the quotient would amplify the noise of a
// near-black surface).
constexpr float kDenoiseMinAlbedo = 0.015625f;
constexpr int kDenoiseMaxPasses = 8, kDenoiseMaxNormalPower = 10;
// timed stages (HIPPT_INFO_DENOISE_NS): the guide query, prepare, the passes, finish
constexpr int kDenoiseStages = 3 + kDenoiseMaxPasses;

// i0 = accumulation / albedo' and the guides, from the accumulation, the camera hit records
// (hipptHit as two float4) and the materials (MeshParams::mats).
struct DenoisePrepareParams {
    const float4 *accum;
    const float4 *hits;
    const float4 *mats;
    float4 *colour;  // (i0.rgb, t)
    float4 *guide;   // (normal, prim as int bits; prim < 0: sky)
    unsigned pixels;
    int demodulate;
};

// Pass k (tap spacing step = 1 << shift) from `in` to `out`.
struct DenoisePassParams {
    const float4 *in;
    const float4 *guide;
    float4 *out;
    int width, height;
    int shift;
    int normalPower;
    float sigma2;      // (sigmaColor * (1.0f / float(step)))^2
    float depthScale;  // float(step); zden(p) = sigmaDepth * (t_p * depthScale)
    float sigmaDepth;
    // set by launch_denoise_pass: 1 / sigma2, the lattices per 128-byte line (min(step, 8)), the patches
    // per lattice row and the block groups (patches x ry x rx / share)
    float rcpSigma2;
    int share, tilesX;
    unsigned groups;
};

// rgba = (i * albedo', 1) and its pixel word; either output may be null.
struct DenoiseFinishParams {
    const float4 *colour;
    const float4 *hits;
    const float4 *mats;
    float4 *rgba;
    uint32_t *words;
    unsigned pixels;
    int demodulate;
    int format;  // kPixelArgb / kPixelRgba8
};

hipError_t launch_denoise_prepare(const DenoisePrepareParams &p, hipStream_t s);
hipError_t launch_denoise_pass(const DenoisePassParams &p, hipStream_t s);
hipError_t launch_denoise_finish(const DenoiseFinishParams &p, hipStream_t s);

}  // namespace hippt
