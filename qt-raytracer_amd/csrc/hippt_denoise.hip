// hippt_denoise.hip — the edge-avoiding À-trous wavelet denoiser (Dammertz et al. 2010) over the
// accumulation buffer, guided by the camera hit records (include/hippt.h hipptDenoise; the
// arithmetic contract: DESIGN.md §13, restated in numpy by tests/denoise_ref.py).
//
// Three kernels:
//   denoise_prepare  i0 = accumulation / albedo' with the hit's t, and the guide (normal, prim).
//   denoise_pass     one pass of the 5x5 sparse-tap filter at spacing s = 2^k.  The taps of a pixel
//                    stay on its own lattice {x = x0, y = y0 (mod s)}, so a block owns a 16x16 patch
//                    of one lattice, stages the patch's (16 + 4)^2 colour and guide entries in LDS
//                    once and takes all 25 taps from there, whatever s is.
//   denoise_finish   rgba = i * albedo' and the renderer's pixel word of it.
//
// Every sum, product and quotient is one IEEE float32 operation in the order the contract writes
// it: no contraction (the pragma below and -ffp-contract=off), correctly rounded division, and
// subnormal weights kept (the build does not flush them).
#include "hippt_denoise.h"

#include <algorithm>
#include <cmath>

#include "hippt_pixel.h"

#pragma clang fp contract(off)

namespace hippt {
namespace {

constexpr int kTile = 16, kReach = 2, kSide = kTile + 2 * kReach;  // a patch and its apron
// Row stride of the LDS tiles in float4: a multiple of 16, so that a ds_read_b128 lane group (8 lanes
// of one patch row and 8 of the next, MI355X LDS banking) covers 16 different 16-byte slots of the
// 256-byte bank row: no conflict for any tap offset (a stride of kSide = 20 is 2-way on a quarter).
constexpr int kStride = 32;
constexpr int kDenoiseBlock = kTile * kTile;
constexpr int kMaterialMask = (1 << 30) - 1;

// albedo'(p): the Lambertian hit's albedo per channel where it is at least kDenoiseMinAlbedo, else 1.
__device__ __forceinline__ float3 albedo_of(const float4 *hits, const float4 *mats, unsigned p, int demodulate) {
    float3 a{1.0f, 1.0f, 1.0f};
    if (!demodulate) return a;
    const float4 h0 = hits[2 * size_t(p)];
    if (__float_as_int(h0.y) < 0) return a;  // sky
    const int mw = __float_as_int(hits[2 * size_t(p) + 1].w);
    const float4 m = mats[2 * size_t(mw & kMaterialMask)];
    if (__float_as_int(m.w) != kLambertian) return a;
    if (m.x >= kDenoiseMinAlbedo) a.x = m.x;
    if (m.y >= kDenoiseMinAlbedo) a.y = m.y;
    if (m.z >= kDenoiseMinAlbedo) a.z = m.z;
    return a;
}

__global__ __launch_bounds__(256) void denoise_prepare(DenoisePrepareParams P) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= P.pixels) return;
    const float4 c = P.accum[p];
    const float4 h0 = P.hits[2 * size_t(p)], h1 = P.hits[2 * size_t(p) + 1];
    const float3 a = albedo_of(P.hits, P.mats, p, P.demodulate);
    P.colour[p] = float4{c.x / a.x, c.y / a.y, c.z / a.z, h0.x};
    P.guide[p] = float4{h0.z, h0.w, h1.x, h0.y};
}

// POW2: sigma2 is a power of two with a finite normal reciprocal, so dc / sigma2 and dc * (1 / sigma2) are
// the same exactly scaled value rounded once: the same bits, one division per tap fewer.
template <bool POW2>
__global__ __launch_bounds__(kDenoiseBlock) void denoise_pass(DenoisePassParams P) {
    __shared__ float4 sCol[kSide * kStride];
    __shared__ float4 sGd[kSide * kStride];
    const int step = 1 << P.shift;
    // The block's lattice (rx, ry) and patch (tx, ty).  The `share` = min(step, 8) lattices whose pixels
    // lie in one 128-byte line (rx = rxHigh * share + rxLow) read the same lines, so their blocks of one
    // patch go to one XCD's L2, close in time: workgroups go round the 8 XCDs by their number, and of 8 *
    // share consecutive numbers L, L % 8 picks one of 8 groups (a patch, ry, rxHigh) and L / 8 the rxLow.
    const unsigned L = blockIdx.x, span = 8u * unsigned(P.share);
    const unsigned slot = L % span, group = (L / span) * 8u + (slot & 7u);
    if (group >= P.groups) return;  // (the whole block: the groups are padded to a multiple of 8)
    const unsigned hi = unsigned(step) / unsigned(P.share);  // rxHigh values
    unsigned rest = group;
    const int rx = int((rest % hi) * unsigned(P.share) + (slot >> 3));
    rest /= hi;
    const int lx0 = int(rest % unsigned(P.tilesX)) * kTile;
    rest /= unsigned(P.tilesX);
    const int ry = int(rest % unsigned(step));
    const int ly0 = int(rest / unsigned(step)) * kTile;
    if (rx + lx0 * step >= P.width || ry + ly0 * step >= P.height) return;  // (the whole block)
    for (int i = threadIdx.x; i < kSide * kSide; i += kDenoiseBlock) {
        const int j = i / kSide, k = i - j * kSide;
        const int x = rx + (lx0 - kReach + k) * step, y = ry + (ly0 - kReach + j) * step;
        float4 c{0.0f, 0.0f, 0.0f, 0.0f}, g{0.0f, 0.0f, 0.0f, __int_as_float(-1)};  // outside: skipped as sky is
        if (x >= 0 && x < P.width && y >= 0 && y < P.height) {
            const size_t q = size_t(y) * size_t(P.width) + size_t(x);
            c = P.in[q];
            g = P.guide[q];
        }
        sCol[j * kStride + k] = c;
        sGd[j * kStride + k] = g;
    }
    __syncthreads();
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x >> 4;
    const int x = rx + (lx0 + lx) * step, y = ry + (ly0 + ly) * step;
    if (x >= P.width || y >= P.height) return;
    const int at = (ly + kReach) * kStride + lx + kReach;
    const float4 cp = sCol[at], gp = sGd[at];
    float4 res = cp;  // a sky pixel is copied
    if (__float_as_int(gp.w) >= 0) {
        const float zden = P.sigmaDepth * (cp.w * P.depthScale);
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
        constexpr float K[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll
        for (int dy = -kReach; dy <= kReach; ++dy) {
#pragma unroll
            for (int dx = -kReach; dx <= kReach; ++dx) {
                const float4 gq = sGd[at + dy * kStride + dx];
                if (__float_as_int(gq.w) < 0) continue;  // outside the image, or sky
                const float4 cq = sCol[at + dy * kStride + dx];
                const float h = K[dy < 0 ? -dy : dy] * K[dx < 0 ? -dx : dx];
                float wn = fmaxf(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
                for (int k = 0; k < P.normalPower; ++k) wn = wn * wn;
                const float xz = fabsf(cp.w - cq.w) / zden;
                const float wz = 1.0f / (1.0f + xz * xz);
                const float ex = cp.x - cq.x, ey = cp.y - cq.y, ez = cp.z - cq.z;
                const float dc = (ex * ex + ey * ey) + ez * ez;
                const float wc = 1.0f / (1.0f + (POW2 ? dc * P.rcpSigma2 : dc / P.sigma2));
                const float w = ((h * wn) * wz) * wc;
                sx = sx + w * cq.x;
                sy = sy + w * cq.y;
                sz = sz + w * cq.z;
                wsum = wsum + w;
            }
        }
        res = float4{sx / wsum, sy / wsum, sz / wsum, cp.w};
    }
    P.out[size_t(y) * size_t(P.width) + size_t(x)] = res;
}

__global__ __launch_bounds__(256) void denoise_finish(DenoiseFinishParams P) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= P.pixels) return;
    const float4 c = P.colour[p];
    const float3 a = albedo_of(P.hits, P.mats, p, P.demodulate);
    const float r = c.x * a.x, g = c.y * a.y, b = c.z * a.z;
    if (P.rgba) P.rgba[p] = float4{r, g, b, 1.0f};
    if (P.words) P.words[p] = pack_pixel(r, g, b, P.format);
}

}  // namespace

hipError_t launch_denoise_prepare(const DenoisePrepareParams &p, hipStream_t s) {
    if (!p.accum || !p.hits || !p.mats || !p.colour || !p.guide || p.pixels == 0 || p.pixels > (1u << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(denoise_prepare, dim3((p.pixels + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_denoise_pass(const DenoisePassParams &p, hipStream_t s) {
    if (!p.in || !p.guide || !p.out || p.in == p.out || p.width <= 0 || p.height <= 0 || p.shift < 0 ||
        p.shift >= kDenoiseMaxPasses || p.normalPower < 0 || p.normalPower > kDenoiseMaxNormalPower ||
        (long long)p.width * p.height > (1LL << 31) - 1)
        return hipErrorInvalidValue;
    // per lattice (step^2 of them) the patches that cover its ceil(width / step) x ceil(height / step) pixels
    const int step = 1 << p.shift;
    DenoisePassParams q = p;
    q.share = std::min(step, 8);
    q.tilesX = ((p.width + step - 1) / step + kTile - 1) / kTile;
    const long long tilesY = ((p.height + step - 1) / step + kTile - 1) / kTile;
    const long long groups = (long long)q.tilesX * tilesY * step * (step / q.share);
    const long long blocks = (groups + 7) / 8 * 8 * q.share;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    q.groups = unsigned(groups);
    // sigma2 a power of two whose reciprocal is a normal float: multiply (denoise_pass POW2)
    int e = 0;
    q.rcpSigma2 = 1.0f / p.sigma2;
    const bool pow2 = std::frexp(p.sigma2, &e) == 0.5f && std::isnormal(p.sigma2) && std::isnormal(q.rcpSigma2);
    hipLaunchKernelGGL(pow2 ? denoise_pass<true> : denoise_pass<false>, dim3(unsigned(blocks)), dim3(kDenoiseBlock), 0, s, q);
    return hipGetLastError();
}

hipError_t launch_denoise_finish(const DenoiseFinishParams &p, hipStream_t s) {
    if (!p.colour || !p.hits || !p.mats || (!p.rgba && !p.words) || p.pixels == 0 || p.pixels > (1u << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(denoise_finish, dim3((p.pixels + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace hippt
