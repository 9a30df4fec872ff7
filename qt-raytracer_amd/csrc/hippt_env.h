// hippt_env.h — the environment map's lookup (include/hippt.h hipptSetEnvironment; DESIGN.md §19;
// tests/env_ref.py is the statement of record).  A pure header: the one text of env(d) for the path
// kernel's miss (hippt_path.hip) and for hipptEnvLookup on the host, so that a CPU test of the host
// function pins the kernel's arithmetic.  It compiles with g++ alone.
//
// The map is a square octahedral image of S x S texels, +y up, the upper hemisphere the inner diamond.
// A direction (dx, dy, dz) of any length is projected by its 1-norm (no square: lengths from 2^-100 to
// 2^80 give the words of a unit direction), the lower hemisphere folded out over the corners, and the
// four texels around the point filtered bilinearly with clamp to edge.  Every line is one IEEE float32
// operation in the association written; fminf/fmaxf are minNum/maxNum (a NaN coordinate gives 0).
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HIPPT_ENV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HIPPT_ENV_HD inline
#endif

namespace hippt {
namespace env {

constexpr int kMaxSize = 4096;

// One texel as the device and the host copy hold it: 16 bytes, so that a tap is one vector load.
struct alignas(16) Texel {
    float r, g, b, pad;
};

HIPPT_ENV_HD float sg(float x) { return x < 0.0f ? -1.0f : 1.0f; }

// The continuous texel coordinate of octahedral coordinate u in [-1, 1], clamped to the centres' range.
HIPPT_ENV_HD float texel_coord(float u, float h, int size) {
    return fminf(fmaxf(fmaf(u, h, h) - 0.5f, 0.0f), float(size - 1));
}

// The octahedral coordinates (u, w) of direction (dx, dy, dz).
HIPPT_ENV_HD void oct_coords(float dx, float dy, float dz, float &u, float &w) {
    const float s = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
    u = dx / s;
    w = dz / s;
    if (dy < 0.0f) {
        const float fu = (1.0f - fabsf(w)) * sg(u);
        const float fw = (1.0f - fabsf(u)) * sg(w);
        u = fu;
        w = fw;
    }
}

// env(d): the filtered texel of direction (dx, dy, dz) in the map E of size x size texels, row y indexing w.
HIPPT_ENV_HD void lookup(const Texel *E, int size, float dx, float dy, float dz, float &e0, float &e1, float &e2) {
    float u, w;
    oct_coords(dx, dy, dz, u, w);
    const float h = 0.5f * float(size);
    const float fx = texel_coord(u, h, size), fy = texel_coord(w, h, size);
    const int x0 = int(fx), y0 = int(fy);
    const int x1 = x0 + 1 < size - 1 ? x0 + 1 : size - 1, y1 = y0 + 1 < size - 1 ? y0 + 1 : size - 1;
    const float a = fx - float(x0), b = fy - float(y0);
    const Texel t00 = E[size_t(y0) * size_t(size) + size_t(x0)], t01 = E[size_t(y0) * size_t(size) + size_t(x1)];
    const Texel t10 = E[size_t(y1) * size_t(size) + size_t(x0)], t11 = E[size_t(y1) * size_t(size) + size_t(x1)];
    const float top0 = fmaf(a, t01.r - t00.r, t00.r), bot0 = fmaf(a, t11.r - t10.r, t10.r);
    const float top1 = fmaf(a, t01.g - t00.g, t00.g), bot1 = fmaf(a, t11.g - t10.g, t10.g);
    const float top2 = fmaf(a, t01.b - t00.b, t00.b), bot2 = fmaf(a, t11.b - t10.b, t10.b);
    e0 = fmaf(b, bot0 - top0, top0);
    e1 = fmaf(b, bot1 - top1, top1);
    e2 = fmaf(b, bot2 - top2, top2);
}

}  // namespace env
}  // namespace hippt
