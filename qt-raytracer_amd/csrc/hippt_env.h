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
#include <cstddef>

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

// ---- sampling the map (HIPPT_OPT_ENV_SAMPLING; tests/envs_ref.py is the statement of record) ----
// The one text of the table's per-texel arithmetic (hippt_refit.hip builds the table with it), of the draw and
// its density (hippt_path.hip env_connect) and of the weight of a miss after a Lambertian scatter
// (env_miss_weight), so that tests/native/env_sample_check.cpp pins them with g++ before a GPU runs.

// One texel of the selection table: c(x, y), the inclusive sum of q along the row, and k(x, y), the density of
// the draw per unit of (u, w) area.  q(x, y) = c(x, y) - c(x - 1, y).
struct alignas(8) TexelSel {
    unsigned c;
    float k;
};

constexpr int kSelTexelOne = 4096;  // q of a row's heaviest texel
constexpr int kSelRowOne = 65536;   // m of the heaviest row

HIPPT_ENV_HD float fdot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(ax, bx, fmaf(ay, by, az * bz));
}

HIPPT_ENV_HD unsigned hash32(unsigned x) {  // hippt_trace.h's
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

HIPPT_ENV_HD float rand01(unsigned &s) {
    s = hash32(s);
    return float(s) * 0x1p-32f;
}

// The point of the octahedron |x| + |y| + |z| = 1 above (u, w) in [-1, 1]^2, the lower hemisphere folded out.
HIPPT_ENV_HD void oct_point(float u, float w, float &dx, float &dy, float &dz) {
    dy = (1.0f - fabsf(u)) - fabsf(w);
    if (dy >= 0.0f) {
        dx = u;
        dz = w;
    } else {
        dx = (1.0f - fabsf(w)) * sg(u);
        dz = (1.0f - fabsf(u)) * sg(w);
    }
}

// W(x, y): the texel's luminance sum times the solid angle per unit of (u, w) area at its centre, 1 / |p|^3; a
// NaN, negative or infinite texel weighs 0.
HIPPT_ENV_HD float texel_weight(const Texel &e, int x, int y, int size) {
    const float uc = float(2 * x + 1) / float(size) - 1.0f, wc = float(2 * y + 1) / float(size) - 1.0f;
    float dx, dy, dz;
    oct_point(uc, wc, dx, dy, dz);
    const float n2 = fdot3(dx, dy, dz, dx, dy, dz);
    const float J = 1.0f / (n2 * sqrtf(n2));
    const float lum = (e.r + e.g) + e.b;
    const float W = lum * J;
    return W > 0.0f && W < INFINITY ? W : 0.0f;
}

// q of a texel of weight W in a row whose largest weight is Wmax, and m of a row of value V among rows whose
// largest value is Vmax (flat: Vmax is not in (0, +inf)).
HIPPT_ENV_HD unsigned texel_q(float W, float Wmax) {
    if (!(Wmax > 0.0f)) return 1u;
    const int v = int((W / Wmax) * float(kSelTexelOne));
    return unsigned(v < 1 ? 1 : v > kSelTexelOne ? kSelTexelOne : v);
}
HIPPT_ENV_HD float row_value(unsigned R, float Wmax) { return (float(R) * 0.000244140625f) * Wmax; }
HIPPT_ENV_HD unsigned row_m(float V, float Vmax) {
    if (!(Vmax > 0.0f && Vmax < INFINITY)) return 1u;
    const int v = int((V / Vmax) * float(kSelRowOne));
    return unsigned(v < 1 ? 1 : v > kSelRowOne ? kSelRowOne : v);
}
HIPPT_ENV_HD float texel_k(unsigned m, unsigned T, unsigned q, unsigned R, int size) {
    return ((float(m) / float(T)) * (float(q) / float(R))) * (0.25f * (float(size) * float(size)));
}

// The smallest index i of c[0 .. n) (stride `stride` words) with c[i] > x; c[n - 1] > x.
HIPPT_ENV_HD int upper_bound(const unsigned *c, int stride, int n, unsigned x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[size_t(mid) * size_t(stride)] > x)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One draw from the table (rowC: C_y; tex: the texels' records): the texel (x, y), the unit direction om and
// n2 * sqrtf(n2) of the unnormalised one (|p|^3), and the texel's k.  Four RNG draws.
struct Draw {
    int x, y;
    float ox, oy, oz, n3, k;
};
HIPPT_ENV_HD Draw draw(const unsigned *rowC, const TexelSel *tex, int size, unsigned &rng) {
    Draw d;
    rng = hash32(rng);
    const unsigned xr = unsigned(((unsigned long long)rng * rowC[size - 1]) >> 32);
    d.y = upper_bound(rowC, 1, size, xr);
    const TexelSel *row = tex + size_t(d.y) * size_t(size);
    rng = hash32(rng);
    const unsigned xc = unsigned(((unsigned long long)rng * row[size - 1].c) >> 32);
    d.x = upper_bound(&row[0].c, 2, size, xc);
    const float a = rand01(rng), b = rand01(rng), g2 = 2.0f / float(size);
    const float u = fmaf(float(d.x) + a, g2, -1.0f), w = fmaf(float(d.y) + b, g2, -1.0f);
    float dx, dy, dz;
    oct_point(u, w, dx, dy, dz);
    const float n2 = fdot3(dx, dy, dz, dx, dy, dz);
    const float inv = 1.0f / sqrtf(n2);
    d.ox = dx * inv, d.oy = dy * inv, d.oz = dz * inv;
    d.n3 = n2 * sqrtf(n2);
    d.k = row[d.x].k;
    return d;
}

// The connection's factor for a draw with cosine cosS to the faced normal, `sel` the coin's probability of the
// map: g = p_scatter / p_table, under MIS g / (1 + g^2).  False: no shadow ray.
HIPPT_ENV_HD bool connect_factor(const Draw &d, float cosS, float sel, bool mis, float &g) {
    const float pl = (d.k * d.n3) * sel;
    if (!(cosS > 0.0f) || !(pl > 0.0f)) return false;
    g = cosS / (3.14159274f * pl);
    if (mis) {
        if (!(g < INFINITY)) return false;
        g = g / fmaf(g, g, 1.0f);
    }
    return true;
}

// MIS: the weight of env(d) met by a segment of direction d that a Lambertian scatter of cosine cb started:
// the scatter's density against the table's at d, squared; 1 where the table could not have drawn d.
HIPPT_ENV_HD float miss_weight(const TexelSel *tex, int size, float dx, float dy, float dz, float cb, float sel) {
    const float s1 = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
    const float r = sqrtf(fdot3(dx, dy, dz, dx, dy, dz)) / s1;
    const float r3 = (r * r) * r;
    float u, w;
    oct_coords(dx, dy, dz, u, w);
    const float h = 0.5f * float(size);
    const int x = int(fminf(fmaxf(fmaf(u, h, h), 0.0f), float(size - 1)));
    const int y = int(fminf(fmaxf(fmaf(w, h, h), 0.0f), float(size - 1)));
    const float pl = (tex[size_t(y) * size_t(size) + size_t(x)].k * r3) * sel;
    float wb = 1.0f;
    if (cb > 0.0f && pl > 0.0f) {
        const float gh = cb / (3.14159274f * pl);
        const float s = gh * gh;
        if (s < INFINITY) wb = s / fmaf(gh, gh, 1.0f);
    }
    return wb;
}

}  // namespace env
}  // namespace hippt
