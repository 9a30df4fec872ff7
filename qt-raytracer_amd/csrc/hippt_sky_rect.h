// hippt_sky_rect.h — the screen rectangle outside which a pinhole camera's rays cannot reach the
// scene (HIPPT_OPT_SKY_RECT, DESIGN.md §5 "Sky rectangle").  A pure host function of the camera as
// the kernels receive it, the image size and the host tree's root box; compiles with g++ alone
// (tests/native/sky_rect_check.cpp drives it against the oracle, tests/test_sky_rect.py).
//
// The camera sample (hippt_trace.h camera_sample) of pixel (x, y) aims at
// llc + s * horizontal + t * vertical with s = (x + rand01) * invW, t = (y + rand01) * invH and
// rand01 in [0, 1]: in pixel units the sample lies in [x, x + 1] x [y, y + 1].  The root box, moved
// out by one more builder pad, is projected through the same four camera vectors in double; its
// bounding rectangle in pixel units, widened by one whole pixel plus 2^-20 of the image size, bounds
// every sample whose ray can meet the builder-padded box, provided the kernel's float direction stays
// within a fraction of a pixel of the ideal one.  That is a condition on the camera, checked here:
// the direction fl(fl(fmaf(t, V, fl(fmaf(s, H, llc)))) - origin) carries an absolute error of up to
// e_k = 2^-24 * (2 * (|llc_k| + sMax*|H_k| + tMax*|V_k|) + |a_k| + sMax*|H_k| + tMax*|V_k|) per
// component: half an ulp of each fused multiply-add's result, both no larger than the first sum, and
// half an ulp of the difference, no larger than the second (a = llc - origin; s and t up to
// sMax = 1 + 2/(W - 1), tMax likewise; taken 1/1000 larger for the bounds' own rounding).  It is about
// an ulp of the origin's coordinates and does not shrink with the direction's length (the focus
// distance).  Written in the basis (a, H, V), a = llc - origin, an error
// alpha*a + beta*H + gamma*V turns the ideal ray of (s, t) into the ideal ray of
// ((s + beta) / (1 + alpha), (t + gamma) / (1 + alpha)): the sample moves on the image plane, by at
// most (|beta| + sMax*|alpha|) / (1 - |alpha|) in s.  With the rows of the basis' inverse this is
// bounded for every error within the e_k (direction_error_pixels).  Above kMaxDirectionErrorPixels
// of a pixel on either axis (a far camera with a short focus distance: a pixel's pitch on the image
// plane comes near an ulp of the origin) there is no rectangle.  Below it the one-pixel margin
// covers the error with 3/4 of a pixel to spare, and the extra pad covers what is left of the
// argument (the box planes' own roundings).  A pixel whose footprint lies outside the rectangle is
// then sky-certain.
#pragma once

#include <cmath>

namespace hippt {
namespace skyrect {

// Pixels [x0, x1) x [y0, y1) may see the scene; every other pixel of the image is sky-certain.
// x0 >= x1 or y0 >= y1: no pixel sees it.  whole(): nothing is skipped.
struct Rect {
    int x0, y0, x1, y1;
};
inline Rect whole(int width, int height) { return Rect{0, 0, width, height}; }
inline bool is_whole(const Rect &r, int width, int height) {
    return r.x0 <= 0 && r.y0 <= 0 && r.x1 >= width && r.y1 >= height;
}
// image pixels outside the rectangle
inline long long pixels_outside(const Rect &r, int width, int height) {
    const long long w = r.x1 > r.x0 ? r.x1 - r.x0 : 0, h = r.y1 > r.y0 ? r.y1 - r.y0 : 0;
    return (long long)width * height - w * h;
}

// The largest move of a sample on the image plane, in pixels per axis, that the rounding of the
// kernel's direction arithmetic can cause (see above).  inv: the inverse of the basis [a H V] by rows
// (alpha, beta, gamma); e: the per-component error bounds.  Infinite when alpha is not small.
constexpr double kMaxDirectionErrorPixels = 0.25;
inline void direction_error_pixels(const double inv[3][3], const double e[3], double sMax, double tMax, double invW,
                                   double invH, double &px, double &py) {
    double m[3];
    for (int r = 0; r < 3; ++r) m[r] = std::fabs(inv[r][0]) * e[0] + std::fabs(inv[r][1]) * e[1] + std::fabs(inv[r][2]) * e[2];
    if (!(m[0] < 0.5)) {
        px = py = INFINITY;
        return;
    }
    px = (m[1] + sMax * m[0]) / (1.0 - m[0]) / invW;
    py = (m[2] + tMax * m[0]) / (1.0 - m[0]) / invH;
}

// Cam: CameraF (hippt_device.h) or any struct with its origin, llc, horizontal, vertical, u, v and
// lens_radius.  lo / hi: the root box as the builder padded it; pad: Bvh::pad.  Returns whole() when
// the bound does not apply: a lens, no primitives, a corner not strictly in front of the camera (the
// camera inside or beside the box), a degenerate camera, a camera whose direction arithmetic is not
// exact to a quarter of a pixel (direction_error_pixels), or anything non-finite.
template <typename Cam>
inline Rect sky_rect(const Cam &cam, int width, int height, const float lo[3], const float hi[3], float pad,
                     int numPrims) {
    const Rect all = whole(width, height);
    if (width <= 0 || height <= 0 || numPrims <= 0) return all;
    if (!(cam.lens_radius == 0.0f)) return all;  // (NaN too)
    if (!(pad >= 0.0f) || !std::isfinite(pad)) return all;
    double o[3], a[3], h[3], v[3], blo[3], bhi[3];
    for (int k = 0; k < 3; ++k) {
        o[k] = cam.origin[k];
        a[k] = double(cam.llc[k]) - o[k];
        h[k] = cam.horizontal[k];
        v[k] = cam.vertical[k];
        blo[k] = double(lo[k]) - double(pad);
        bhi[k] = double(hi[k]) + double(pad);
        // (u, v: the kernel's fast path takes the lens offset lens_radius * (u, v) as zero)
        if (!std::isfinite(o[k]) || !std::isfinite(a[k]) || !std::isfinite(h[k]) || !std::isfinite(v[k]) ||
            !std::isfinite(blo[k]) || !std::isfinite(bhi[k]) || !(blo[k] <= bhi[k]) || !std::isfinite(cam.u[k]) ||
            !std::isfinite(cam.v[k]))
            return all;
    }
    auto det3 = [](const double *p, const double *q, const double *r) {
        return p[0] * (q[1] * r[2] - q[2] * r[1]) - p[1] * (q[0] * r[2] - q[2] * r[0]) +
               p[2] * (q[0] * r[1] - q[1] * r[0]);
    };
    // corner - origin = l * (a + s*h + t*v): (l, l*s, l*t) by Cramer's rule
    const double det = det3(a, h, v);
    if (!std::isfinite(det) || det == 0.0) return all;
    // the kernel's own pixel scale: s = (x + rand01) * invW, invW = 1 / max(1, W - 1) as a float
    const double invW = double(1.0f / float(width > 1 ? width - 1 : 1));
    const double invH = double(1.0f / float(height > 1 ? height - 1 : 1));
    {
        // the inverse of [a H V] by cofactors: row r of the inverse is (cross of the other two columns) / det
        const double *col[3] = {a, h, v};
        double inv[3][3], e[3];
        for (int r = 0; r < 3; ++r) {
            const double *p = col[(r + 1) % 3], *q = col[(r + 2) % 3];
            inv[r][0] = (p[1] * q[2] - p[2] * q[1]) / det;
            inv[r][1] = (p[2] * q[0] - p[0] * q[2]) / det;
            inv[r][2] = (p[0] * q[1] - p[1] * q[0]) / det;
        }
        const double sLim = 1.0 + 2.0 * invW, tLim = 1.0 + 2.0 * invH;
        for (int k = 0; k < 3; ++k) {
            const double hv = sLim * std::fabs(h[k]) + tLim * std::fabs(v[k]);
            e[k] = (2.0 * (std::fabs(double(cam.llc[k])) + hv) + std::fabs(a[k]) + hv) * (1.001 / 16777216.0);
        }
        double epx, epy;
        direction_error_pixels(inv, e, sLim, tLim, invW, invH, epx, epy);
        if (!(epx <= kMaxDirectionErrorPixels) || !(epy <= kMaxDirectionErrorPixels)) return all;
    }
    double sMin = INFINITY, sMax = -INFINITY, tMin = INFINITY, tMax = -INFINITY;
    for (int c = 0; c < 8; ++c) {
        double q[3];
        for (int k = 0; k < 3; ++k) q[k] = (((c >> k) & 1) ? bhi[k] : blo[k]) - o[k];
        const double l = det3(q, h, v) / det, ls = det3(a, q, v) / det, lt = det3(a, h, q) / det;
        if (!std::isfinite(l) || !(l > 0.0)) return all;  // not strictly in front of the camera
        const double px = ls / l / invW, py = lt / l / invH;
        if (!std::isfinite(px) || !std::isfinite(py)) return all;
        sMin = std::fmin(sMin, px);
        sMax = std::fmax(sMax, px);
        tMin = std::fmin(tMin, py);
        tMax = std::fmax(tMax, py);
    }
    // one whole pixel on every side plus 2^-20 of the image size; pixel x's footprint [x, x + 1]
    // meets [A, B] when x >= A - 1 and x <= B
    const double ex = 1.0 + double(width) * (1.0 / 1048576.0), ey = 1.0 + double(height) * (1.0 / 1048576.0);
    auto clampi = [](double d, int hiLim) { return d <= 0.0 ? 0 : d >= double(hiLim) ? hiLim : int(d); };
    Rect r;
    r.x0 = clampi(std::ceil(sMin - ex - 1.0), width);
    r.y0 = clampi(std::ceil(tMin - ey - 1.0), height);
    r.x1 = clampi(std::floor(sMax + ex) + 1.0, width);
    r.y1 = clampi(std::floor(tMax + ey) + 1.0, height);
    if (r.x1 <= r.x0 || r.y1 <= r.y0) return Rect{0, 0, 0, 0};  // the scene is off-screen: every pixel outside
    return r;
}

// ---- runs wholly outside the rectangle (HIPPT_OPT_SKY_COMBINE, DESIGN.md §5 "Sky runs in the combine") ----
// Host and device both compile what follows.
#if defined(__HIPCC__)
#define HIPPT_SKY_HD __host__ __device__ __forceinline__
#else
#define HIPPT_SKY_HD inline
#endif

// The band's run geometry (item_order.h RunLayout and the band's rows): band row k is image row
// y0 + k * rowStride; tileShift < 6: tiles of 2^tileShift columns x 2^(6 - tileShift) band rows over the
// band's whole strips, runs of 64 consecutive band pixels over the rest; 6: consecutive runs only.
struct RunShape {
    unsigned width, rows, tileShift;
    int y0, rowStride;
};
HIPPT_SKY_HD unsigned shape_band_pixels(const RunShape S) { return S.width * S.rows; }
// band pixels the tiles cover (the whole strips), 0 without tiles
HIPPT_SKY_HD unsigned shape_tile_pixels(const RunShape S) {
    if (S.tileShift >= 6u) return 0u;
    const unsigned th = 64u >> S.tileShift;
    return (S.rows / th) * th * S.width;
}
template <typename R>
HIPPT_SKY_HD bool pixel_outside(const R &r, unsigned x, unsigned y) {
    return x - unsigned(r.x0) >= unsigned(r.x1 - r.x0) || y - unsigned(r.y0) >= unsigned(r.y1 - r.y0);
}
// (a rectangle that skips nothing: the mode has nothing to do)
template <typename R>
HIPPT_SKY_HD bool rect_valid(const R &r) {
    return r.x0 >= 0 && r.y0 >= 0 && r.x1 >= r.x0 && r.y1 >= r.y0;
}

// "This 64-item run is wholly sky-certain": the run whose item 0 is band pixel `base` (a tile when
// `tile`) has 64 valid pixels, all outside the rectangle.  It is the refill path's test,
// __ballot(skyLane) == ~0ull (hippt_kernels.hip), as a function of the run: lane k has
// skyLane = (item k valid) && pixel_outside(rect, x_k, y_k), with (x_k, y_k) from the same base + offset
// arithmetic as run_pixel, and a ballot of all ones is the conjunction over the 64 lanes.  Where a refill's
// 64 positions are one table slot (a band of a multiple of 64 pixels: every frame's row starts aligned)
// the two tests are the same test.  Where they are not (a row length that is no multiple of 64: later
// frames start unaligned and a claim straddles two slots) the ballot may differ, and nothing depends on
// it: the host alone decides which runs the table leaves out, with this function, the combine asks the
// same function through pixel_in_sky_run, and for a sample of a pixel outside the rectangle the refill
// path and the combine compute the same bits, whichever of them finishes it.  A tile is a product of a
// column range and a row set, so it is outside iff its columns miss [x0, x1) or every one of its rows
// misses [y0, y1); a consecutive run is a row range with a column interval per row.
template <typename R>
HIPPT_SKY_HD bool run_sky_certain(const RunShape S, const R &rect, unsigned base, bool tile) {
    if (!rect_valid(rect) || S.width == 0u) return false;
    if (tile) {
        const unsigned tw = 1u << S.tileShift, th = 64u >> S.tileShift;
        const unsigned yb = base / S.width, x = base - yb * S.width;
        if (x + tw > S.width || yb + th > S.rows) return false;
        // columns [x, x + tw) against [x0, x1)
        if (int(x + tw) <= rect.x0 || int(x) >= rect.x1) return true;
        for (unsigned k = 0; k < th; ++k) {
            const unsigned y = unsigned(S.y0) + (yb + k) * unsigned(S.rowStride);
            if (y - unsigned(rect.y0) < unsigned(rect.y1 - rect.y0)) return false;
        }
        return true;
    }
    if (base + 64u > shape_band_pixels(S)) return false;
    unsigned p = base;
    while (p < base + 64u) {
        const unsigned yb = p / S.width, x = p - yb * S.width;
        const unsigned n = (S.width - x) < (base + 64u - p) ? S.width - x : base + 64u - p;  // this row's pixels
        const unsigned y = unsigned(S.y0) + yb * unsigned(S.rowStride);
        const bool rowIn = y - unsigned(rect.y0) < unsigned(rect.y1 - rect.y0);
        if (rowIn && !(int(x + n) <= rect.x0 || int(x) >= rect.x1)) return false;
        p += n;
    }
    return true;
}

// The inverse the combine needs: band pixel p's run (item_order.h run_base) -> base and shape; false
// for a pixel in no whole run (the band's last bandPixels % 64 pixels).
HIPPT_SKY_HD bool pixel_run(const RunShape S, unsigned p, unsigned &base, bool &tile) {
    const unsigned tp = shape_tile_pixels(S), bp = shape_band_pixels(S);
    if (p >= bp) return false;
    if (p < tp) {
        const unsigned tw = 1u << S.tileShift, th = 64u >> S.tileShift;
        const unsigned yb = p / S.width, x = p - yb * S.width;
        base = (yb / th) * th * S.width + (x & ~(tw - 1u));
        tile = true;
        return true;
    }
    base = tp + ((p - tp) & ~63u);
    tile = false;
    return base + 64u <= bp;
}
template <typename R>
HIPPT_SKY_HD bool pixel_in_sky_run(const RunShape S, const R &rect, unsigned p) {
    unsigned base = 0;
    bool tile = false;
    return pixel_run(S, p, base, tile) && run_sky_certain(S, rect, base, tile);
}

// A queue position of a batch whose table has `runCount` runs per frame out of the band's
// bandPixels / 64 (the omitted ones are finished by the combine): frame fl = pos / rowLen and offset
// q = pos % rowLen with rowLen = 64 * runCount + bandPixels % 64.  q < 64 * runCount is item q % 64 of
// table entry fl * runCount + q / 64; the rest are the band's last pixels in image order,
// fl * bandPixels + (bandPixels - rowLen) + q.  With every run in the table rowLen is bandPixels.
HIPPT_SKY_HD unsigned order_row_len(unsigned bandPixels, unsigned runCount) { return 64u * runCount + (bandPixels & 63u); }
HIPPT_SKY_HD unsigned order_tail_item(unsigned bandPixels, unsigned rowLen, unsigned fl, unsigned q) {
    return fl * bandPixels + (bandPixels - rowLen) + q;
}
// n / d and n % d from d's float reciprocal, corrected by one (trace::divmod's arithmetic)
HIPPT_SKY_HD void divmod_rcp(unsigned n, unsigned d, float rcp, unsigned &q, unsigned &r) {
    q = unsigned(float(n) * rcp);
    int rem = int(n - q * d);
    if (rem < 0) {
        --q;
        rem += int(d);
    } else if (rem >= int(d)) {
        ++q;
        rem -= int(d);
    }
    r = unsigned(rem);
}
// The item at queue position pos of such a table (trace::order_item calls this; the model test decodes
// every position of its tables with it): a table entry's item k is its band pixel + k, or for a tile
// (bit 31) column k mod 2^tileShift, band row k >> tileShift of the tile.
HIPPT_SKY_HD unsigned order_position_item(unsigned pos, unsigned bandPixels, unsigned rowLen, float rcpRowLen,
                                          unsigned runCount, const unsigned *table, unsigned width, unsigned tileShift) {
    unsigned fl, q;
    divmod_rcp(pos, rowLen, rcpRowLen, fl, q);
    const unsigned run = q >> 6, k = q & 63u;
    if (run >= runCount) return order_tail_item(bandPixels, rowLen, fl, q);
    const unsigned v = table[fl * runCount + run];
    return (v & 0x7fffffffu) + ((v >> 31) ? (k & ((1u << tileShift) - 1u)) + (k >> tileShift) * width : k);
}

}  // namespace skyrect
}  // namespace hippt
