// hippt_slab.h — the arithmetic of the BVH box (slab) test and of the render megakernel's node-box
// trim as pure functions.  The gfx950 kernels call them (hippt_trace.h prepare, child_key,
// child_key_p; hippt_kernels.hip's LDS scene copy); tests/native/pad_model.cpp compiles this header
// with g++ and measures, over the oracle's rays, how much padding the test needs to stay
// conservative (tests/test_render_pad.py).
//
// The test is not result-defining (hippt_trace.h): a box only has to be hit by every ray whose
// closest accepted hit lies under it.  What it computes, per axis with near/far planes chosen by
// the direction's sign:
//   inv = rcp(clamp_dir(d))                the caller's reciprocal: v_rcp_f32 on the device (within
//                                          1 ulp), the correctly rounded one moved by -1, 0, +1 ulp
//                                          in the host model
//   oi  = o * inv                          one rounding
//   t   = fma(plane, inv, -oi)             one rounding
//   n   = max(t_near.x, t_near.y, t_near.z, tmin),  f = min(t_far.x, t_far.y, t_far.z, bestT)
//   hit = n <= f
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HIPPT_SL __host__ __device__ __forceinline__
#else
#define HIPPT_SL inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hippt {
namespace slab {

// A direction component kept away from zero (its sign kept): the reciprocal stays finite.
HIPPT_SL float clamp_dir(float d) { return copysignf(fmaxf(fabsf(d), 1e-20f), d); }

// The origin's term of an axis, o * inv (subtracted inside each plane's FMA).
HIPPT_SL float origin_term(float o, float inv) { return o * inv; }

// Ray parameter at which the ray crosses `plane` on an axis.
HIPPT_SL float plane_t(float plane, float inv, float oi) { return fmaf(plane, inv, -oi); }

// min(a, b) as one v_min_f32 on the device: fminf() of the loop-carried bestT makes the compiler
// quieten a possible signaling NaN first (a v_max_f32 b, b per node visit); the box test has no NaN
// (finite padded boxes, clamped reciprocals), and v_min_f32 of non-NaN inputs is fminf.
HIPPT_SL float fmin_raw(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float d;
    asm("v_min_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
#else
    return fminf(a, b);
#endif
}

// Entry and exit distances of a box from its near and far planes' ray parameters.
HIPPT_SL float entry_t(float ax, float ay, float az, float tmin) { return fmaxf(fmaxf(ax, ay), fmaxf(az, tmin)); }
HIPPT_SL float exit_t(float bx, float by, float bz, float bestT) { return fminf(fminf(bx, by), fmin_raw(bz, bestT)); }

// The decision: the ray's interval [tmin, bestT] meets the box.  A macro and not a function: the
// kernels' generated code must not move with this header, and both a bool-returning helper and a
// helper holding the key's select changed the instruction schedules of some mesh kernels.
#define HIPPT_SLAB_MEETS(n, f) ((n) <= (f))

// The whole test of one box for a prepared ray (inv*, oi*), as the kernels' child_key puts the
// pieces above together; n = the entry distance (the child sort key's float).
HIPPT_SL bool box_hit(float nx, float fx, float ny, float fy, float nz, float fz, float ix, float iy, float iz,
                      float oix, float oiy, float oiz, float tmin, float bestT, float &n) {
    const float ax = plane_t(nx, ix, oix), bx = plane_t(fx, ix, oix);
    const float ay = plane_t(ny, iy, oiy), by = plane_t(fy, iy, oiy);
    const float az = plane_t(nz, iz, oiz), bz = plane_t(fz, iz, oiz);
    n = entry_t(ax, ay, az, tmin);
    const float f = exit_t(bx, by, bz, bestT);
    return HIPPT_SLAB_MEETS(n, f);
}

// ---- node-box trim of the render megakernel's LDS scene copy --------------------------------------
// The builder and the refit pad every box by pad = M * 2^-16 (M: the largest |coordinate| of the
// scene and the camera, at least 1e-3; bvh_builder.cpp).  The render megakernel's rays start on a
// primitive or at the camera; while the camera's origin lies within M and no triangle is a thin
// sliver (the host checks both per batch, hippt_api.cpp render_pad_holds, and passes a trim scale
// of 0 otherwise) the test above needs far less: its
// LDS copy of an LDS-resident 4-wide float tree moves every plane back inward by
// trim = pad - renderPad, renderPad = M * 2^-exponent, so that a scattered ray's own flat leaf is
// culled at its parent's visit more often.  The trees in global memory, which the ray queries
// traverse with arbitrary origins, keep the builder's pad.
constexpr int kPadExponent = 16;  // the builder's pad: M * 2^-16
// HIPPT_OPT_RENDER_PAD: exponents the option takes (0: no trim), and the default (DESIGN.md §5:
// 4 x the measured requirement, a power of two, never below M * 2^-21)
constexpr int kRenderPadMin = 17, kRenderPadMax = 21, kRenderPadDefault = 19;

// trim / pad for a render pad of M * 2^-exponent; 0 for exponent 0 (no trim).  Exact.
HIPPT_SL float trim_scale(int exponent) {
    return exponent >= kRenderPadMin && exponent <= kRenderPadMax ? 1.0f - ldexpf(1.0f, kPadExponent - exponent) : 0.0f;
}
// The distance every plane moves inward (one rounding, below 2^-24 of the pad).
HIPPT_SL float trim_of(float pad, float scale) { return pad * scale; }
// A padded lo / hi plane trimmed (one rounding each, at most half an ulp of the plane).  An unused
// slot's far point (bvh_builder.h kFarPoint, magnitudes >= 1e20) is unchanged by any trim.
HIPPT_SL float trim_lo(float lo, float trim) { return lo + trim; }
HIPPT_SL float trim_hi(float hi, float trim) { return hi - trim; }

// ---- the ray queries' box test: a per-ray slack and a relative direction clamp ----------------------
// The builder's pad covers the rounding of the test above for rays that start within a few M of the
// scene.  A query's ray may start anywhere: at |o| = K * M the terms o * inv and plane * inv - oi are
// about K * M * |inv| and round by 2^-24 of that, which exceeds the pad's pad * |inv| from K of a few
// hundred on; and the absolute 1e-20 of clamp_dir replaces every component of a short direction.  The
// queries therefore prepare their rays with the functions below (hippt_ray_loop.h prepare_query;
// tests/native/far_model.cpp measures them, DESIGN.md §5 "Query slack"):
//   floor = max(dmax * 2^-40, reach * 2^-120)     dmax, omax: the largest |component| of the direction
//                                                 and the origin; reach = omax + M
//   inv   = rcp(clamp(d, floor))                  per axis, the caller's reciprocal
//   oi    = o * inv,  s = kQuerySlack * away * |inv|    away = max(omax - 2 M, 0): every box grown by
//                                                 kQuerySlack * away (the oracle's own t errs by ulps
//                                                 of |o| / |d|, whichever axis the box is thin on)
//   near planes use oi + s, far planes oi - s     (plane_t: the near t moves down, the far t up, by s)
//   an axis whose component was clamped: its far planes use oi - (s + tb), tb = 2 * reach * min |inv|
// tb bounds every hit's t (the hit lies within M of the origin's frame on the longest axis), so a far
// plane of a clamped axis, whose true crossing lies beyond the computed one, never ends a ray early;
// its near plane errs on the safe side by itself.  The node loop is the same instructions over two
// origin terms per axis.
constexpr float kQuerySlack = 128.0f * 0x1p-24f;  // 4 x the measured requirement, a power of two

HIPPT_SL float query_dir_floor(float dmax, float reach) { return fmaxf(dmax * 0x1p-40f, reach * 0x1p-120f); }
HIPPT_SL float query_clamp_dir(float d, float floor) { return copysignf(fmaxf(fabsf(d), floor), d); }
HIPPT_SL float query_far_bound(float reach, float invMin) { return 2.0f * reach * invMin; }
// How far outside the builder's assumption the origin lies: 0 within 2 M (the pad alone covers such
// rays, and their box tests are the parent's bit for bit), else its largest |component| less 2 M.
HIPPT_SL float query_away(float omax, float M) { return fmaxf(omax - 2.0f * M, 0.0f); }

// An axis' two origin terms from its reciprocal (of query_clamp_dir(d, floor)); slack: kQuerySlack
// in the kernels, the model varies it.
HIPPT_SL void query_origin_terms(float o, float d, float inv, float floor, float tb, float away, float slack,
                                 float &oiNear, float &oiFar) {
    const float oi = origin_term(o, inv);
    const float s = (slack * away) * fabsf(inv);
    oiNear = oi + s;
    oiFar = oi - (fabsf(d) < floor ? s + tb : s);
}

// A scene with spheres: the oracle's sphere test squares (o - c) . d and multiplies |d|^2 by |o - c|^2,
// which overflow from about dmax * reach = 2^62 on; what it then accepts (a hit at t = 0, say) is no
// point of the ray that a box could enclose.  Such a ray takes every box: near terms +inf and far
// terms -inf make every plane's t -inf / +inf, and the traversal is the oracle's loop over all primitives.
HIPPT_SL bool query_all_boxes(float dmax, float reach) { return dmax * reach >= 0x1p60f; }
constexpr float kAllBoxesNear = __builtin_inff();

// box_hit over the two origin terms.
HIPPT_SL bool box_hit_query(float nx, float fx, float ny, float fy, float nz, float fz, float ix, float iy, float iz,
                            float onx, float ony, float onz, float ofx, float ofy, float ofz, float tmin, float bestT,
                            float &n) {
    const float ax = plane_t(nx, ix, onx), bx = plane_t(fx, ix, ofx);
    const float ay = plane_t(ny, iy, ony), by = plane_t(fy, iy, ofy);
    const float az = plane_t(nz, iz, onz), bz = plane_t(fz, iz, ofz);
    n = entry_t(ax, ay, az, tmin);
    const float f = exit_t(bx, by, bz, bestT);
    return HIPPT_SLAB_MEETS(n, f);
}

}  // namespace slab
}  // namespace hippt
