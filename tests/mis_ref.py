"""The reference of light sampling with multiple importance sampling (include/hippt.h HIPPT_OPT_LIGHT_SAMPLING_MODE 2,
DESIGN.md §17): nee_ref.NeeRef with the connection and the light hit after a Lambertian vertex each weighted by
the power heuristic (beta = 2) against the other technique.  This file is the statement of record of the rule;
the GPU matches it bit for bit.

A path carries Lacc = (0, 0, 0) and cb = -1 in place of NeeRef's spec: cb < 0 means that the last scatter was not
Lambertian or that there was none yet; otherwise cb is the cosine between the faced normal and the scattered
direction of the last (Lambertian) scatter, whose solid-angle density is cb / pi.

  Lambertian         po_scatter first, as in NeeRef; with sd the scattered direction it leaves and n the faced normal
                     cb = fdot(n, sd) * (1 / sqrt(fdot(sd, sd)))
                     then NeeRef's connection (the same draws, k, q, A, cosS, cosL, d2, skip conditions and g), and
    unless g < +inf: no shadow ray
    Ld = (thr' * Le) * (g / fmaf(g, g, 1))            g = p_b / p_l, so g / (1 + g^2) = g * p_l^2 / (p_l^2 + p_b^2)
  Metal, Dielectric  po_scatter, cb = -1
  hit on a light     ends the path, before the depth check, at t on the segment (o, d):
    cb < 0:   L = Lacc + thr * Le                                            (NeeRef's spec)
    else:     L = Lacc + (thr * Le) * wb, with
        dd = fdot(d, d); d2 = (t * t) * dd; om = d * (1 / sqrt(dd))
        nl = the triangle's unit normal, or (fmaf(t, d, o) - c) / r for a sphere (hit_ref's unfaced normal)
        cosL = |fdot(nl, om)|; A = the light's area as in the connection
        if cb > 0 and cosL > 0 and d2 > 0 and A > 0:
            gh = (((cb * cosL) * A) * float32(nLights)) / (3.14159274 * d2); s = gh * gh
            if s < +inf: wb = s / fmaf(gh, gh, 1)                            p_b^2 / (p_b^2 + p_l^2)
        in every other case wb = 1 (light sampling could not have produced the point)
  miss, depth, absorbed, the shadow ray, the segment counts: NeeRef's.

Fixed here beyond the rule's text: every product, sum, quotient and square root is one float32 operation;
1 / sqrt(x) is the quotient float32(1) / sqrt(x) of the correctly rounded root; (thr * Le) is formed first and
the weight multiplies it; (t * t) is formed before * dd; the comparison "cb < 0" decides the hit's branch, so a
NaN cb takes the weighted branch and, failing cb > 0 there, wb = 1; the area of a triangle light is
0.5 * sqrt(fdot(c, c)), c = fcross(e1, e2), of a sphere (12.566371 * r) * r, whatever side is hit.
With no light in the scene the paths are NeeRef's, which are PathRef's (tests/test_mis_ref_cpu.py)."""
import ctypes
import functools

import numpy as np

import emit_ref as er
import hippt
import nee_ref as nr
import path_ref as pr
import pyoracle as po
from hippt import scenes
from hit_ref import f3, fcross, fdot, fmaf
from nee_ref import (ABSORBED, BACKFACING, DEPTH, EMITTED, FAR_SIDE, INVALID, LIGHT_AFTER_DIFFUSE,  # noqa: F401
                     LIGHT_SPECULAR, MISS, OCCLUDED, PI, VISIBLE, F, INF)

# further event bits (detail["events"]); NeeRef's keep their meaning: LIGHT_AFTER_DIFFUSE is a light hit with
# cb >= 0 (it no longer adds 0), LIGHT_SPECULAR one with cb < 0
WEIGHTED_HIT = 64                    # a light hit with cb >= 0 whose wb came from the formula
WEIGHTED_CONNECTION = 128            # a shadow ray was traced for a connection with the weight g / (1 + g^2)
UNWEIGHTED_HIT_AFTER_DIFFUSE = 256   # a light hit with cb >= 0 and wb = 1
INFINITE_G = 512                     # no shadow ray: g is not below +inf
EVENTS = dict(nr.EVENTS, **{"weighted hit": WEIGHTED_HIT, "weighted connection": WEIGHTED_CONNECTION,
                            "unweighted hit after diffuse": UNWEIGHTED_HIT_AFTER_DIFFUSE, "infinite g": INFINITE_G})


class MisRef(nr.NeeRef):
    """The paths with light sampling and the power heuristic over a scene; `ref` is its test_gpu_ray_query.Ref."""

    def area(self, k):
        """The area of primitive k as the connection forms it."""
        if k < self.hits.ntris:
            tri = self.ref.tris[k]
            c = fcross(f3(tri.e1), f3(tri.e2))
            return F(0.5) * np.sqrt(fdot(c, c))
        r = F(self.hits.spheres[k - self.hits.ntris][3])
        return (nr.FOUR_PI * r) * r

    def connect(self, p, n, thr, st):
        """NeeRef.connect with the weight: Ld = (thr * Le) * (g / fmaf(g, g, 1)), and no shadow ray unless
        g < +inf (why = INFINITE_G)."""
        nl_count = len(self.lights)
        u0 = F(po.lib().po_rand01(ctypes.byref(st)))
        k = self.lights[min(int(u0 * F(nl_count)), nl_count - 1)]
        q, nl, A, sph = self.light_point(k, st)
        w = tuple(q[i] - p[i] for i in range(3))
        d2 = fdot(w, w)
        il = F(1.0) / np.sqrt(d2)
        om = tuple(w[i] * il for i in range(3))
        cos_s = fdot(n, om)
        s_l = fdot(nl, om)
        why = 0
        if sph is None:
            cos_l = np.abs(s_l)
        else:
            c, r = sph
            oc = tuple(p[i] - c[i] for i in range(3))
            outside = bool(fdot(oc, oc) >= r * r)
            cos_l = -s_l if outside else s_l
            if outside and not cos_l > 0:
                why = FAR_SIDE
        if not cos_s > 0:
            why = BACKFACING
        if not cos_s > 0 or not cos_l > 0 or not d2 > 0 or not A > 0:
            return None, om, k, why
        g = (((cos_s * cos_l) * A) * F(nl_count)) / (PI * d2)
        if not g < INF:
            return None, om, k, INFINITE_G
        wg = g / fmaf(g, g, F(1.0))
        le = self.prim_emission[k]
        return tuple((F(thr[i]) * le[i]) * wg for i in range(3)), om, k, 0

    def hit_weight(self, prim, t, o, d, cb):
        """wb of a light hit with cb >= 0 at t on the segment (o, d), and whether the formula gave it."""
        dd = fdot(d, d)
        d2 = (t * t) * dd
        inv = F(1.0) / np.sqrt(dd)
        om = tuple(d[i] * inv for i in range(3))
        nl = self.hits.normal(prim, t, o, d)[0]
        cos_l = np.abs(fdot(nl, om))
        A = self.area(prim)
        if cb > 0 and cos_l > 0 and d2 > 0 and A > 0:
            gh = (((cb * cos_l) * A) * F(len(self.lights))) / (PI * d2)
            s = gh * gh
            if s < INF:
                return s / fmaf(gh, gh, F(1.0)), True
        return F(1.0), False

    def path(self, ray, seed, max_depth, detail=None):
        """NeeRef.path's results under the rule above."""
        if not len(self.lights) or not self.sample:
            return super().path(ray, seed, max_depth, detail)
        out = np.zeros(4, F)
        if detail is not None:
            detail["events"], detail["shadow"] = 0, 0
        if not pr.valid(ray):
            return out, 0, INVALID, 0
        o = (ctypes.c_float * 3)(*[float(x) for x in ray[0:3]])
        d = (ctypes.c_float * 3)(*[float(x) for x in ray[4:7]])
        thr = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        st = ctypes.c_uint32(int(seed) & 0xFFFFFFFF)
        seg = np.zeros((1, 8), F)
        lacc = np.zeros(3, F)
        cb = F(-1.0)
        segs, kinds, end, events, shadow = 0, 0, DEPTH, 0, 0
        with np.errstate(all="ignore"):
            for depth in range(max_depth):
                seg[0, 0:3], seg[0, 4:7] = o[:], d[:]
                seg[0, 3], seg[0, 7] = (ray[3], ray[7]) if depth == 0 else (F(0.001), INF)
                t, p = self.ref.closest(seg)
                segs += 1
                prim = int(p[0])
                if prim < 0:
                    out[0:3] = lacc + np.array(pr.sky(tuple(F(x) for x in d[:]), thr[:]), F)
                    end = MISS
                    break
                if depth == 0:
                    out[3] = 1.0
                if self.prim_kind[prim] == scenes.MAT_EMISSIVE:  # before the depth check
                    le = np.array(thr[:], F) * self.prim_emission[prim]
                    if cb < 0:
                        out[0:3] = lacc + le
                        events |= LIGHT_SPECULAR
                    else:
                        wb, formula = self.hit_weight(prim, F(t[0]), f3(o), f3(d), cb)
                        out[0:3] = lacc + le * wb
                        events |= LIGHT_AFTER_DIFFUSE | (WEIGHTED_HIT if formula else UNWEIGHTED_HIT_AFTER_DIFFUSE)
                    end = EMITTED
                    break
                if depth + 1 >= max_depth:
                    out[0:3] = lacc
                    break
                kind = int(self.prim_kind[prim])
                kinds |= 1 << kind
                n = self.hits.normal(prim, F(t[0]), f3(o), f3(d))[1]
                if not self.L.po_scatter(self.ora.handle, prim, float(t[0]), o, d, ctypes.byref(st), thr):
                    out[0:3] = lacc
                    end = ABSORBED
                    break
                if kind != scenes.MAT_LAMBERTIAN:
                    cb = F(-1.0)
                    continue
                sd = f3(d)
                cb = fdot(n, sd) * (F(1.0) / np.sqrt(fdot(sd, sd)))
                ld, om, k, why = self.connect(f3(o), n, thr, st)
                events |= why
                if ld is None:
                    continue
                seg[0, 0:3], seg[0, 4:7] = o[:], om
                seg[0, 3], seg[0, 7] = F(0.001), INF
                _, sp = self.ref.closest(seg)
                segs += 1
                shadow += 1
                events |= WEIGHTED_CONNECTION
                if int(sp[0]) == k:
                    lacc = lacc + np.array(ld, F)
                    if max(ld) > 0:
                        events |= VISIBLE
                else:
                    events |= OCCLUDED
            else:
                out[0:3] = lacc
        if detail is not None:
            detail["events"], detail["shadow"] = events, shadow
        return out, segs, end, kinds


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def scene_ref(name):
    """(scene, MisRef) of a lit scene (emit_ref.LIT), a scene of lit_scenes.SETS or one of hippt.scenes.SCENES;
    the scene object and its Ref are nee_ref's or lit_scenes' own."""
    import lit_scenes as ls
    if name in ls.SETS:
        sc, nee, _ = ls.scene_refs(name)
    else:
        sc, nee = nr.scene_ref(name)
    return sc, MisRef(sc, nee.ref)


@functools.lru_cache(maxsize=None)
def mis_case(name, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds, events, shadow rays) under the MIS rule, with
    nee_ref.nee_case's rays and seeds for a scene of emit_ref.LIT and lit_scenes.rays_seeds' for one of
    lit_scenes.SETS; computed once, never modified."""
    import lit_scenes as ls
    sc, ref = scene_ref(name)
    if name in ls.SETS:
        rays, seeds = ls.rays_seeds(name)
    else:
        from test_gpu_ray_query import N, make_rays
        rays = make_rays(sc, N)
        seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    return (sc, rays, seeds) + _frozen(ref.paths_events(rays, seeds, max_depth))


@functools.lru_cache(maxsize=None)
def render_case(name, w=32, h=24, frames=3, max_depth=pr.MAX_DEPTH):
    """(scene, accumulation (h, w, 4), pixel words (h, w), segments, shadow rays among them) of a render under
    the MIS rule (lit_scenes.render_nee's loop); computed once, never modified."""
    import lit_scenes as ls
    sc, ref = scene_ref(name)
    return (sc,) + _frozen(ls.render_nee(ref, sc, w, h, frames, max_depth))
