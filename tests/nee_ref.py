"""The reference of light sampling (include/hippt.h HIPPT_OPT_LIGHT_SAMPLING, DESIGN.md §2 "Light sampling"):
emit_ref.EmitRef extended by next-event estimation at Lambertian vertices.  This file is the statement of
record of the rule; the GPU matches it bit for bit.

A path carries Lacc = (0, 0, 0) and spec = True (the last scatter was not Lambertian, or there was none yet).

  hit on a light     ends the path, before the depth check: L = Lacc + thr * Le if spec, else L = Lacc
  miss               L = Lacc + thr * sky
  depth, absorbed    L = Lacc
  Metal, Dielectric  the oracle's po_scatter, spec = True
  Lambertian         (a hit with depth + 1 < maxDepth) po_scatter first: it gives p (the new origin), thr' and
                     the advanced RNG state; n is hit_ref's faced normal of the hit; spec = False.  Then, from
                     the same RNG state:
    k   = min(int(rand01 * float32(nLights)), nLights - 1)    lights: emissive primitives, ascending id
    triangle (v0, e1, e2, unit normal ng):  a = rand01, b = rand01; if a + b > 1: a = 1 - a, b = 1 - b
        q = fmaf(b, e2, fmaf(a, e1, v0)); A = 0.5 * sqrt(fdot(c, c)), c = fcross(e1, e2); nl = ng
    sphere (c, r):  u = draw * (1 / sqrt(|draw|^2)), draw = po_random_in_unit_sphere (scatter's own draw)
        q = fmaf(r, u, c); nl = u; A = (12.566371 * r) * r
    w = q - p; d2 = fdot(w, w); il = 1 / sqrt(d2); om = w * il; cosS = fdot(n, om); sL = fdot(nl, om)
    triangle: cosL = |sL|;  sphere: cosL = -sL if fdot(p - c, p - c) >= r * r else sL
    unless cosS > 0 and cosL > 0 and d2 > 0 and A > 0: no shadow ray (the draws are consumed all the same)
    g  = (((cosS * cosL) * A) * float32(nLights)) / (3.14159274 * d2);  Ld = (thr' * Le) * g
    the shadow ray (p, om), tmin 0.001, no tmax: Ref.closest; it counts as a segment; if its closest hit is
    light k: Lacc += Ld.  The path goes on along the scattered ray.

Every product, sum, quotient and square root is one float32 operation (numpy float32 scalars), fmaf the C
library's.  With `sample` False, or no light in the scene, no connection is made and spec stays True: the
paths are EmitRef's (tests/test_nee_ref_cpu.py asserts it, and PathRef's for a scene without a light)."""
import ctypes
import functools

import numpy as np

import emit_ref as er
import hippt
import path_ref as pr
import pyoracle as po
from hippt import scenes
from hit_ref import HitRef, f3, fcross, fdot, fmaf
from path_ref import ABSORBED, DEPTH, INVALID, MISS, F, INF  # noqa: F401 (re-exported ends)

EMITTED = er.EMITTED
PU32 = ctypes.POINTER(ctypes.c_uint32)
PI = F(3.14159274)
FOUR_PI = F(12.566371)

# what happened at the vertices of a path (detail["events"], a bit mask)
VISIBLE = 1      # a shadow ray reached its light with Ld > 0
OCCLUDED = 2     # a shadow ray ended on something else
BACKFACING = 4   # no shadow ray: cosS <= 0
FAR_SIDE = 8     # no shadow ray: the far side of a sphere light seen from outside
LIGHT_AFTER_DIFFUSE = 16  # the path ended on a light after a Lambertian bounce (adds 0)
LIGHT_SPECULAR = 32       # the path ended on a light at segment 0 or after Metal / Dielectric (adds emission)
EVENTS = {"visible": VISIBLE, "occluded": OCCLUDED, "backfacing": BACKFACING, "far side": FAR_SIDE,
          "light after diffuse": LIGHT_AFTER_DIFFUSE, "light specular": LIGHT_SPECULAR}


class NeeRef(er.EmitRef):
    """The paths with light sampling over a scene; `ref` is its test_gpu_ray_query.Ref."""

    def __init__(self, sc, ref, sample=True):
        super().__init__(sc, ref)
        self.hits = HitRef(sc, ref)
        self.lights = [int(i) for i in np.flatnonzero(self.prim_kind == scenes.MAT_EMISSIVE)]  # ascending id
        self.sample = bool(sample)

    def light_point(self, k, st):
        """(q, nl, A, sphere (c, r) or None) of a point drawn on light k from RNG state st (advanced)."""
        L = po.lib()
        if k < self.hits.ntris:
            tri = self.ref.tris[k]
            v0, e1, e2 = f3(tri.v0), f3(tri.e1), f3(tri.e2)
            a = F(L.po_rand01(ctypes.byref(st)))
            b = F(L.po_rand01(ctypes.byref(st)))
            if a + b > F(1.0):
                a, b = F(1.0) - a, F(1.0) - b
            q = tuple(fmaf(b, e2[i], fmaf(a, e1[i], v0[i])) for i in range(3))
            c = fcross(e1, e2)
            return q, f3(tri.n), F(0.5) * np.sqrt(fdot(c, c)), None
        s = self.hits.spheres[k - self.hits.ntris]
        c, r = f3(s[0:3]), F(s[3])
        draw = (ctypes.c_float * 3)()
        L.po_random_in_unit_sphere(ctypes.byref(st), draw)
        dr = f3(draw)
        r2 = fdot(dr, dr)
        inv = F(np.inf) if r2 == 0 else F(1.0) / np.sqrt(r2)
        u = tuple(dr[i] * inv for i in range(3))
        return tuple(fmaf(r, u[i], c[i]) for i in range(3)), u, (FOUR_PI * r) * r, (c, r)

    def connect(self, p, n, thr, st):
        """The connection from vertex p (faced normal n, throughput thr after the scatter) with RNG state st
        (advanced): (Ld or None when no shadow ray is to be traced, om, light id, why skipped)."""
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
        le = self.prim_emission[k]
        return tuple((F(thr[i]) * le[i]) * g for i in range(3)), om, k, 0

    def path(self, ray, seed, max_depth, detail=None):
        """(rgba (4,) float32, segments, how it ended, bit mask of the material kinds it scattered at).
        detail (a dict): "events" the bit mask of what happened on the way (EVENTS), "shadow" the shadow rays
        traced."""
        out = np.zeros(4, F)
        if detail is not None:
            detail["events"], detail["shadow"] = 0, 0
        if not pr.valid(ray):
            return out, 0, INVALID, 0
        nee = self.sample and len(self.lights) > 0
        o = (ctypes.c_float * 3)(*[float(x) for x in ray[0:3]])
        d = (ctypes.c_float * 3)(*[float(x) for x in ray[4:7]])
        thr = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        st = ctypes.c_uint32(int(seed) & 0xFFFFFFFF)
        seg = np.zeros((1, 8), F)
        lacc = np.zeros(3, F)
        spec = True
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
                    out[0:3] = lacc + np.array(thr[:], F) * self.prim_emission[prim] if spec else lacc
                    events |= LIGHT_SPECULAR if spec else LIGHT_AFTER_DIFFUSE
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
                if not nee:
                    continue
                spec = kind != scenes.MAT_LAMBERTIAN
                if spec:
                    continue
                ld, om, k, why = self.connect(f3(o), n, thr, st)
                events |= why
                if ld is None:
                    continue
                seg[0, 0:3], seg[0, 4:7] = o[:], om
                seg[0, 3], seg[0, 7] = F(0.001), INF
                _, sp = self.ref.closest(seg)
                segs += 1
                shadow += 1
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

    def paths_events(self, rays, seeds, max_depth=pr.MAX_DEPTH):
        """paths() plus (events (n,) int32, shadow rays (n,) int32)."""
        n = len(rays)
        rad = np.zeros((n, 4), F)
        segs, ends, kinds = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        events, shadow = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i in range(n):
            det = {}
            rad[i], segs[i], ends[i], kinds[i] = self.path(rays[i], seeds[i], max_depth, det)
            events[i], shadow[i] = det["events"], det["shadow"]
        return rad, segs, ends, kinds, events, shadow


@functools.lru_cache(maxsize=None)
def scene_ref(name):
    """(scene, NeeRef) of a lit scene (emit_ref.LIT) or a scene of hippt.scenes.SCENES."""
    from test_gpu_ray_query import Ref
    sc = er.lit_scene(name) if name in er.LIT else scenes.get_scene(name)
    return sc, NeeRef(sc, Ref(sc))


@functools.lru_cache(maxsize=None)
def nee_case(name, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds, events, shadow rays) of a lit scene with
    emit_ref.emit_case's rays and seeds (make_rays(sc, 4097), path_seeds(n, 0)); computed once, never
    modified."""
    from test_gpu_ray_query import N, make_rays
    sc, ref = scene_ref(name)
    rays = make_rays(sc, N)
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    out = ref.paths_events(rays, seeds, max_depth)
    for a in (rays, seeds, *out):
        a.setflags(write=False)
    return (sc, rays, seeds) + out


@functools.lru_cache(maxsize=None)
def render_case(name, w=32, h=24, frames=3, max_depth=pr.MAX_DEPTH):
    """(scene, accumulation (h, w, 4), pixel words (h, w), segments, shadow rays among them) of a render with
    light sampling: emit_ref.render_with's loop over NeeRef's paths; computed once, never modified."""
    sc, ref = scene_ref(name)
    L = po.lib()
    acc = np.zeros((h * w, 4), F)
    px = np.zeros(h * w, np.uint32)
    total = shadow = 0
    for f in range(frames):
        rays, seeds = pr.camera_rays_seeds(sc, w, h, f)
        rad, nseg, _, _, _, nshadow = ref.paths_events(rays, seeds, max_depth)
        total += int(nseg.sum())
        shadow += int(nshadow.sum())
        rgb = np.ascontiguousarray(rad[:, :3])
        for i in range(h * w):
            px[i] = L.po_accumulate(acc[i].ctypes.data_as(er.PF), rgb[i].ctypes.data_as(er.PF), f)
    acc, px = acc.reshape(h, w, 4), px.reshape(h, w)
    acc.setflags(write=False)
    px.setflags(write=False)
    return sc, acc, px, total, shadow
