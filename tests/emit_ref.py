"""The reference of emissive materials (include/hippt.h HIPPT_MAT_EMISSIVE): path_ref.PathRef
with one more way for a path to end.  A segment whose closest hit is a primitive with an emissive material
ends the path there with rgb = throughput * emission, one numpy float32 multiply per channel, before the
depth check, without an RNG draw; the segment counts, and a = 1 if it was segment 0.

The oracle knows no such material, and never scatters at one, so its handle (po_scatter's scene) is built
from the scene with the emissive kinds replaced by Lambertian.  The closest hit is the same Ref.closest.
The render reference takes each pixel's ray and RNG state of each frame from path_ref.camera_rays_seeds and
feeds the path's rgb through the oracle's po_accumulate.

tests/test_emit_ref_cpu.py pins this restatement to PathRef before any GPU test relies on it."""
import copy
import ctypes
import functools

import numpy as np

import hippt
import path_ref as pr
import pyoracle as po
from hippt import scenes
from path_ref import ABSORBED, DEPTH, INVALID, MISS, F, INF  # noqa: F401 (re-exported ends)

EMITTED = 4
PF = ctypes.POINTER(ctypes.c_float)

# the lit scenes of the tests: hippt.scenes.cornell_lit(base, sphere)
LIT = {"cornell34_lit": ("cornell34", True), "cornell_mixed_lit": ("cornell_mixed", True),
       "cornell34_lit_tris": ("cornell34", False)}


def lambertian_substitute(sc):
    """sc with every emissive material's kind replaced by Lambertian (albedo words kept)."""
    out = copy.copy(sc)
    if sc.mat_kind is not None:
        k = np.array(sc.mat_kind, np.int32)
        k[k == scenes.MAT_EMISSIVE] = scenes.MAT_LAMBERTIAN
        out.mat_kind = k
    return out


class EmitRef(pr.PathRef):
    """The paths over a scene that may hold emissive materials; `ref` is its test_gpu_ray_query.Ref."""

    def __init__(self, sc, ref):
        super().__init__(lambertian_substitute(sc), ref)
        m = sc.materials()
        self.prim_kind = np.concatenate([m["kind"][np.asarray(sc.tri_mat, np.int64)],
                                         m["kind"][np.asarray(sc.sph_mat, np.int64)]]).astype(np.int32)
        self.prim_emission = np.concatenate([m["albedo"][np.asarray(sc.tri_mat, np.int64)],
                                             m["albedo"][np.asarray(sc.sph_mat, np.int64)]]).astype(F).reshape(-1, 3)

    def path(self, ray, seed, max_depth, detail=None):
        """(rgba (4,) float32, segments, how it ended, bit mask of the material kinds it scattered at).
        detail (a dict): "thr" the throughput at the path's end, "prim" the primitive of the last hit (-1)."""
        out = np.zeros(4, F)
        if detail is not None:
            detail["thr"], detail["prim"] = np.ones(3, F), -1
        if not pr.valid(ray):
            return out, 0, INVALID, 0
        o = (ctypes.c_float * 3)(*[float(x) for x in ray[0:3]])
        d = (ctypes.c_float * 3)(*[float(x) for x in ray[4:7]])
        thr = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        st = ctypes.c_uint32(int(seed) & 0xFFFFFFFF)
        seg = np.zeros((1, 8), F)
        segs, kinds, end, prim = 0, 0, DEPTH, -1
        with np.errstate(all="ignore"):
            for depth in range(max_depth):
                seg[0, 0:3], seg[0, 4:7] = o[:], d[:]
                seg[0, 3], seg[0, 7] = (ray[3], ray[7]) if depth == 0 else (F(0.001), INF)
                t, p = self.ref.closest(seg)
                segs += 1
                prim = int(p[0])
                if prim < 0:
                    out[0:3] = pr.sky(tuple(F(x) for x in d[:]), thr[:])
                    end = MISS
                    break
                if depth == 0:
                    out[3] = 1.0
                if self.prim_kind[prim] == scenes.MAT_EMISSIVE:  # before the depth check
                    out[0:3] = np.array(thr[:], F) * self.prim_emission[prim]
                    end = EMITTED
                    break
                if depth + 1 >= max_depth:
                    break
                kinds |= 1 << int(self.prim_kind[prim])
                if not self.L.po_scatter(self.ora.handle, prim, float(t[0]), o, d, ctypes.byref(st), thr):
                    end = ABSORBED
                    break
        if detail is not None:
            detail["thr"], detail["prim"] = np.array(thr[:], F), prim
        return out, segs, end, kinds

    def paths_detail(self, rays, seeds, max_depth=pr.MAX_DEPTH):
        """paths() plus (throughput at the end (n, 3) float32, primitive of the last hit (n,))."""
        n = len(rays)
        rad = np.zeros((n, 4), F)
        segs, ends, kinds = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        thr, prim = np.ones((n, 3), F), np.full(n, -1, np.int32)
        for i in range(n):
            det = {}
            rad[i], segs[i], ends[i], kinds[i] = self.path(rays[i], seeds[i], max_depth, det)
            thr[i], prim[i] = det["thr"], det["prim"]
        return rad, segs, ends, kinds, thr, prim


def lit_scene(name):
    base, sphere = LIT[name]
    return scenes.cornell_lit(base, sphere)


@functools.lru_cache(maxsize=None)
def _scene_ref(name):
    from test_gpu_ray_query import Ref
    sc = lit_scene(name) if name in LIT else scenes.get_scene(name)
    return sc, EmitRef(sc, Ref(sc))


@functools.lru_cache(maxsize=None)
def emit_case(name, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds, throughput, last primitive) of a lit scene (LIT) or
    a scene of hippt.scenes.SCENES with test_gpu_ray_query.make_rays(sc, 4097) and path_seeds(n, 0); computed
    once, never modified."""
    from test_gpu_ray_query import N, make_rays
    sc, ref = _scene_ref(name)
    rays = make_rays(sc, N)
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    out = ref.paths_detail(rays, seeds, max_depth)
    for a in (rays, seeds, *out):
        a.setflags(write=False)
    return (sc, rays, seeds) + out


def render_with(ref, sc, w, h, frames, max_depth=pr.MAX_DEPTH):
    """(accumulation (h, w, 4) float32, pixel words (h, w) uint32, segments, ends (frames, h * w), segments per
    path (frames, h * w)) of frames 0..frames-1 over scene sc with its paths from `ref`."""
    L = po.lib()
    acc = np.zeros((h * w, 4), F)
    px = np.zeros(h * w, np.uint32)
    ends = np.zeros((frames, h * w), np.int32)
    nseg = np.zeros((frames, h * w), np.int32)
    for f in range(frames):
        rays, seeds = pr.camera_rays_seeds(sc, w, h, f)
        rad, nseg[f], ends[f], _ = ref.paths(rays, seeds, max_depth)
        rgb = np.ascontiguousarray(rad[:, :3])
        for i in range(h * w):
            px[i] = L.po_accumulate(acc[i].ctypes.data_as(PF), rgb[i].ctypes.data_as(PF), f)
    return acc.reshape(h, w, 4), px.reshape(h, w), int(nseg.sum()), ends, nseg


@functools.lru_cache(maxsize=None)
def render_case(name, w=32, h=24, frames=3, max_depth=pr.MAX_DEPTH):
    """(scene,) + render_with's results for a named scene; computed once, never modified."""
    sc, ref = _scene_ref(name)
    out = render_with(ref, sc, w, h, frames, max_depth)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return (sc,) + out
