"""The reference of the path queries (include/hippt.h hipptTraceRadiance, hipptCameraRays), restated per
ray from the oracle's own pieces: po_mesh_sample (oracle/pt_oracle.c) from its line
`float thr[3] = {1,1,1}` on, with the closest hit of test_gpu_ray_query.Ref.closest (one ray at a time),
the oracle's po_scatter on a pyoracle.MeshScene handle, and the sky's four float32 operations
((1/sqrtf(dot))*d.y, 0.5f*(uy+1), 1-a, fmaf) with the C library's fmaf.  Segment 0 uses the ray's own
tmin and exclusive tmax, every later one 0.001 and inf.  An invalid ray (the query contract's: non-finite
origin, direction or tmin, NaN tmax, zero direction, tmin < 0, tmax <= tmin) is (0, 0, 0, 0), 0 segments.

tests/test_path_ref_cpu.py pins this restatement to MeshScene.sample before any GPU test relies on it.

The GPU tests' fixed ray sets are test_gpu_ray_query.case(name)'s rays (make_rays' seed 11, as there) with
hippt.path_seeds(n, frame=SEED_FRAME).  SEED_FRAME = 0 was tried first and kept: with it every set meets
the conditions test_path_ref_cpu.py asserts on the reference alone (paths ended by a primary miss, by
the sky after three or more segments, black by the depth limit, a quarter with two or more segments,
Dielectric and Metal hits where the scene has them)."""
import ctypes
import functools

import numpy as np

import hippt
import pyoracle as po
from hit_ref import fdot, fmaf, scatter_lib

F = np.float32
INF = F(np.inf)
PF = ctypes.POINTER(ctypes.c_float)
SEED_FRAME = 0
MAX_DEPTH = 8

# how a path ended
INVALID, MISS, DEPTH, ABSORBED = 0, 1, 2, 3


def valid(ray) -> bool:
    """The query contract's validity of one ray (8 float32)."""
    o, tmin, d, tmax = ray[0:3], ray[3], ray[4:7], ray[7]
    return bool(np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(tmin) and not np.isnan(tmax)
                and (d != 0).any() and tmin >= 0 and tmax > tmin)


def sky(d, thr):
    """po_mesh_sample's miss: throughput x sky gradient of direction d, in float32."""
    uy = (F(1.0) / np.sqrt(fdot(d, d))) * d[1]
    a = F(0.5) * (uy + F(1.0))
    b = F(1.0) - a
    s = (fmaf(a, F(0.5), b), fmaf(a, F(0.7), b), fmaf(a, F(1.0), b))
    return tuple(F(thr[k]) * s[k] for k in range(3))


class PathRef:
    """The paths over a scene; `ref` is its test_gpu_ray_query.Ref."""

    def __init__(self, sc, ref):
        self.ref = ref
        self.ora = po.MeshScene(sc, 4, 4)  # (the camera is not used)
        self.L = scatter_lib()
        m = sc.materials()
        self.prim_kind = np.concatenate([m["kind"][np.asarray(sc.tri_mat, np.int64)],
                                         m["kind"][np.asarray(sc.sph_mat, np.int64)]]).astype(np.int32)

    def path(self, ray, seed, max_depth):
        """(rgba (4,) float32, segments, how it ended, bit mask of the material kinds it scattered at)."""
        out = np.zeros(4, F)
        if not valid(ray):
            return out, 0, INVALID, 0
        o = (ctypes.c_float * 3)(*[float(x) for x in ray[0:3]])
        d = (ctypes.c_float * 3)(*[float(x) for x in ray[4:7]])
        thr = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        st = ctypes.c_uint32(int(seed) & 0xFFFFFFFF)
        seg = np.zeros((1, 8), F)
        segs, kinds, end = 0, 0, DEPTH
        with np.errstate(all="ignore"):
            for depth in range(max_depth):
                seg[0, 0:3], seg[0, 4:7] = o[:], d[:]
                seg[0, 3], seg[0, 7] = (ray[3], ray[7]) if depth == 0 else (F(0.001), INF)
                t, p = self.ref.closest(seg)
                segs += 1
                if p[0] < 0:
                    out[0:3] = sky(tuple(F(x) for x in d[:]), thr[:])
                    end = MISS
                    break
                if depth == 0:
                    out[3] = 1.0
                if depth + 1 >= max_depth:
                    break
                kinds |= 1 << int(self.prim_kind[p[0]])
                if not self.L.po_scatter(self.ora.handle, int(p[0]), float(t[0]), o, d, ctypes.byref(st), thr):
                    end = ABSORBED
                    break
        return out, segs, end, kinds

    def paths(self, rays, seeds, max_depth=MAX_DEPTH):
        """(radiance (n, 4) float32, segments (n,) int32, ends (n,), kinds (n,)) of rays (n, 8), seeds (n,)."""
        n = len(rays)
        rad = np.zeros((n, 4), F)
        segs, ends, kinds = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i in range(n):
            rad[i], segs[i], ends[i], kinds[i] = self.path(rays[i], seeds[i], max_depth)
        return rad, segs, ends, kinds


def path_ref(sc, rays, seeds, max_depth=MAX_DEPTH):
    """(radiance (N, 4), segments) of the rays over scene sc."""
    from test_gpu_ray_query import Ref
    return PathRef(sc, Ref(sc)).paths(rays, seeds, max_depth)[:2]


@functools.lru_cache(maxsize=None)
def path_case(name, max_depth=MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds) of a named case of test_gpu_ray_query.case with
    path_seeds(n, SEED_FRAME); computed once, never modified."""
    from test_gpu_ray_query import Ref, case
    sc, rays, _, _ = case(name)
    seeds = hippt.path_seeds(len(rays), SEED_FRAME)
    out = PathRef(sc, Ref(sc)).paths(rays, seeds, max_depth)
    for a in (seeds, *out):
        a.setflags(write=False)
    return (sc, rays, seeds) + out


def camera_rays_seeds(sc, w, h, frame):
    """The rays hipptRenderFrames starts sample `frame` with, row-major, and the RNG state each is left with
    after the camera sample (test_gpu_ray_query.camera_rays that also keeps seed.value)."""
    L = po.lib()
    cam = po.scene_camera(sc, w, h)
    inv_w = F(1.0) / F(max(w - 1, 1))
    inv_h = F(1.0) / F(max(h - 1, 1))
    rays = np.zeros((h * w, 8), F)
    rays[:, 3] = 0.001
    rays[:, 7] = INF
    seeds = np.zeros(h * w, np.uint32)
    o, d = (ctypes.c_float * 3)(), (ctypes.c_float * 3)()
    for y in range(h):
        for x in range(w):
            seed = ctypes.c_uint32(L.po_pixel_seed(x, y, w, frame))
            s = (F(x) + F(L.po_rand01(ctypes.byref(seed)))) * inv_w
            t = (F(y) + F(L.po_rand01(ctypes.byref(seed)))) * inv_h
            L.po_camera_get_ray(ctypes.byref(cam), float(s), float(t), ctypes.byref(seed), o, d)
            rays[y * w + x, 0:3] = o[:]
            rays[y * w + x, 4:7] = d[:]
            seeds[y * w + x] = seed.value
    return rays, seeds


def assert_paths(rad, segs, want_rad, want_segs, what=""):
    """All four radiance words and the segment count of every ray bit-identical."""
    rad, segs = np.asarray(rad), np.asarray(segs)
    assert rad.dtype == np.float32 and segs.dtype == np.int32, (rad.dtype, segs.dtype)
    assert rad.shape == want_rad.shape and segs.shape == want_segs.shape, (rad.shape, segs.shape)
    g, w = np.ascontiguousarray(rad).view(np.uint32), np.ascontiguousarray(want_rad).view(np.uint32)
    bad = np.flatnonzero((g != w).any(axis=1) | (segs != want_segs))
    assert bad.size == 0, f"{what}: {bad.size} of {len(w)} paths differ, first {bad[:4]}: {rad[bad[:4]]} / " \
                          f"{segs[bad[:4]]} vs {want_rad[bad[:4]]} / {want_segs[bad[:4]]}"
