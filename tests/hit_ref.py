"""The reference of the hit records (include/hippt.h hipptHit), restated per ray from the oracle's
arithmetic (oracle/pt_oracle.c) in float32, with the C library's correctly rounded fmaf: every
product, sum and quotient below is one float32 operation, and fdot / fcross are written as the
oracle writes them.

(t, prim) come from test_gpu_ray_query.Ref.closest; the other six words are formed here:
  normal    triangles: po_tri_setup's n; spheres: (p - c) / r at p = fmaf(t, d, o); negated unless
            fdot(d, n) < 0 (po_scatter's n)
  u, v      un / det and vn / det of po_tri_hit; 0 for spheres
  matFlags  the material index, | HIT_SPHERE for a sphere, | HIT_BACKFACE when the normal was negated
A miss is (inf, -1, 0, 0, 0, 0, 0, -1).  tests/test_hit_records_cpu.py pins the restatement to the
oracle (po_tri_hit's t, po_scatter's origin and direction) before any GPU test relies on it."""
import ctypes
import ctypes.util
import functools

import numpy as np

import hippt
import pyoracle as po

F = np.float32
PF = ctypes.POINTER(ctypes.c_float)

_m = ctypes.CDLL(ctypes.util.find_library("m"))
_m.fmaf.restype = ctypes.c_float
_m.fmaf.argtypes = [ctypes.c_float] * 3


def fmaf(a, b, c):
    return F(_m.fmaf(float(a), float(b), float(c)))


def fdot(a, b):
    return fmaf(a[0], b[0], fmaf(a[1], b[1], a[2] * b[2]))


def fcross(a, b):
    return (fmaf(a[1], b[2], -(a[2] * b[1])), fmaf(a[2], b[0], -(a[0] * b[2])), fmaf(a[0], b[1], -(a[1] * b[0])))


def f3(p):
    return (F(p[0]), F(p[1]), F(p[2]))


def scatter_lib():
    """liboracle.so with po_scatter's signature set (pyoracle binds the rest)."""
    L = po.lib()
    L.po_scatter.restype = ctypes.c_int
    L.po_scatter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, PF, PF, ctypes.POINTER(ctypes.c_uint32), PF]
    return L


def tri_terms(tri, o, d):
    """po_tri_hit's (det, un, vn, fdot(e2, qv)) of PoTri `tri` and the ray (o, d)."""
    e1, e2 = f3(tri.e1), f3(tri.e2)
    pv = fcross(d, e2)
    det = fdot(e1, pv)
    tv = tuple(o[k] - F(tri.v0[k]) for k in range(3))
    un = fdot(tv, pv)
    qv = fcross(tv, e1)
    vn = fdot(d, qv)
    return det, un, vn, fdot(e2, qv)


def at(o, d, t):
    """Ray::at: fmaf(t, d, o) per component."""
    return tuple(fmaf(t, d[k], o[k]) for k in range(3))


class HitRef:
    """The attribute words over a scene; `ref` is its test_gpu_ray_query.Ref (PoTri array, spheres)."""

    def __init__(self, sc, ref):
        self.ref = ref
        self.ntris = ref.ntris
        self.tri_mat = np.ascontiguousarray(sc.tri_mat, np.int32)
        self.spheres = np.ascontiguousarray(sc.spheres, F).reshape(-1, 4)
        self.sph_mat = np.ascontiguousarray(sc.sph_mat, np.int32)

    def normal(self, prim, t, o, d):
        """(unfaced normal, faced normal, front) of the hit of primitive `prim` at t."""
        if prim < self.ntris:
            n = f3(self.ref.tris[prim].n)
        else:
            c = self.spheres[prim - self.ntris]
            p = at(o, d, t)
            n = tuple((p[k] - c[k]) / c[3] for k in range(3))
        front = bool(fdot(d, n) < F(0.0))
        return n, (n if front else tuple(-x for x in n)), front

    def records(self, rays, t, prim):
        """HIT_DTYPE (n,) for rays (n, 8) with their reference (t, prim)."""
        out = np.zeros(len(rays), hippt.HIT_DTYPE)
        out["t"] = np.inf
        out["prim"] = -1
        out["matFlags"] = -1
        with np.errstate(all="ignore"):
            for i in np.flatnonzero(np.asarray(prim) >= 0):
                p = int(prim[i])
                o, d = f3(rays[i, 0:3]), f3(rays[i, 4:7])
                _, n, front = self.normal(p, F(t[i]), o, d)
                if p < self.ntris:
                    det, un, vn, _ = tri_terms(self.ref.tris[p], o, d)
                    u, v, mf = un / det, vn / det, int(self.tri_mat[p])
                else:
                    u, v, mf = F(0.0), F(0.0), int(self.sph_mat[p - self.ntris]) | hippt.HIT_SPHERE
                if not front:
                    mf |= hippt.HIT_BACKFACE
                out[i] = (t[i], p, n, u, v, mf)
        return out


@functools.lru_cache(maxsize=None)
def hit_case(name):
    """(scene, rays, t, prim, Ref, HitRef, records) of a named case of test_gpu_ray_query.case; computed
    once, never modified."""
    from test_gpu_ray_query import Ref, case
    sc, rays, t, p = case(name)
    ref = Ref(sc)
    href = HitRef(sc, ref)
    rec = href.records(rays, t, p)
    rec.setflags(write=False)
    return sc, rays, t, p, ref, href, rec


def assert_records(got, want, what=""):
    """All 8 words of every record bit-identical."""
    got = np.ascontiguousarray(got).reshape(-1)
    want = np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == hippt.HIT_DTYPE and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(w)} records differ, first {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"
