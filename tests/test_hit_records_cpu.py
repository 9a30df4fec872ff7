"""Hit records without a GPU: the reference restatement (tests/hit_ref.py) pinned to the oracle, the
condition on the test inputs, and the C ABI of hipptTraceHits / hipptTraceCameraHits (size, exports,
argument errors before any device call).

The pins: on every hit of the four ray sets of test_gpu_ray_query.case,
  * the restated fdot(e2, qv) / det is po_tri_hit's t bit for bit, with u >= 0 and v >= 0 (the
    restated det, un, vn are the oracle's);
  * with every material made Lambertian, po_scatter returns the origin fmaf(t, d, o) and the direction
    n_faced + r * (1 / sqrt(fdot(r, r))), r from po_random_in_unit_sphere on a copy of the RNG state
    (n_faced alone where that sum is shorter than 1e-4, as po_scatter has it): the restated normal and
    facing are po_scatter's, for triangles and spheres."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import hippt
import pyoracle as po
from hippt import scenes
from hit_ref import F, PF, at, f3, fdot, hit_case, scatter_lib, tri_terms
from test_gpu_ray_query import SCENES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(SCENES)


@pytest.mark.parametrize("name", NAMES)
def test_restated_t_is_the_oracles(name):
    sc, rays, rt, rp, ref, _, _ = hit_case(name)
    L = po.lib()
    tt = ctypes.c_float()
    n = 0
    for i in np.flatnonzero((rp >= 0) & (rp < ref.ntris)):
        o, d = f3(rays[i, 0:3]), f3(rays[i, 4:7])
        tri = ref.tris[int(rp[i])]
        det, un, vn, tn = tri_terms(tri, o, d)
        ob, db = np.array(o, F), np.array(d, F)
        assert L.po_tri_hit(ctypes.byref(tri), ob.ctypes.data_as(PF), db.ctypes.data_as(PF), float(rays[i, 3]),
                            ctypes.byref(tt))
        t = tn / det
        assert F(t).tobytes() == F(tt.value).tobytes() == F(rt[i]).tobytes(), (i, t, tt.value, rt[i])
        assert un / det >= 0.0 and vn / det >= 0.0, (i, un, vn, det)
        n += 1
    print(f"{name}: {n} triangle hits pinned")
    assert n > 0 or ref.ntris == 0


@pytest.mark.parametrize("name", NAMES)
def test_restated_normal_and_facing_are_po_scatters(name):
    sc, rays, rt, rp, ref, href, _ = hit_case(name)
    lamb = dataclasses.replace(sc, mat_kind=None, fuzz=None, ir=None)
    ora = po.MeshScene(lamb, 64, 48)
    L = scatter_lib()
    hits = spheres = 0
    for i in np.flatnonzero(rp >= 0):
        o, d = f3(rays[i, 0:3]), f3(rays[i, 4:7])
        prim, t = int(rp[i]), F(rt[i])
        _, n, _ = href.normal(prim, t, o, d)
        state = ctypes.c_uint32(0x1234567 + 977 * int(i))
        draw = ctypes.c_uint32(state.value)
        r = (ctypes.c_float * 3)()
        L.po_random_in_unit_sphere(ctypes.byref(draw), r)
        rv = f3(r)
        inv = F(1.0) / np.sqrt(fdot(rv, rv))
        sd = tuple(n[k] + rv[k] * inv for k in range(3))
        if fdot(sd, sd) < F(1e-8):
            sd = n
        ob, db, thr = np.array(o, F), np.array(d, F), np.ones(3, F)
        assert L.po_scatter(ora.handle, prim, float(t), ob.ctypes.data_as(PF), db.ctypes.data_as(PF),
                            ctypes.byref(state), thr.ctypes.data_as(PF)) == 1
        assert state.value == draw.value
        assert ob.tobytes() == np.array(at(o, d, t), F).tobytes(), (i, prim)
        assert db.tobytes() == np.array(sd, F).tobytes(), (i, prim, db, sd)
        hits += 1
        spheres += prim >= ref.ntris
    print(f"{name}: {hits} hits pinned, {spheres} on spheres")
    assert hits > 0


@pytest.mark.parametrize("name", NAMES)
def test_inputs_hit_both_sides_and_spheres(name):
    """Asserted on the reference alone: per scene at least 10 % of the hits front-facing and 10 %
    back-facing; the scenes with spheres have at least 100 sphere hits."""
    sc, rays, rt, rp, ref, href, rec = hit_case(name)
    hit = rec["prim"] >= 0
    back = np.count_nonzero(rec["matFlags"][hit] < 0)
    front = np.count_nonzero(hit) - back
    sph = np.count_nonzero(rec["matFlags"][hit] & hippt.HIT_SPHERE)
    print(f"{name}: front {front}, back {back}, spheres {sph}")
    assert front >= 0.1 * (front + back) and back >= 0.1 * (front + back)
    if name in ("cornell_mixed", "random_scene"):
        assert sph >= 100
    assert np.all(rec["matFlags"][~hit] == -1) and not rec["normal"][~hit].any()
    assert np.array_equal(sph > 0, ref.r2.shape[0] > 0)


# ---- the C ABI -----------------------------------------------------------------------------------------
def test_abi_size_exports_and_signatures():
    assert ctypes.sizeof(hippt.Hit) == 32 and hippt.HIT_DTYPE.itemsize == 32
    assert [hippt.HIT_DTYPE.fields[k][1] for k in ("t", "prim", "normal", "u", "v", "matFlags")] == [0, 4, 8, 20, 24, 28]
    lib = hippt.load_library()
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    for name in ("hipptTraceHits", "hipptTraceCameraHits"):
        assert name in hippt.EXPORTS
        assert getattr(lib, name).restype is ctypes.c_bool
    assert ("bool hipptTraceHits(const float *rays, long long numRays, int flags, hipptHit *hits, "
            "const char **errorMessage);") in header
    assert "bool hipptTraceCameraHits(int frame, int flags, hipptHit *hits, const char **errorMessage);" in header
    assert re.search(r"HIPPT_HIT_SPHERE\s*=\s*1\s*<<\s*30\b", header) and hippt.HIT_SPHERE == 1 << 30
    assert re.search(r"HIPPT_HIT_BACKFACE\s*=\s*\(int\)\(1u\s*<<\s*31\)", header) and hippt.HIT_BACKFACE == -(1 << 31)


@pytest.fixture()
def lib():
    L = hippt.load_library()
    L.cudaPathTracerShutdown()  # no Init
    yield L
    hippt.PathTracer().useBuiltinScene(hippt.SCENE_SPHERE4)
    L.cudaPathTracerShutdown()


def _calls(L, rays, n, hits, flags=0, frame=0):
    out = []
    for name, call in (("hits", lambda e: L.hipptTraceHits(rays, n, flags, hits, e)),
                       ("camera", lambda e: L.hipptTraceCameraHits(frame, flags, hits, e))):
        e = ctypes.c_char_p()
        ok = call(ctypes.byref(e))
        out.append((name, bool(ok), e.value.decode() if e.value else ""))
    return out


def test_argument_errors_return_false_with_a_message(lib):
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros(4, hippt.HIT_DTYPE)
    R, H = rays.ctypes.data, hits.ctypes.data
    pt = hippt.PathTracer()
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)  # nothing to query
    for name, ok, msg in _calls(lib, R, 4, H):
        assert not ok and "scene" in msg, (name, msg)
    pt.uploadMesh(scenes.cornell34())  # a mesh, but no Init
    for flags in (0, hippt.RAYS_DEVICE):
        for name, ok, msg in _calls(lib, R, 4, H, flags):
            assert not ok and "not initialized" in msg, (name, msg)
    name, ok, msg = _calls(lib, R, -1, H)[0]
    assert not ok and "negative" in msg, msg
    name, ok, msg = _calls(lib, None, 4, H)[0]
    assert not ok and "null" in msg, msg
    for name, ok, msg in _calls(lib, R, 4, None):
        assert not ok and "output" in msg, (name, msg)
    for name, ok, msg in _calls(lib, R, 4, H, flags=6):  # unknown flags: never a success
        assert not ok and msg, (name, msg)
    name, ok, msg = _calls(lib, R, 4, H, frame=-1)[1]
    assert not ok and "negative frame" in msg, msg
    assert not lib.hipptTraceHits(R, 4, 0, H, None)  # a null message pointer is allowed
    assert b"not initialized" in lib.hipptLastError()
    assert not hits.view(np.uint32).any()  # nothing was written


def test_wrapper_validates_before_any_call(lib):
    pt = hippt.PathTracer()
    pt.uploadMesh(scenes.cornell34())
    with pytest.raises(hippt.HipptError, match="shape"):
        pt.traceHits(np.zeros((4, 7), np.float32))
    with pytest.raises(hippt.HipptError, match="float32"):
        pt.traceHits(np.zeros((4, 8), np.float64))
    for call in (lambda: pt.traceHits(np.zeros((4, 8), np.float32)), pt.traceCameraHits, pt.gbuffer):
        with pytest.raises(hippt.HipptError, match="not initialized"):
            call()
    with pytest.raises(hippt.HipptError, match="outside"):
        pt.pickHit(0, 0)  # no image yet
    with pytest.raises(hippt.HipptError, match="no scene"):
        hippt.PathTracer().gbuffer()
