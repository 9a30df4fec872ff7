"""Batched ray queries (GPU): hipptTraceRays, hipptOccluded and hipptTraceCamera against the oracle,
bit for bit.

The reference is the contract restated per ray with the oracle's own functions: po_closest_hit over
the triangles and po_sphere_t over the spheres (r^2 formed in float32), the minimum of (t, primitive
id), then t < tmax.  Every comparison is exact: the t buffers' bytes, the ids, and
occluded == (prim >= 0).  A scene's rays and reference are computed once and shared by its tests."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import chain_audit
import hippt
import pyoracle as po
from hippt import scenes
from test_gpu_fuzz import fuzz_scene

pytestmark = pytest.mark.gpu

N = 4097
INF = np.float32(np.inf)
PF = ctypes.POINTER(ctypes.c_float)


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    opts = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
            (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0))
    for k, v in opts:
        t.setOption(k, v)
    yield t
    for k, v in opts:
        t.setOption(k, v)
    hippt.load_library().cudaPathTracerShutdown()


# ---- the reference -----------------------------------------------------------------------------------
class Ref:
    """A scene's PoTri array and spheres, built once."""

    def __init__(self, sc):
        v = np.ascontiguousarray(sc.verts, np.float32).reshape(-1, 9)
        self.ntris = int(v.shape[0])
        self.tris = (po.PoTri * max(1, self.ntris))()
        L = po.lib()
        for i in range(self.ntris):
            L.po_tri_setup(v[i].ctypes.data_as(PF), ctypes.byref(self.tris[i]))
        sp = np.ascontiguousarray(sc.spheres, np.float32).reshape(-1, 4)
        self.centres = np.ascontiguousarray(sp[:, :3])
        self.r2 = (sp[:, 3] * sp[:, 3]).astype(np.float32)  # float32 product

    def closest(self, rays):
        """(t float32 (n,), prim int32 (n,)): min (t, id) over hits with t >= tmin, then t < tmax."""
        L = po.lib()
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        o = np.ascontiguousarray(rays[:, 0:3])
        d = np.ascontiguousarray(rays[:, 4:7])
        t_out = np.full(n, INF, np.float32)
        p_out = np.full(n, -1, np.int32)
        tt = ctypes.c_float()
        ob, db, cb = o.ctypes.data, d.ctypes.data, self.centres.ctypes.data
        for i in range(n):
            op, dp = ctypes.cast(ob + 12 * i, PF), ctypes.cast(db + 12 * i, PF)
            tmin, tmax = float(rays[i, 3]), rays[i, 7]
            best_t, best_p = INF, -1
            if self.ntris:
                k = L.po_closest_hit(self.tris, None, self.ntris, op, dp, tmin, ctypes.byref(tt))
                if k >= 0:
                    best_t, best_p = np.float32(tt.value), k
            for s in range(self.r2.shape[0]):
                if L.po_sphere_t(ctypes.cast(cb + 12 * s, PF), float(self.r2[s]), op, dp, tmin, ctypes.byref(tt)):
                    ts = np.float32(tt.value)
                    # ids of spheres follow the triangles', so an equal t keeps the earlier primitive
                    if best_p < 0 or ts < best_t:
                        best_t, best_p = ts, self.ntris + s
            if best_p >= 0 and best_t < tmax:
                t_out[i], p_out[i] = best_t, best_p
        return t_out, p_out


def scene_box(sc):
    pts = [np.asarray(sc.verts, np.float64).reshape(-1, 3)]
    sp = np.asarray(sc.spheres, np.float64).reshape(-1, 4)
    if sp.shape[0]:
        pts += [sp[:, :3] - sp[:, 3:4], sp[:, :3] + sp[:, 3:4]]
    p = np.concatenate(pts)
    return p.min(axis=0), p.max(axis=0)


def degenerate_rays():
    """Rays the queries report as a miss without traversing them: each a ray from inside the Cornell
    box with one field spoilt.  The oracle's arithmetic yields a miss for them too, except for
    tmin < 0 (entry NEGATIVE_TMIN), where it accepts hits from t = tmin on: there the miss is the
    query contract's (include/hippt.h), not the oracle's."""
    nan, inf = np.nan, np.inf
    base = np.array([278.0, 278.0, 278.0, 0.001, 0.3, -0.5, 0.8, inf], np.float32)
    out = []
    for k, v in ((0, nan), (1, inf), (2, -inf), (4, nan), (5, inf), (6, -inf), (3, nan), (3, inf), (7, nan), (7, -inf)):
        r = base.copy()
        r[k] = v
        out.append(r)
    zero = base.copy()
    zero[4:7] = 0.0
    neg = base.copy()
    neg[3] = -0.5
    eq = base.copy()
    eq[3] = eq[7] = 5.0
    below = base.copy()
    below[3], below[7] = 5.0, 1.0
    return np.stack(out + [zero, neg, eq, below])


NEGATIVE_TMIN = 11  # its index in degenerate_rays()


def make_rays(sc, n=N, seed=11):
    """Four quarters: from lookfrom into the box; in-box origins with directions of any length; in-box
    origins aimed at mesh vertices (sphere centres without triangles): shared edges and corners; origins
    on primitives' surfaces with random directions (t ~ 0 is rejected by tmin).  The last quarter ends
    with the degenerate rays."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    q = [n - 3 * (n // 4), n // 4, n // 4, n // 4]
    verts = np.asarray(sc.verts, np.float64).reshape(-1, 3)
    sp = np.asarray(sc.spheres, np.float64).reshape(-1, 4)
    rays = np.zeros((n, 8), np.float64)
    rays[:, 3] = 0.001
    rays[:, 7] = np.inf
    a = 0
    eye = np.asarray(sc.lookfrom, np.float64)
    rays[a:a + q[0], 0:3] = eye
    rays[a:a + q[0], 4:7] = rng.uniform(lo, hi, size=(q[0], 3)) - eye
    a += q[0]
    rays[a:a + q[1], 0:3] = rng.uniform(lo, hi, size=(q[1], 3))
    rays[a:a + q[1], 4:7] = rng.normal(size=(q[1], 3)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(q[1], 1))
    a += q[1]
    org = rng.uniform(lo, hi, size=(q[2], 3))
    aim = verts[rng.integers(0, verts.shape[0], size=q[2])] if verts.shape[0] else \
        sp[rng.integers(0, sp.shape[0], size=q[2]), :3]
    rays[a:a + q[2], 0:3] = org
    rays[a:a + q[2], 4:7] = aim - org
    a += q[2]
    if verts.shape[0]:
        tri = verts.reshape(-1, 3, 3)[rng.integers(0, verts.shape[0] // 3, size=q[3])]
        b = rng.dirichlet((1.0, 1.0, 1.0), size=q[3])
        surf = (tri * b[:, :, None]).sum(axis=1)
    else:
        s = sp[rng.integers(0, sp.shape[0], size=q[3])]
        u = rng.normal(size=(q[3], 3))
        surf = s[:, :3] + s[:, 3:4] * u / np.linalg.norm(u, axis=1, keepdims=True)
    rays[a:a + q[3], 0:3] = surf
    rays[a:a + q[3], 4:7] = rng.normal(size=(q[3], 3))
    rays = rays.astype(np.float32)
    deg = degenerate_rays()
    if n >= 4 * deg.shape[0]:
        rays[n - deg.shape[0]:] = deg
    return np.ascontiguousarray(rays)


SCENES = {
    "cornell34": scenes.cornell34,
    "cornell_mixed": scenes.cornell_mixed,
    "blob64x34": lambda: scenes.blob_scene(64, 34),
    "random_scene": scenes.random_scene,
}
RAYS = {"cornell34": N, "cornell_mixed": N, "blob64x34": N, "random_scene": 257}


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, rays, reference t, reference prim) of a named scene; computed once, never modified."""
    sc = SCENES[name]()
    rays = make_rays(sc, RAYS[name])
    t, p = Ref(sc).closest(rays)
    if rays.shape[0] == N:  # the degenerate rays: a miss by the query contract
        first = N - degenerate_rays().shape[0]
        oracle_tail = p[first:].copy()
        oracle_tail[NEGATIVE_TMIN] = -1
        assert np.all(oracle_tail == -1), "the oracle hits a degenerate ray"
        t[first:], p[first:] = INF, -1
    for a in (rays, t, p):
        a.setflags(write=False)
    return sc, rays, t, p


def upload(pt, sc, lds=1, width=0, w=64, h=48):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    pt.uploadMesh(sc)
    assert pt.initialize(w, h), pt.lastError()


def assert_same(t, prim, rt, rp, what=""):
    t, prim = np.asarray(t), np.asarray(prim)
    assert t.dtype == np.float32 and prim.dtype == np.int32
    bad = np.flatnonzero((t.view(np.uint32) != rt.view(np.uint32)) | (prim != rp))
    assert bad.size == 0, f"{what}: {bad.size} of {rt.size} rays differ, first {bad[:5]}: " \
                          f"t {t[bad[:5]]} vs {rt[bad[:5]]}, prim {prim[bad[:5]]} vs {rp[bad[:5]]}"
    assert t.tobytes() == rt.tobytes()


# ---- 1. parity with the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_reference_is_neither_all_hits_nor_all_misses(name):
    """The condition on the ray set, asserted on the oracle alone: at least 50 % hits and 2 % misses."""
    _, rays, _, rp = case(name)
    share = np.count_nonzero(rp >= 0) / rp.size
    print(f"{name}: oracle hit share {share:.3f}, primitives hit {np.unique(rp[rp >= 0]).size}")
    assert 0.5 <= share <= 0.98


@pytest.mark.parametrize("width", [0, 2])
@pytest.mark.parametrize("name,lds", [("cornell34", 1), ("cornell_mixed", 1), ("blob64x34", 0), ("random_scene", 1)])
def test_closest_hit_and_occlusion_match_oracle(pt, name, lds, width):
    sc, rays, rt, rp = case(name)
    upload(pt, sc, lds, width)
    sizes = (1, 63, 65, N) if rays.shape[0] == N else (rays.shape[0],)
    for n in sizes:
        t, prim = pt.traceRays(np.ascontiguousarray(rays[:n]))
        assert_same(t, prim, rt[:n], rp[:n], f"{name} n={n}")
        occ = pt.occluded(np.ascontiguousarray(rays[:n]))
        assert occ.dtype == np.uint8 and np.array_equal(occ, (rp[:n] >= 0).astype(np.uint8)), f"{name} n={n}"


def test_zero_rays_and_single_outputs(pt):
    sc, rays, rt, rp = case("cornell34")
    upload(pt, sc)
    t, prim = pt.traceRays(np.zeros((0, 8), np.float32))
    assert t.shape == (0,) and prim.shape == (0,)
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    t = np.empty(65, np.float32)
    prim = np.empty(65, np.int32)
    r = np.ascontiguousarray(rays[:65])
    assert lib.hipptTraceRays(r.ctypes.data, 65, 0, t.ctypes.data, None, ctypes.byref(e)), e.value
    assert lib.hipptTraceRays(r.ctypes.data, 65, 0, None, prim.ctypes.data, ctypes.byref(e)), e.value
    assert_same(t, prim, rt[:65], rp[:65])


# ---- 2. tmax is strict -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lds", [("cornell_mixed", 1), ("blob64x34", 0)])
def test_tmax_is_exclusive(pt, name, lds):
    sc, rays, rt, rp = case(name)
    upload(pt, sc, lds)
    hit = np.flatnonzero(rp >= 0)[:1024]
    at = rays[hit].copy()
    at[:, 7] = rt[hit]  # tmax = t: that hit is out, and everything else is farther
    past = rays[hit].copy()
    past[:, 7] = np.nextafter(rt[hit], INF)  # the next float: the same hit
    ref = Ref(sc)
    for r, what in ((at, "tmax = t"), (past, "tmax = nextafter(t)")):
        et, ep = ref.closest(r)
        t, prim = pt.traceRays(r)
        assert_same(t, prim, et, ep, what)
        assert np.array_equal(pt.occluded(r), (ep >= 0).astype(np.uint8)), what
    assert np.all(ref.closest(at)[1] == -1) and np.array_equal(ref.closest(past)[1], rp[hit])


# ---- 3. tmin belongs to the ray ---------------------------------------------------------------------
@pytest.mark.parametrize("name,lds", [("cornell_mixed", 1), ("blob64x34", 0)])
def test_tmin_is_the_rays_own(pt, name, lds):
    sc, rays, rt, rp = case(name)
    upload(pt, sc, lds)
    hit = np.flatnonzero(rp >= 0)[:1024]
    o = rays[hit, 0:3].astype(np.float64)
    d = rays[hit, 4:7].astype(np.float64)
    p = o + rt[hit, None].astype(np.float64) * d
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    near = np.zeros((hit.size, 8), np.float32)
    near[:, 0:3] = p - 0.0005 * dn  # just in front of the surface point
    near[:, 4:7] = dn
    near[:, 7] = INF
    ref = Ref(sc)
    shares = []
    for tmin in (0.0, 0.001):
        near[:, 3] = tmin
        et, ep = ref.closest(near)
        t, prim = pt.traceRays(near)
        assert_same(t, prim, et, ep, f"tmin = {tmin}")
        assert np.array_equal(pt.occluded(near), (ep >= 0).astype(np.uint8))
        shares.append(np.count_nonzero(et < np.float32(0.001)) / et.size)
    # the near surface is what tmin = 0 reports and what tmin = 0.001 must not
    assert shares[0] > 0.5 and shares[1] == 0.0, shares


# ---- 4. ties -----------------------------------------------------------------------------------------
def test_coincident_triangles_report_the_lower_id(pt):
    sc, rays, rt, rp = case("cornell34")
    twice = dataclasses.replace(sc, name="cornell34x2", verts=np.concatenate([sc.verts, sc.verts]),
                                tri_mat=np.concatenate([sc.tri_mat, sc.tri_mat]))
    for lds in (1, 0):
        upload(pt, twice, lds)
        t, prim = pt.traceRays(rays)
        assert prim.max() < 34
        assert_same(t, prim, rt, rp, f"lds={lds}")


# ---- 5. edge geometry --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 5, 9])
def test_fuzz_scenes_match_oracle(pt, seed):
    sc = fuzz_scene(seed)
    rays = make_rays(sc, 1025)
    rt, rp = Ref(sc).closest(rays)
    for lds in (1, 0):
        pt.setOption(hippt.OPT_LDS_SCENE, lds)
        pt.uploadScene(sc)
        assert pt.initialize(48, 32), pt.lastError()
        t, prim = pt.traceRays(rays)
        assert_same(t, prim, rt, rp, f"fuzz{seed} lds={lds}")
        assert np.array_equal(pt.occluded(rays), (rp >= 0).astype(np.uint8))


# ---- 6. slicing --------------------------------------------------------------------------------------
def test_slices_give_the_same_bytes(pt):
    sc, rays, rt, rp = case("cornell_mixed")
    upload(pt, sc)
    pt.setOption(hippt.OPT_QUERY_SLICE, 1000)
    t, prim = pt.traceRays(rays)
    assert_same(t, prim, rt, rp, "slice 1000")
    assert np.array_equal(pt.occluded(rays), (rp >= 0).astype(np.uint8))


# ---- 7. camera buffers -------------------------------------------------------------------------------
def camera_rays(sc, w, h, frame):
    """The rays hipptRenderFrames starts sample `frame` with, row-major."""
    L = po.lib()
    cam = po.scene_camera(sc, w, h)
    inv_w = np.float32(1.0) / np.float32(max(w - 1, 1))
    inv_h = np.float32(1.0) / np.float32(max(h - 1, 1))
    rays = np.zeros((h * w, 8), np.float32)
    rays[:, 3] = 0.001
    rays[:, 7] = INF
    o, d = (ctypes.c_float * 3)(), (ctypes.c_float * 3)()
    for y in range(h):
        for x in range(w):
            seed = ctypes.c_uint32(L.po_pixel_seed(x, y, w, frame))
            s = (np.float32(x) + np.float32(L.po_rand01(ctypes.byref(seed)))) * inv_w
            t = (np.float32(y) + np.float32(L.po_rand01(ctypes.byref(seed)))) * inv_h
            L.po_camera_get_ray(ctypes.byref(cam), float(s), float(t), ctypes.byref(seed), o, d)
            rays[y * w + x, 0:3] = o[:]
            rays[y * w + x, 4:7] = d[:]
    return rays


@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_camera_buffers(pt, name):
    w, h = 45, 26
    sc = case(name)[0]
    if name == "cornell_mixed":
        sc = dataclasses.replace(sc, aperture=12.0, focus=900.0)  # a thin lens
    upload(pt, sc, w=w, h=h)
    ref = Ref(sc)
    ora = po.MeshScene(sc, w, h)
    for frame in (0, 7):
        rt, rp = ref.closest(camera_rays(sc, w, h, frame))
        t, prim = pt.traceCamera(frame)
        assert t.shape == (h, w) and prim.shape == (h, w)
        assert_same(t.reshape(-1), prim.reshape(-1), rt, rp, f"{name} frame {frame}")
        # independent of the reference above: a depth-1 sample is black exactly where the first ray hits
        for y in range(h):
            for x in range(w):
                rgb, _ = ora.sample(x, y, frame, 1)
                assert (prim[y, x] >= 0) == (not rgb.any()), (x, y, frame)
        for x, y in ((0, 0), (w - 1, h - 1), (w // 2, h // 2), (7, 19)):
            assert pt.pick(x, y, frame) == (int(prim[y, x]), float(t[y, x]))
    with pytest.raises(hippt.HipptError):
        pt.pick(w, 0)


# ---- 8. device memory --------------------------------------------------------------------------------
def test_device_memory_rays(pt):
    assert torch.cuda.is_available()
    sc, rays, rt, rp = case("cornell_mixed")
    pt.setDevices([0])
    upload(pt, sc)
    ht, hp = pt.traceRays(rays)
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(np.array(rays)).to(dev)
    t, prim = pt.traceRays(dr)
    occ = pt.occluded(dr)
    assert t.device == dr.device and prim.device == dr.device and occ.device == dr.device
    assert t.dtype == torch.float32 and prim.dtype == torch.int32 and occ.dtype == torch.uint8
    assert t.cpu().numpy().tobytes() == ht.tobytes() == rt.tobytes()
    assert np.array_equal(prim.cpu().numpy(), hp) and np.array_equal(hp, rp)
    assert np.array_equal(occ.cpu().numpy(), (rp >= 0).astype(np.uint8))
    # pointers that are not memory of a context's device
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    t0, p0 = np.empty(N, np.float32), np.empty(N, np.int32)
    assert not lib.hipptTraceRays(rays.ctypes.data, N, hippt.RAYS_DEVICE, t0.ctypes.data, p0.ctypes.data, ctypes.byref(e))
    assert e.value
    if torch.cuda.device_count() > 1:
        with pytest.raises(hippt.HipptError, match="device"):
            pt.traceRays(torch.from_numpy(np.array(rays)).to(torch.device("cuda", 1)))
    del dr, t, prim, occ


# ---- 9. queries do not disturb rendering ------------------------------------------------------------
def test_query_between_async_frames_leaves_the_image_alone(pt):
    w, h = 45, 26
    sc, rays, rt, rp = case("cornell34")
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    hippt.chain_audit()  # (drops records of earlier tests)
    upload(pt, sc, w=w, h=h)
    pt.resetStats()
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    t, prim = pt.traceRays(rays)
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    px, acc = pt.readback()
    runs = hippt.chain_audit()
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 0)
    assert_same(t, prim, rt, rp)
    opx, oacc, segs, _ = po.MeshScene(sc, w, h).frames(0, 6, 8)
    assert np.array_equal(px, opx) and acc.tobytes() == oacc.tobytes()
    problems = chain_audit.check(runs)
    assert not problems, problems[:6]
    assert pt.stats()["segments"] == segs  # queries add nothing
