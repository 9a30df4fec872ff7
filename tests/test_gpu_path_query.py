"""Path queries (GPU): hipptTraceRadiance and hipptCameraRays against the oracle, bit for bit.

The reference is tests/path_ref.py: po_mesh_sample's loop per ray over test_gpu_ray_query.Ref.closest and
the oracle's po_scatter (pinned to MeshScene.sample by tests/test_path_ref_cpu.py, which also asserts on
the reference alone that the fixed ray sets reach every kind of path end).  Every comparison is exact: all
four radiance words and the segment count of every ray.  A scene's rays, seeds and reference are computed
once and shared by its tests."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import chain_audit
import hippt
import path_ref as pr
import pyoracle as po
from refit_util import verts_of, with_verts, wobble
from test_gpu_ray_query import N, Ref, case, degenerate_rays, pt, upload  # noqa: F401 (pt: the fixture)

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


# ---- 1. parity with the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed", "blob64x34", "random_scene"])
def test_radiance_and_segments_match_oracle(pt, name, lds, width):
    sc, rays, seeds, rad, segs, _, _ = pr.path_case(name)
    upload(pt, sc, lds, width)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name} lds={lds} width={width}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_limits_match_oracle(pt, depth):
    sc, rays, seeds, rad, segs, _, _ = pr.path_case("cornell34", depth)
    assert segs.max() == depth
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, depth)
    pr.assert_paths(got, gs, rad, segs, f"maxDepth {depth}")


def test_default_seeds_zero_rays_and_no_segments(pt):
    sc, rays, seeds, rad, segs, _, _ = pr.path_case("cornell34")
    assert pr.SEED_FRAME == 0  # seeds=None is path_seeds(N, 0)
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays)
    pr.assert_paths(got, gs, rad, segs, "default seeds")
    got, gs = pt.traceRadiance(rays, seeds.view(np.int32))
    pr.assert_paths(got, gs, rad, segs, "int32 seeds")
    got, gs = pt.traceRadiance(np.zeros((0, 8), np.float32))
    assert got.shape == (0, 4) and gs.shape == (0,)
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    only = np.empty((65, 4), np.float32)
    r, s = np.ascontiguousarray(rays[:65]), np.ascontiguousarray(seeds[:65])
    assert lib.hipptTraceRadiance(r.ctypes.data, s.ctypes.data, 65, 8, 0, only.ctypes.data, None, ctypes.byref(e)), e.value
    assert only.tobytes() == rad[:65].tobytes()


# ---- 2. it is the renderer ------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_camera_rays_traced_are_the_renderers_sample(pt, name, lds):
    w, h = 45, 26
    sc = case(name)[0]
    if name == "cornell_mixed":
        sc = dataclasses.replace(sc, aperture=12.0, focus=900.0)  # a thin lens
    upload(pt, sc, lds, w=w, h=h)
    rays, seeds = pt.cameraRays(0)
    want_rays, want_seeds = pr.camera_rays_seeds(sc, w, h, 0)
    assert rays.dtype == np.float32 and rays.shape == (h * w, 8) and seeds.dtype == np.uint32 and seeds.shape == (h * w,)
    assert rays.tobytes() == want_rays.tobytes() and np.array_equal(seeds, want_seeds)
    # frame 0 alone: by po_accumulate its average is the sample itself
    assert pt.resetAccumulation(), pt.lastError()
    assert pt.renderFrames(1, 8), pt.lastError()
    _, acc = pt.readback()
    rad, segs = pt.traceRadiance(rays, seeds, 8)
    assert np.ascontiguousarray(rad[:, :3]).tobytes() == np.ascontiguousarray(acc.reshape(-1, 4)[:, :3]).tobytes()
    # frame 7 against the oracle's sample, per pixel
    ora = po.MeshScene(sc, w, h)
    rays7, seeds7 = pt.cameraRays(7)
    rad7, segs7 = pt.traceRadiance(rays7, seeds7, 8)
    hits = 0
    for y in range(h):
        for x in range(w):
            rgb, n = ora.sample(x, y, 7, 8)
            assert rad7[y * w + x, :3].tobytes() == rgb.tobytes() and segs7[y * w + x] == n, (x, y)
            hits += int(rad7[y * w + x, 3] == 1.0)
    assert 0 < hits < w * h  # both the box and the sky are in the image
    # either output alone
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    r1, s1 = np.empty((h * w, 8), np.float32), np.empty(h * w, np.uint32)
    assert lib.hipptCameraRays(7, 0, r1.ctypes.data, None, ctypes.byref(e)), e.value
    assert lib.hipptCameraRays(7, 0, None, s1.ctypes.data, ctypes.byref(e)), e.value
    assert r1.tobytes() == rays7.tobytes() and np.array_equal(s1, seeds7)


# ---- 3. tmin and tmax belong to segment 0 only -------------------------------------------------------
@pytest.mark.parametrize("name,lds", [("cornell_mixed", 1), ("blob64x34", 0)])
def test_tmin_and_tmax_hold_for_the_first_segment_only(pt, name, lds):
    sc, rays, rt, rp = case(name)
    seeds = hippt.path_seeds(len(rays))
    upload(pt, sc, lds)
    hit = np.flatnonzero(rp >= 0)[:512]
    ref = pr.PathRef(sc, Ref(sc))
    # tmax before the first hit: the sky of the ray's own direction, a = 0, one segment
    short = rays[hit].copy()
    short[:, 7] = rt[hit] * np.float32(0.5)
    keep = short[:, 7] > short[:, 3]  # (still a valid interval)
    short, ss = np.ascontiguousarray(short[keep]), np.ascontiguousarray(seeds[hit][keep])
    assert len(short) > 256
    want, wsegs, ends, _ = ref.paths(short, ss, 8)
    assert np.all(wsegs == 1) and np.all(ends == pr.MISS) and not want[:, 3].any()
    for i in (0, len(short) - 1):
        assert tuple(want[i, :3]) == pr.sky(tuple(short[i, 4:7]), (1.0, 1.0, 1.0))
    got, gs = pt.traceRadiance(short, ss, 8)
    pr.assert_paths(got, gs, want, wsegs, "tmax before the first hit")
    # tmin past the first surface: the path starts from the second one; later segments use 0.001 and inf
    past = rays[hit].copy()
    past[:, 3] = np.nextafter(rt[hit], INF)
    sp = np.ascontiguousarray(seeds[hit])
    want, wsegs, _, _ = ref.paths(past, sp, 8)
    base, bsegs, _, _ = ref.paths(np.ascontiguousarray(rays[hit]), sp, 8)
    # conditions on the reference alone: most paths change, and at least a wave's worth (64) start from a
    # second surface and go on from there (rays from outside a convex-ish mesh mostly leave it instead)
    assert np.count_nonzero((want != base).any(axis=1)) > len(hit) // 2
    assert np.count_nonzero((want[:, 3] == 1.0) & (wsegs >= 2)) >= 64
    got, gs = pt.traceRadiance(past, sp, 8)
    pr.assert_paths(got, gs, want, wsegs, "tmin past the first surface")


# ---- 4. device memory --------------------------------------------------------------------------------
def test_device_memory_paths(pt):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs, _, _ = pr.path_case("cornell_mixed")
    pt.setDevices([0])
    upload(pt, sc)
    hr, hs = pt.traceRadiance(rays, seeds, 8)
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(np.array(rays)).to(dev)
    ds = torch.from_numpy(np.array(seeds).view(np.int32)).to(dev)
    r, s = pt.traceRadiance(dr, ds, 8)
    assert r.device == dr.device and s.device == dr.device and r.dtype == torch.float32 and s.dtype == torch.int32
    assert r.shape == (N, 4) and s.shape == (N,)
    assert r.cpu().numpy().tobytes() == hr.tobytes() == rad.tobytes()
    assert s.cpu().numpy().tobytes() == hs.tobytes() == segs.tobytes()
    r2, s2 = pt.traceRadiance(dr)  # default seeds, made on the rays' device
    assert r2.cpu().numpy().tobytes() == rad.tobytes() and s2.device == dr.device
    like = hippt.path_seeds(N, 0, like=dr)
    assert like.device == dr.device and np.array_equal(like.cpu().numpy().view(np.uint32), seeds)
    # the camera's rays on the device
    cr, cs = pt.cameraRays(3, device=True)
    hcr, hcs = pt.cameraRays(3)
    assert cr.device == dr.device and cs.device == dr.device
    assert cr.cpu().numpy().tobytes() == hcr.tobytes() and cs.cpu().numpy().view(np.uint32).tobytes() == hcs.tobytes()
    a, b = pt.traceRadiance(cr, cs, 8)
    c, d = pt.traceRadiance(hcr, hcs, 8)
    assert a.cpu().numpy().tobytes() == c.tobytes() and b.cpu().numpy().tobytes() == d.tobytes()
    # pointers that are not memory of a context's device, or misaligned
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    out, so = torch.empty((N + 1, 4), dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    host_out = np.empty((N, 4), np.float32)
    D = hippt.RAYS_DEVICE
    assert not lib.hipptTraceRadiance(rays.ctypes.data, ds.data_ptr(), N, 8, D, out.data_ptr(), so.data_ptr(), ctypes.byref(e))
    assert b"needs device memory pointers" in e.value
    assert not lib.hipptTraceRadiance(dr.data_ptr(), seeds.ctypes.data, N, 8, D, out.data_ptr(), so.data_ptr(), ctypes.byref(e))
    assert b"needs device memory pointers" in e.value
    assert not lib.hipptTraceRadiance(dr.data_ptr(), ds.data_ptr(), N, 8, D, host_out.ctypes.data, None, ctypes.byref(e))
    assert b"needs device memory pointers" in e.value
    assert not lib.hipptTraceRadiance(dr.data_ptr(), ds.data_ptr(), N, 8, D, out.data_ptr() + 4, so.data_ptr(), ctypes.byref(e))
    assert b"misaligned device pointer" in e.value
    assert not lib.hipptTraceRadiance(dr.data_ptr() + 8, ds.data_ptr(), N - 1, 8, D, out.data_ptr(), so.data_ptr(), ctypes.byref(e))
    assert b"misaligned device pointer" in e.value
    assert not lib.hipptTraceRadiance(dr.data_ptr(), ds.data_ptr() + 2, N - 1, 8, D, out.data_ptr(), so.data_ptr(), ctypes.byref(e))
    assert b"misaligned device pointer" in e.value
    assert not lib.hipptCameraRays(0, D, hcr.ctypes.data, None, ctypes.byref(e)) and b"needs device memory pointers" in e.value
    assert not lib.hipptCameraRays(0, D, cr.data_ptr() + 4, None, ctypes.byref(e)) and b"misaligned device pointer" in e.value
    with pytest.raises(hippt.HipptError, match="where the rays are"):
        pt.traceRadiance(dr, seeds)
    del dr, ds, r, s, r2, s2, like, cr, cs, a, b, out, so


# ---- 5. slicing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rays_per_slice", [64, 1024])
def test_slices_give_the_same_bytes(pt, rays_per_slice):
    sc, rays, seeds, rad, segs, _, _ = pr.path_case("cornell_mixed")
    upload(pt, sc)
    d_rad, d_segs = pt.traceRadiance(rays, seeds, 8)
    pt.setOption(hippt.OPT_QUERY_SLICE, rays_per_slice)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    assert got.tobytes() == d_rad.tobytes() == rad.tobytes() and gs.tobytes() == d_segs.tobytes() == segs.tobytes()


# ---- 6. path queries do not disturb rendering ------------------------------------------------------
def test_path_query_between_async_frames_leaves_the_image_alone(pt):
    w, h = 45, 26
    sc, rays, seeds, rad, segs, _, _ = pr.path_case("cornell34")
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    hippt.chain_audit()  # (drops records of earlier tests)
    upload(pt, sc, w=w, h=h)
    pt.resetStats()
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    got, gs = pt.traceRadiance(rays, seeds, 8)
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    px, acc = pt.readback()
    runs = hippt.chain_audit()
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 0)
    pr.assert_paths(got, gs, rad, segs)
    opx, oacc, osegs, _ = po.MeshScene(sc, w, h).frames(0, 6, 8)
    assert np.array_equal(px, opx) and acc.tobytes() == oacc.tobytes()
    problems = chain_audit.check(runs)
    assert not problems, problems[:6]
    assert pt.stats()["segments"] == osegs  # the query's segments are not the renderer's


# ---- 7. animated mesh ----------------------------------------------------------------------------------
def test_radiance_follows_a_vertex_update(pt):
    sc, rays, seeds, rad0, segs0, _, _ = pr.path_case("cornell34")
    n = N - degenerate_rays().shape[0]
    rays, seeds = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n])
    upload(pt, sc)
    v1 = wobble(verts_of(sc))
    pt.updateVertices(v1)
    sc1 = with_verts(sc, v1)
    rad, segs = pr.path_ref(sc1, rays, seeds, 8)
    # a condition on the reference alone: the update changes what most paths return
    assert np.count_nonzero((rad != rad0[:n]).any(axis=1)) > n // 2
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, "after updateVertices")
