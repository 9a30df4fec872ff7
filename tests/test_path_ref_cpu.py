"""Path queries without a GPU: the per-ray reference of tests/path_ref.py is the oracle's sample, the
fixed ray sets of the GPU tests exercise what they are meant to (conditions on the reference alone), the C
ABI of hipptTraceRadiance and hipptCameraRays rejects every argument error before any device call, and
hippt.path_seeds is the renderer's pixel_seed."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import hippt
import path_ref as pr
import pyoracle as po
from hippt import scenes
from test_gpu_ray_query import RAYS, Ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12


def model_scene(name):
    if name == "cornell34":
        return scenes.cornell34()
    sc = scenes.cornell_mixed()
    if name == "cornell_mixed_lens":
        sc = dataclasses.replace(sc, aperture=12.0, focus=900.0)  # the thin lens of test_camera_buffers
    return sc


# ---- the model is the oracle's sample --------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed", "cornell_mixed_lens"])
def test_path_ref_is_the_oracles_sample(name):
    sc = model_scene(name)
    ora = po.MeshScene(sc, W, H)
    ref = pr.PathRef(sc, Ref(sc))
    checked = 0
    for frame in (0, 5):
        rays, seeds = pr.camera_rays_seeds(sc, W, H, frame)
        for depth in (1, 2, 8):
            rad, segs, _, _ = ref.paths(rays, seeds, depth)
            for y in range(H):
                for x in range(W):
                    rgb, n = ora.sample(x, y, frame, depth)
                    i = y * W + x
                    assert rad[i, :3].tobytes() == rgb.tobytes() and segs[i] == n, (name, frame, depth, x, y)
                    checked += 1
            if depth == 1:  # a = 1 exactly where the camera ray hits: a depth-1 sample is black there
                assert np.array_equal(rad[:, 3] == 1.0, ~rad[:, :3].any(axis=1))
    assert checked == 2 * 3 * W * H


def test_camera_rays_with_seeds_are_the_query_tests_camera_rays():
    from test_gpu_ray_query import camera_rays
    sc = model_scene("cornell_mixed_lens")
    rays, seeds = pr.camera_rays_seeds(sc, W, H, 5)
    assert rays.tobytes() == camera_rays(sc, W, H, 5).tobytes()
    assert seeds.dtype == np.uint32 and np.unique(seeds).size > W * H // 2


# ---- the GPU tests' ray sets are not vacuous ---------------------------------------------------------
@pytest.mark.parametrize("name", list(RAYS))
def test_fixed_ray_sets_cover_every_outcome(name):
    sc, rays, seeds, rad, segs, ends, kinds = pr.path_case(name)
    ok = ends != pr.INVALID
    n = int(np.count_nonzero(ok))
    assert n >= len(rays) - 14 and np.all(segs[~ok] == 0) and not rad[~ok].any()
    primary_miss = np.count_nonzero(ok & (ends == pr.MISS) & (segs == 1))
    late_sky = np.count_nonzero((ends == pr.MISS) & (segs >= 3))
    black = np.count_nonzero((ends == pr.DEPTH) & (segs == pr.MAX_DEPTH))
    two = np.count_nonzero(segs >= 2)
    print(f"{name}: {n} valid, primary miss {primary_miss}, sky after >= 3 segments {late_sky}, depth limit {black}, "
          f">= 2 segments {two}, absorbed {np.count_nonzero(ends == pr.ABSORBED)}, "
          f"through metal {np.count_nonzero(kinds & 2)}, through dielectric {np.count_nonzero(kinds & 4)}")
    assert primary_miss >= 1 and late_sky >= 1 and black >= 1
    assert not rad[ends == pr.DEPTH, :3].any() and np.all(rad[ends == pr.DEPTH, 3] == 1.0)
    assert np.all(rad[ok & (segs == 1) & (ends == pr.MISS), 3] == 0.0)
    assert 4 * two >= n
    if name in ("cornell_mixed", "random_scene"):
        assert np.count_nonzero(kinds & (1 << scenes.MAT_METAL)) >= 1
        assert np.count_nonzero(kinds & (1 << scenes.MAT_DIELECTRIC)) >= 1


# ---- seeds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,frame", [(0, 0), (1, 0), (4097, 0), (4097, 5), (500000, 123456)])
def test_path_seeds_are_pixel_seeds(n, frame):
    s = hippt.path_seeds(n, frame)
    assert s.dtype == np.uint32 and s.shape == (n,)
    L = po.lib()
    for i in sorted({0, 1, n // 3, n - 2, n - 1} & set(range(n))):
        assert int(s[i]) == L.po_pixel_seed(i, 0, max(n, 1), frame), (i, n, frame)
    if n:
        want = (np.arange(n, dtype=np.uint64) * 9781 + (frame + 1) * 6271) & 0xFFFFFFFF
        assert np.array_equal(s, want.astype(np.uint32))
    assert np.array_equal(hippt.path_seeds(7), hippt.path_seeds(7, 0))


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_both_entry_points():
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    assert re.search(r"bool hipptTraceRadiance\(const float \*rays, const unsigned int \*seeds, long long numRays, "
                     r"int maxDepth,\s+int flags, float \*radiance, int \*segments, const char \*\*errorMessage\);", header)
    assert re.search(r"bool hipptCameraRays\(int frame, int flags, float \*rays, unsigned int \*seeds, "
                     r"const char \*\*errorMessage\);", header)
    assert "hipptTraceRadiance" in hippt.EXPORTS and "hipptCameraRays" in hippt.EXPORTS


def test_argument_errors_come_before_any_device_call():
    lib = hippt.load_library()
    lib.cudaPathTracerShutdown()
    pt = hippt.PathTracer()
    pt.uploadMesh(scenes.cornell34())  # a scene, no Init
    rays = np.zeros((4, 8), np.float32)
    seeds = np.zeros(4, np.uint32)
    rad = np.zeros((4, 4), np.float32)
    segs = np.zeros(4, np.int32)
    cam_rays = np.zeros((16, 8), np.float32)
    cam_seeds = np.zeros(16, np.uint32)
    none = object()

    def radiance(r=rays, s=seeds, n=4, depth=8, flags=0, out=rad, sg=segs):
        e = ctypes.c_char_p()
        ok = lib.hipptTraceRadiance(None if r is none else r.ctypes.data, None if s is none else s.ctypes.data, n, depth,
                                    flags, None if out is none else out.ctypes.data,
                                    None if sg is none else sg.ctypes.data, ctypes.byref(e))
        return ok, (e.value or b"").decode()

    def camera(frame=0, flags=0, r=cam_rays, s=cam_seeds):
        e = ctypes.c_char_p()
        ok = lib.hipptCameraRays(frame, flags, None if r is none else r.ctypes.data,
                                 None if s is none else s.ctypes.data, ctypes.byref(e))
        return ok, (e.value or b"").decode()

    bad = [({"depth": 0}, "maxDepth"), ({"depth": -3}, "maxDepth"), ({"r": none}, "null ray buffer"),
           ({"s": none}, "null seed buffer"), ({"out": none}, "no output buffer"), ({"n": -1}, "negative ray count"),
           ({"flags": 2}, "unknown flags"), ({"flags": 4 | hippt.RAYS_DEVICE}, "unknown flags"),
           ({"n": 0, "flags": 8}, "unknown flags"), ({"n": 0, "depth": 0}, "maxDepth")]
    cam_bad = [({"frame": -1}, "negative frame"), ({"flags": 2}, "unknown flags"), ({"r": none, "s": none}, "no output buffer")]
    for state in ("no Init", "built-in scene"):
        for fields, word in bad:
            ok, msg = radiance(**fields)
            assert not ok and word in msg and msg.startswith("path query:"), (state, fields, msg)
        for fields, word in cam_bad:
            ok, msg = camera(**fields)
            assert not ok and word in msg and msg.startswith("path query:"), (state, fields, msg)
        # everything valid: the state is what is wrong
        word = "not initialized" if state == "no Init" else "built-in scene"
        for ok, msg in (radiance(), radiance(sg=none), radiance(n=0, r=none, s=none, out=none), camera(), camera(r=none),
                        camera(s=none)):
            assert not ok and word in msg, (state, msg)
        assert not lib.hipptTraceRadiance(rays.ctypes.data, seeds.ctypes.data, 4, 8, 0, rad.ctypes.data, None, None)
        assert not lib.hipptCameraRays(0, 0, cam_rays.ctypes.data, None, None)  # a null message pointer is allowed
        if state == "no Init":
            with pytest.raises(hippt.HipptError, match="not initialized"):
                pt.traceRadiance(rays)
            pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    with pytest.raises(hippt.HipptError, match="built-in scene"):
        pt.traceRadiance(rays, seeds, 8)
    with pytest.raises(hippt.HipptError, match="built-in scene"):
        pt.cameraRays()
    assert not rad.any() and not segs.any() and not cam_rays.any()  # nothing was written
    lib.cudaPathTracerShutdown()


def test_python_argument_checks():
    pt = hippt.PathTracer()
    rays = np.zeros((4, 8), np.float32)
    for seeds, word in ((np.zeros(3, np.uint32), "shape"), (np.zeros(4, np.int64), "int32 or uint32"),
                        (np.zeros((4, 1), np.uint32), "shape"), ([0, 0, 0, 0], "numpy array")):
        with pytest.raises(hippt.HipptError, match=word):
            pt.traceRadiance(rays, seeds)
    with pytest.raises(hippt.HipptError, match="shape"):
        pt.traceRadiance(np.zeros((4, 7), np.float32))
