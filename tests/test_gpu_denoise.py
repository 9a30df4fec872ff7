"""The denoiser (GPU): hipptDenoise against the numpy float32 model of its contract (tests/denoise_ref.py),
bit for bit: the rgba floats and the pixel words, for every pass count, both pixel formats, images smaller
than the tap reach and larger than a tile, trees in LDS and in global memory.

The model runs on the accumulation readback() returns and on guide records built from the oracle-pinned
references of the ray-query tests; a case's guides are computed once and shared."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import chain_audit
import denoise_ref as dr
import hippt
import pyoracle as po
from hippt import scenes
from refit_util import verts_of, with_verts, wobble

pytestmark = pytest.mark.gpu


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    opts = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
            (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB),
            (hippt.OPT_DENOISE_TIMING, 0))
    for k, v in opts:
        t.setOption(k, v)
    yield t
    for k, v in opts:
        t.setOption(k, v)
    t.setDevices([])
    t.setRowRange(0, 0)
    hippt.load_library().cudaPathTracerShutdown()


def scene(name):
    if name == "cornell_mixed_lens":
        return dataclasses.replace(scenes.cornell_mixed(), aperture=12.0, focus=900.0)  # a thin lens
    if name == "blob64x34":
        return scenes.blob_scene(64, 34)
    return scenes.get_scene(name)


@functools.lru_cache(maxsize=None)
def guides(name, w, h, frame):
    g = dr.guides(scene(name), w, h, frame)
    g.setflags(write=False)
    return g


def start(pt, sc, w, h, frames=4, lds=1):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.uploadMesh(sc)
    assert pt.initialize(w, h), pt.lastError()
    assert pt.renderFrames(frames, 8), pt.lastError()


def assert_same(got, want, what):
    px, rgba = got
    wpx, wrgba = want
    assert px.dtype == np.uint32 and rgba.dtype == np.float32 and px.shape == wpx.shape and rgba.shape == wrgba.shape
    bad = np.argwhere((rgba.view(np.uint32) != wrgba.view(np.uint32)).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} of {wpx.size} pixels differ, first (y, x) {bad[:4].tolist()}: " \
                          f"{rgba[tuple(bad[0])]} vs {wrgba[tuple(bad[0])]}"
    assert np.array_equal(px, wpx), f"{what}: {np.count_nonzero(px != wpx)} words differ"


# ---- 1. parity with the model -----------------------------------------------------------------------
CASES = [("cornell34", 45, 26), ("cornell34", 64, 48), ("cornell34", 130, 70), ("cornell34", 7, 5),
         ("cornell_mixed", 45, 26), ("cornell_mixed", 64, 48), ("cornell_mixed", 130, 70), ("cornell_mixed", 7, 5),
         ("cornell_mixed_lens", 64, 48)]


@pytest.mark.parametrize("name,w,h", CASES)
def test_denoise_matches_the_model(pt, name, w, h):
    sc = scene(name)
    start(pt, sc, w, h)
    rpx, acc = pt.readback()
    mats = sc.materials()
    g0 = guides(name, w, h, 0)
    assert_same(pt.denoise(), dr.denoise(acc, g0, mats), f"{name} {w}x{h} defaults")
    for passes in (0, 1, 3, 8):
        assert_same(pt.denoise(passes=passes), dr.denoise(acc, g0, mats, passes=passes), f"{name} {w}x{h} passes={passes}")
    assert_same(pt.denoise(guide_frame=3), dr.denoise(acc, guides(name, w, h, 3), mats), f"{name} {w}x{h} guide 3")
    px2, acc2 = pt.readback()  # the image is as it was
    assert np.array_equal(px2, rpx) and acc2.tobytes() == acc.tobytes()


def test_other_parameters_and_rgba8_words(pt):
    name, w, h = "cornell_mixed", 64, 48
    sc = scene(name)
    pt.setOption(hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_RGBA8)
    start(pt, sc, w, h)
    _, acc = pt.readback()
    mats, g0 = sc.materials(), guides(name, w, h, 0)
    assert_same(pt.denoise(), dr.denoise(acc, g0, mats, fmt=dr.PIXEL_RGBA8), "rgba8 defaults")
    kw = dict(passes=4, sigma_color=0.37, sigma_depth=0.011, normal_power=2)
    assert_same(pt.denoise(**kw), dr.denoise(acc, g0, mats, fmt=dr.PIXEL_RGBA8, **kw), "rgba8 other parameters")
    kw = dict(passes=2, normal_power=0, demodulate=False)
    assert_same(pt.denoise(**kw), dr.denoise(acc, g0, mats, fmt=dr.PIXEL_RGBA8, **kw), "rgba8 no demodulation")
    kw = dict(passes=2, normal_power=10, sigma_color=3.0)
    assert_same(pt.denoise(**kw), dr.denoise(acc, g0, mats, fmt=dr.PIXEL_RGBA8, **kw), "rgba8 power 10")


def test_tree_in_global_memory(pt):
    name, w, h = "blob64x34", 64, 48
    sc = scene(name)
    start(pt, sc, w, h, lds=0)
    _, acc = pt.readback()
    assert_same(pt.denoise(), dr.denoise(acc, guides(name, w, h, 0), sc.materials()), "blob64x34, LDS scene copy off")


# ---- 2. no passes, no demodulation: the image itself -------------------------------------------------
@pytest.mark.parametrize("fmt", [hippt.PIXEL_ARGB, hippt.PIXEL_RGBA8])
def test_no_passes_without_demodulation_gives_the_rendered_words(pt, fmt):
    pt.setOption(hippt.OPT_PIXEL_FORMAT, fmt)
    start(pt, scene("cornell_mixed"), 45, 26)
    rpx, acc = pt.readback()
    px, rgba = pt.denoise(passes=0, demodulate=False)
    assert px.tobytes() == rpx.tobytes()
    assert rgba[..., :3].tobytes() == np.ascontiguousarray(acc[..., :3]).tobytes() and np.all(rgba[..., 3] == 1.0)


# ---- 3. the renderer does not notice -----------------------------------------------------------------
def test_denoise_between_async_frames_leaves_the_image_alone(pt):
    name, w, h = "cornell34", 45, 26
    sc = scene(name)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    hippt.chain_audit()  # (drops records of earlier tests)
    pt.uploadMesh(sc)
    assert pt.initialize(w, h), pt.lastError()
    pt.resetStats()
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    got = pt.denoise()
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    px, acc = pt.readback()
    runs = hippt.chain_audit()
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 0)
    ora = po.MeshScene(sc, w, h)
    _, acc3, _, _ = ora.frames(0, 3, 8)
    assert_same(got, dr.denoise(acc3, guides(name, w, h, 0), sc.materials()), "after three async frames")
    opx, oacc, segs, _ = ora.frames(0, 6, 8)
    assert np.array_equal(px, opx) and acc.tobytes() == oacc.tobytes()
    problems = chain_audit.check(runs)
    assert not problems, problems[:6]
    assert pt.stats()["segments"] == segs  # the guide query adds nothing


# ---- 4. the guides follow the scene and the camera ---------------------------------------------------
def test_denoise_follows_a_vertex_update(pt):
    w, h = 64, 48
    sc = scene("cornell34")
    start(pt, sc, w, h)
    v1 = wobble(verts_of(sc))
    pt.updateVertices(v1)
    sc1 = with_verts(sc, v1)
    _, acc = pt.readback()
    g0, g1 = guides("cornell34", w, h, 0), dr.guides(sc1, w, h, 0)
    # a condition on the references alone: the update changes most pixels' guides
    assert np.count_nonzero((g1["normal"] != g0["normal"]).any(axis=-1)) > w * h // 2
    assert_same(pt.denoise(), dr.denoise(acc, g1, sc.materials()), "after updateVertices")


def test_denoise_follows_the_camera(pt):
    w, h = 64, 48
    sc = scene("cornell34")
    start(pt, sc, w, h)
    moved = dataclasses.replace(sc, lookat=(278.0 + 150.0, 278.0 - 60.0, 0.0))
    cam = hippt.build_camera(moved.lookfrom, moved.lookat, moved.vup, moved.vfov, w / h, moved.aperture, moved.focus)
    err = ctypes.c_char_p()
    assert hippt.load_library().hipptSetCamera(ctypes.byref(cam), ctypes.byref(err)), err.value
    _, acc = pt.readback()
    g0, g1 = guides("cornell34", w, h, 0), dr.guides(moved, w, h, 0)
    assert np.count_nonzero(g1["prim"] != g0["prim"]) > w * h // 8  # (on the references alone)
    assert_same(pt.denoise(), dr.denoise(acc, g1, sc.materials()), "after hipptSetCamera")


# ---- 5. device outputs -------------------------------------------------------------------------------
def test_device_outputs_and_placement_errors(pt):
    assert torch.cuda.is_available()
    name, w, h = "cornell_mixed", 64, 48
    sc = scene(name)
    pt.setDevices([0])
    start(pt, sc, w, h)
    hpx, hrgba = pt.denoise()
    dpx, drgba = pt.denoise(tensors=True)
    dev = torch.device("cuda", 0)
    assert dpx.device == dev and drgba.device == dev and drgba.dtype == torch.float32
    assert tuple(dpx.shape) == (h, w) and tuple(drgba.shape) == (h, w, 4)
    assert drgba.cpu().numpy().tobytes() == hrgba.tobytes()
    assert dpx.cpu().numpy().tobytes() == hpx.tobytes()
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    p = hippt.DenoiseParams()
    lib.hipptDenoiseDefaults(ctypes.byref(p))
    p.flags = hippt.DENOISE_DEVICE
    buf = torch.empty(4 * w * h + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    assert not lib.hipptDenoise(ctypes.byref(p), None, buf.data_ptr() + 4, ctypes.byref(e))
    assert b"misaligned" in e.value
    host = np.empty((h, w, 4), np.float32)
    assert not lib.hipptDenoise(ctypes.byref(p), None, host.ctypes.data, ctypes.byref(e))
    assert b"device memory" in e.value
    assert lib.hipptDenoise(ctypes.byref(p), None, buf.data_ptr(), ctypes.byref(e)), e.value  # rgba alone
    assert buf[:4 * w * h].cpu().numpy().tobytes() == hrgba.tobytes()
    del buf, dpx, drgba
    # one context must hold every row
    pt.setRowRange(0, h // 2)
    assert pt.initialize(w, h), pt.lastError()
    with pytest.raises(hippt.HipptError, match="row range"):
        pt.denoise()
    pt.setRowRange(0, 0)
    pt.setRowInterleave(1, 2)
    assert pt.initialize(w, h), pt.lastError()
    with pytest.raises(hippt.HipptError, match="row interleave"):
        pt.denoise()
    pt.setRowRange(0, 0)
    if torch.cuda.device_count() > 1:
        pt.setDevices([0, 1])
        assert pt.initialize(w, h), pt.lastError()
        with pytest.raises(hippt.HipptError, match="more than one device"):
            pt.denoise()


# ---- 6. the measuring aid ----------------------------------------------------------------------------
def test_stage_timing_changes_nothing(pt):
    start(pt, scene("cornell34"), 64, 48)
    plain = pt.denoise(passes=3)
    pt.setOption(hippt.OPT_DENOISE_TIMING, 1)
    timed = pt.denoise(passes=3)
    times = pt.denoiseTimes()
    pt.setOption(hippt.OPT_DENOISE_TIMING, 0)
    assert timed[0].tobytes() == plain[0].tobytes() and timed[1].tobytes() == plain[1].tobytes()
    assert sorted(times) == sorted(["guides", "prepare", "pass0", "pass1", "pass2", "finish"])
    assert all(0.0 < ms < 1000.0 for ms in times.values()), times
