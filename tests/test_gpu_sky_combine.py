"""HIPPT_OPT_SKY_COMBINE (GPU; DESIGN.md §5 "Sky runs in the combine"): a batch with a sky rectangle and an item
table leaves the 64-pixel runs wholly outside the rectangle out of its queues, and its combine computes their
samples.  Every case compares pixels and accumulation bit for bit with the same library under the option at 0
and with the oracle, and asserts that the mode applied (HIPPT_INFO_SKY_COMBINE between 0 and the band's pixel
count, exclusive) and that hipptGetStats counts the same segments and pixel samples either way.  The camera
(tests/sky_combine_cam.py) leaves whole sky tiles on all four sides at 104x72 (tests/test_sky_combine_model.py).
3 spp, depth 3."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime

import chain_audit
import hippt
import pyoracle as po
import sky_combine_cam as scc
from hippt import scenes
from refit_util import verts_of, with_verts

pytestmark = pytest.mark.gpu

SPP, DEPTH = 3, 3
W, H = scc.WIDTH, scc.HEIGHT
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_BVH_QUANT, -1),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_ITEM_ORDER, -1), (hippt.OPT_COUNT_TRAVERSAL, 0),
        (hippt.OPT_CAMERA_POOL, -1), (hippt.OPT_PIXEL_TILE, -1), (hippt.OPT_SKY_RECT, 1), (hippt.OPT_SKY_COMBINE, -1),
        (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB))


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    for k, v in OPTS:
        t.setOption(k, v)
    yield t
    for k, v in OPTS:
        t.setOption(k, v)
    t.setDevices([])
    t.setRowRange(0, 0)
    hippt.load_library().cudaPathTracerShutdown()


@functools.lru_cache(maxsize=None)
def scene(name="cornell34", aperture=0.0):
    return scc.pulled_back(getattr(scenes, name), aperture=aperture)


@functools.lru_cache(maxsize=None)
def oracle(name, w, frames, aperture=0.0):
    return po.MeshScene(scene(name, aperture), w, H).frames(0, frames, DEPTH)


def info():
    return int(hippt.load_library().hipptGetOption(hippt.INFO_SKY_COMBINE))


def camera_of(sc, w):
    return hippt.build_camera(lookfrom=sc.lookfrom, lookat=sc.lookat, vup=sc.vup, vfov=sc.vfov, aspect=w / H,
                              aperture=sc.aperture, focus=sc.focus)


def set_camera(cam):
    err = ctypes.c_char_p()
    assert hippt.load_library().hipptSetCamera(ctypes.byref(cam), ctypes.byref(err)), err.value


def both(pt, sc, w, body, band=None, applies=True, setup=None):
    """Runs body(pt) (renders; returns nothing) on a fresh upload with the option automatic and at 0; returns
    {option: (pixels, accum, segments, pixelSamples)} after asserting the two are bit-equal, that the mode
    applied (or did not), and that the counts agree."""
    got = {}
    for opt in (-1, 0):
        pt.setOption(hippt.OPT_SKY_COMBINE, opt)
        pt.setOption(hippt.OPT_ITEM_ORDER, 1)  # the table at once (automatic mode estimates on a thread of its own)
        if setup:
            setup(pt)
        pt.uploadScene(sc)
        assert pt.initialize(w, H), pt.lastError()
        pt.resetStats()
        seen = body(pt)
        px, acc = pt.readback()
        st = pt.stats()
        got[opt] = (px, acc, st["segments"], st["pixelSamples"])
        n = seen if seen is not None else info()
        print(f"option {opt}: HIPPT_INFO_SKY_COMBINE {n}, segments {st['segments']}, samples {st['pixelSamples']}")
        if opt == -1 and applies:
            assert 0 < n < (band if band is not None else w * H), n
        else:
            assert n == 0, n
    diff = int(np.count_nonzero(got[-1][0] != got[0][0]))
    assert diff == 0 and got[-1][1].tobytes() == got[0][1].tobytes(), f"{diff} pixels differ between option -1 and 0"
    assert got[-1][2:] == got[0][2:], (got[-1][2:], got[0][2:])
    return got


def assert_oracle(got, want, rows=slice(None), counts=True):
    for opt in (-1, 0):
        diff = int(np.count_nonzero(got[opt][0][rows] != want[0][rows]))
        assert diff == 0 and got[opt][1][rows].tobytes() == want[1][rows].tobytes(), f"option {opt}: {diff} pixels differ"
        if counts:
            assert got[opt][2:] == (want[2], want[3])


def blocking(pt):
    pt.setOption(hippt.OPT_CHAIN, 0)
    assert pt.renderFrames(SPP, DEPTH), pt.lastError()
    return info()


def test_blocking_render(pt):
    assert_oracle(both(pt, scene(), W, blocking), oracle("cornell34", W, SPP))


def test_width_100(pt):
    """8x8 tiles do not divide 100: runs of 64 consecutive band pixels."""
    assert_oracle(both(pt, scene(), 100, blocking), oracle("cornell34", 100, SPP))


def test_chained_run_then_the_same_frames_again(pt):
    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, 8)
        for _ in range(3):
            assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        n = info()
        px, acc = pt.readback()
        want = oracle("cornell34", W, 3 * SPP)
        assert np.array_equal(px, want[0]) and acc.tobytes() == want[1].tobytes()
        assert pt.resetAccumulation()
        for _ in range(3):
            assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        return n

    got = both(pt, scene(), W, body)
    want = oracle("cornell34", W, 3 * SPP)
    assert_oracle(got, want, counts=False)
    assert got[-1][2:] == (2 * want[2], 2 * want[3])


@pytest.mark.parametrize("w", [W, 100])
def test_held_group(pt, w):
    """A longer first batch, then a burst: the batches that arrive while the run's last launch has not started
    are held and traced as one group.  Width 104: the compacted row length is a multiple of 64 and the batches
    are groupable; width 100: it is not (7200 mod 64 = 32), so the run must not group them (launch_mesh refuses a
    group whose totalItems is no multiple of 64).  The library does not report whether a group formed while the
    mode is on (the audit that would tell turns the mode off), so the image is what is asserted."""
    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, 8)
        assert pt.renderFramesAsync(48, DEPTH), pt.lastError()
        for _ in range(5):
            assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        return info()

    assert_oracle(both(pt, scene(), w, body), oracle("cornell34", w, 48 + 5 * SPP))


def test_row_interleave_share(pt):
    """Rank 1 of 2: rows 1, 3, 5, ...; row runs, their rows two image rows apart."""
    got = both(pt, scene(), W, blocking, band=W * (H // 2), setup=lambda t: t.setRowInterleave(1, 2))
    assert_oracle(got, oracle("cornell34", W, SPP), rows=slice(1, None, 2), counts=False)


def test_cornell_mixed_general_kernel(pt):
    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, 8)
        for _ in range(2):
            assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        return info()

    assert_oracle(both(pt, scene("cornell_mixed"), W, body), oracle("cornell_mixed", W, 2 * SPP))


@pytest.mark.parametrize("chain", [0, 8])
def test_camera_move_before_the_deferred_combine(pt, chain):
    """The batch's combine runs in the next launch, after hipptSetCamera: it must use the batch's camera."""
    sc = scene()
    moved = dataclasses.replace(sc, lookfrom=(sc.lookfrom[0] + 400.0, sc.lookfrom[1] - 250.0, sc.lookfrom[2]))
    cam = camera_of(moved, W)

    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, chain)
        assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        n = info()
        set_camera(cam)
        assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        return n

    got = both(pt, sc, W, body)
    a = oracle("cornell34", W, SPP)
    b = po.MeshScene(sc, W, H, cam=po.PoCamera.from_buffer_copy(bytes(cam))).frames(SPP, SPP, DEPTH, accum=a[1])
    assert_oracle(got, (b[0], b[1]), counts=False)


def test_vertex_update_moves_the_rectangle(pt):
    sc = scene()
    v = verts_of(sc).copy()
    v[0, 0] -= np.float32(900.0)
    want = po.MeshScene(with_verts(sc, v), W, H).frames(0, SPP, DEPTH)
    seen = []

    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, 0)
        assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        seen.append(info())
        pt.updateVertices(v)
        assert pt.resetAccumulation()
        assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        seen.append(info())
        return seen[-1]

    assert_oracle(both(pt, sc, W, body), want, counts=False)
    assert 0 < seen[1] < seen[0]


def test_pixel_format_switch_before_the_flush(pt):
    """A batch enqueued under ARGB, the format switched while its combine is pending, then a batch under RGBA8 whose
    launch takes that combine along: the final words are the oracle's RGBA8 quantization of its accumulation."""
    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, 0)
        pt.setOption(hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB)
        assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        n = info()
        pt.setOption(hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_RGBA8)
        assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        return n

    got = both(pt, scene(), W, body)
    want = oracle("cornell34", W, 2 * SPP)
    assert_oracle(got, (po.rgba8(want[1]).reshape(want[0].shape), want[1], want[2], want[3]))


def test_lens_camera_keeps_every_sample_traced(pt):
    sc = scene(aperture=20.0)
    assert_oracle(both(pt, sc, W, blocking, applies=False), oracle("cornell34", W, SPP, 20.0))


def test_audited_run_keeps_every_sample_traced(pt):
    def body(pt):
        pt.setOption(hippt.OPT_CHAIN, 8)
        pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
        hippt.chain_audit()
        for _ in range(3):
            assert pt.renderFramesAsync(SPP, DEPTH), pt.lastError()
        n = info()
        pt.synchronize()
        return n

    got = both(pt, scene(), W, body, applies=False)
    runs = hippt.chain_audit()
    problems = chain_audit.check(runs)
    assert runs and not problems, problems[:4]
    assert_oracle(got, oracle("cornell34", W, 3 * SPP))



def test_info_reads_zero_after_the_builtin_scene(pt):
    pt.setOption(hippt.OPT_ITEM_ORDER, 1)
    pt.setOption(hippt.OPT_CHAIN, 0)
    pt.uploadScene(scene())
    assert pt.initialize(W, H) and pt.renderFrames(SPP, DEPTH), pt.lastError()
    assert info() > 0
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    assert pt.initialize(W, H) and pt.renderFrame(DEPTH), pt.lastError()
    assert info() == 0
