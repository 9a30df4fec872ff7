"""HIPPT_OPT_SKY_RECT (GPU): the camera-pool megakernels finish a wave's 64 new work items on the spot, as
sky misses, when every one of them is of a pixel outside the screen rectangle the scene's bounding box
projects into (hippt_sky_rect.h).  The rectangle only skips traversals that must miss: with
the option on and off every image must be the oracle's, bit for bit, with the same segment and sample
counts; chained and unchained; for a width the 8x8 tiles do not divide; after hipptSetCamera moves
(scene half off-screen, only sky, camera inside the box, a far camera with a short focus distance); for
an interleaved row share; and around a device-memory vertex update, during which the rectangle is off.  The counted pass must show exactly one
node visit fewer per skipped sample.  Oracle images are computed once per case."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime

import chain_audit
import hippt
import pyoracle as po
from hippt import scenes
from refit_util import verts_of, with_verts

pytestmark = pytest.mark.gpu

SPP, DEPTH = 4, 8
SIZES = ((96, 54), (100, 54))
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_BVH_QUANT, -1),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_ITEM_ORDER, -1), (hippt.OPT_COUNT_TRAVERSAL, 0),
        (hippt.OPT_CAMERA_POOL, -1), (hippt.OPT_PIXEL_TILE, -1), (hippt.OPT_SKY_RECT, 1))

SCENES = {"cornell34": scenes.cornell34, "blob70k": scenes.blob70k, "cornell_mixed": scenes.cornell_mixed,
          "random_scene": scenes.random_scene}
# hipptSetCamera moves of cornell34's camera
MOVES = {
    "half_off_screen": dict(lookat=(278.0 + 450.0, 278.0, 0.0)),
    "only_sky": dict(lookat=(278.0 + 866.0, 278.0, -800.0 + 500.0)),
    "inside": dict(lookfrom=(278.0, 278.0, 278.0), lookat=(278.0, 278.0, 555.0)),
    # far, oblique, long lens, focus 1: the direction's rounding may be half a pixel at 96x54 (tests/test_sky_rect.py)
    "far_short_focus": dict(lookfrom=(5278.0, 2278.0, -6000.0), lookat=(278.0, 278.0, 278.0), vfov=6.0, focus=1.0),
}


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
def scene(name, move=None):
    sc = SCENES[name]()
    return dataclasses.replace(sc, **MOVES[move]) if move else sc


@functools.lru_cache(maxsize=None)
def oracle(name, w, h, spp=SPP, move=None):
    px, acc, segs, samples = po.MeshScene(scene(name, move), w, h).frames(0, spp, DEPTH)
    return px, acc, segs, samples


def sky_pixels():
    return int(hippt.load_library().hipptGetOption(hippt.INFO_SKY_RECT_PIXELS))


def assert_image(pt, want, what, rows=slice(None)):
    px, acc = pt.readback()
    diff = int(np.count_nonzero(px[rows] != want[0][rows]))
    assert diff == 0 and acc[rows].tobytes() == want[1][rows].tobytes(), f"{what}: {diff} pixels differ"


def render_blocking(pt, spp=SPP):
    pt.setOption(hippt.OPT_CHAIN, 0)
    pt.resetStats()
    assert pt.resetAccumulation() and pt.renderFrames(spp, DEPTH), pt.lastError()


def render_chained(pt, spp, batches):
    """`batches` asynchronous batches of spp frames each, one chained run, audited."""
    pt.setOption(hippt.OPT_CHAIN, 8)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    hippt.chain_audit()
    pt.resetStats()
    assert pt.resetAccumulation(), pt.lastError()
    for _ in range(batches):
        assert pt.renderFramesAsync(spp, DEPTH), pt.lastError()


def audit_ok():
    runs = hippt.chain_audit()
    problems = chain_audit.check(runs)
    assert runs and not problems, f"chain audit: {len(runs)} runs, {problems[:4]}"


def set_camera(sc, w, h):
    cam = hippt.build_camera(lookfrom=sc.lookfrom, lookat=sc.lookat, vup=sc.vup, vfov=sc.vfov, aspect=w / h,
                             aperture=sc.aperture, focus=sc.focus)
    err = ctypes.c_char_p()
    assert hippt.load_library().hipptSetCamera(ctypes.byref(cam), ctypes.byref(err)), err.value
    return cam


def on_and_off(pt, want, what, rows=slice(None), total=True):
    """The image with the option on and off: both the oracle's, with equal counters.  Returns the
    rectangle's pixel count with the option on."""
    got = {}
    for on in (1, 0):
        pt.setOption(hippt.OPT_SKY_RECT, on)
        render_blocking(pt)
        assert_image(pt, want, f"{what}, option {on}", rows)
        st = pt.stats()
        got[on] = (st["segments"], st["pixelSamples"], sky_pixels())
    pt.setOption(hippt.OPT_SKY_RECT, 1)
    assert got[1][:2] == got[0][:2], what
    if total:
        assert got[1][:2] == (want[2], want[3]), what
    assert got[0][2] == 0
    return got[1][2]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_images_are_the_oracles(pt, name, size):
    w, h = size
    pt.uploadScene(scene(name))
    assert pt.initialize(w, h), pt.lastError()
    outside = on_and_off(pt, oracle(name, w, h), f"{name} {w}x{h}")
    print(f"{name} {w}x{h}: {outside} of {w * h} pixels outside the rectangle")
    if name == "random_scene":  # its own aperture: a lens camera has no rectangle
        assert scene(name).aperture != 0 and outside == 0
    else:
        assert w * h // 3 <= outside < w * h


def test_camera_moves(pt):
    w, h = SIZES[0]
    pt.uploadMesh(scene("cornell34"))
    assert pt.initialize(w, h), pt.lastError()
    base = on_and_off(pt, oracle("cornell34", w, h), "before the moves")
    set_camera(scene("cornell34", "half_off_screen"), w, h)
    half = on_and_off(pt, oracle("cornell34", w, h, move="half_off_screen"), "scene half off-screen")
    assert 0 < half < w * h and half != base
    # only sky: every sample takes the fast path
    set_camera(scene("cornell34", "only_sky"), w, h)
    want = oracle("cornell34", w, h, move="only_sky")
    assert want[2] == want[3] == w * h * SPP  # (one segment per sample: the oracle sees no hit)
    assert on_and_off(pt, want, "only sky") == w * h
    set_camera(scene("cornell34", "inside"), w, h)
    assert on_and_off(pt, oracle("cornell34", w, h, move="inside"), "camera inside the box") == 0
    set_camera(scene("cornell34", "far_short_focus"), w, h)
    assert on_and_off(pt, oracle("cornell34", w, h, move="far_short_focus"), "far camera, focus 1") == 0
    set_camera(scene("cornell34"), w, h)
    assert on_and_off(pt, oracle("cornell34", w, h), "camera back") == base


def test_row_interleave(pt):
    """Rank 1 of 4: rows 1, 5, 9, ... of the image; the test is on image coordinates."""
    w, h = SIZES[1]
    pt.setRowInterleave(1, 4)
    pt.uploadMesh(scene("cornell34"))
    assert pt.initialize(w, h), pt.lastError()
    outside = on_and_off(pt, oracle("cornell34", w, h), "rows 1 mod 4", rows=slice(1, None, 4), total=False)
    assert outside > 0


@pytest.mark.parametrize("name", ["cornell34", "blob70k", "cornell_mixed"])
def test_chained_run_audited(pt, name):
    w, h = SIZES[1]
    pt.uploadScene(scene(name))
    assert pt.initialize(w, h), pt.lastError()
    want = oracle(name, w, h, spp=6 * SPP)
    got = {}
    for on in (1, 0):
        pt.setOption(hippt.OPT_SKY_RECT, on)
        render_chained(pt, SPP, 6)
        assert_image(pt, want, f"{name} chained, option {on}")
        audit_ok()
        st = pt.stats()
        got[on] = (st["segments"], st["pixelSamples"])
        assert (sky_pixels() > 0) == (on == 1)
    assert got[1] == got[0] == (want[2], want[3])


def test_device_memory_update(pt):
    """A device-memory update that pushes a vertex far outside the old rectangle: the rectangle is off
    until the host copy has the vertices (a host-memory update brings it along), and comes back wider."""
    w, h = SIZES[0]
    base = scene("cornell34")
    pt.uploadMesh(base)
    assert pt.initialize(w, h), pt.lastError()
    before = on_and_off(pt, oracle("cornell34", w, h), "before the update")
    v = verts_of(base).copy()
    v[0, 0] -= np.float32(1500.0)  # off the left edge of the image at any depth of the room
    want = po.MeshScene(with_verts(base, v), w, h).frames(0, SPP, DEPTH)
    assert np.any(want[0] != oracle("cornell34", w, h)[0])
    dv = torch.from_numpy(v).to(torch.device("cuda", 0))
    pt.updateVertices(dv)
    render_blocking(pt)
    assert_image(pt, want, "device-memory update")
    assert sky_pixels() == 0
    assert (pt.stats()["segments"], pt.stats()["pixelSamples"]) == (want[2], want[3])
    pt.updateVertices(v)
    after = on_and_off(pt, want, "host-memory update")
    assert 0 < after < before


def rule(cam, w, h, lo, hi, pad):
    """hippt_sky_rect.h's rule restated: the rectangle (x0, y0, x1, y1) of a pinhole camera in front of
    the box."""
    o, llc, hz, vt = (np.asarray(getattr(cam, k)[:], np.float64) for k in ("origin", "llc", "horizontal", "vertical"))
    A = np.stack([llc - o, hz, vt], axis=1)
    invw, invh = float(np.float32(1.0) / np.float32(max(1, w - 1))), float(np.float32(1.0) / np.float32(max(1, h - 1)))
    px, py = [], []
    for c in range(8):
        q = np.array([(hi[k] + pad) if (c >> k) & 1 else (lo[k] - pad) for k in range(3)], np.float64) - o
        lam, ls, lt = np.linalg.solve(A, q)
        assert lam > 0
        px.append(ls / lam / invw)
        py.append(lt / lam / invh)
    ex, ey = 1.0 + w * 2.0 ** -20, 1.0 + h * 2.0 ** -20
    clamp = lambda d, n: int(min(max(d, 0), n))
    return (clamp(np.ceil(min(px) - ex - 1.0), w), clamp(np.ceil(min(py) - ey - 1.0), h),
            clamp(np.floor(max(px) + ex) + 1.0, w), clamp(np.floor(max(py) + ey) + 1.0, h))


def test_counted_pass_skips_one_node_visit_per_sample(pt):
    """cornell34's tree is LDS-resident: a camera ray that misses visits the root and nothing else, so the
    counted pass with the option on reports one node visit fewer for every sample of a run of 64 items that
    lies wholly outside the rectangle.  The runs (item_order.h): 8x8 tiles over the image's whole strips
    of 8 rows, then 64 consecutive pixels over the rest.  8 spp: each of the 8 work queues then holds whole
    runs of one frame (96 * 54 * 8 / 8 = 81 * 64), so a wave's 64 new items are always one run, whatever
    the launch's timing (at 4 spp the queues' ends split runs between waves)."""
    w, h = SIZES[0]
    spp = 8
    assert (w * h * spp) % 512 == 0 and (w * h) % 64 == 0
    sc = scene("cornell34")
    pt.setOption(hippt.OPT_COUNT_TRAVERSAL, 1)
    pt.setOption(hippt.OPT_ITEM_ORDER, 1)
    pt.setOption(hippt.OPT_PIXEL_TILE, 8)
    pt.uploadMesh(sc)
    assert pt.initialize(w, h), pt.lastError()
    want = oracle("cornell34", w, h, spp=spp)
    got = {}
    for on in (1, 0):
        pt.setOption(hippt.OPT_SKY_RECT, on)
        render_blocking(pt, spp)
        assert_image(pt, want, f"counted pass, option {on}")
        got[on] = pt.stats()
        assert (got[on]["segments"], got[on]["pixelSamples"]) == (want[2], want[3])
        if on:
            outside = sky_pixels()
    # the rectangle, restated: the root box is the vertices' box moved out by the builder's pad
    p = verts_of(sc).reshape(-1, 3)
    M = np.float32(max(float(np.abs(p).max()), max(abs(c) for c in sc.lookfrom)))
    pad = np.float32(M * np.float32(2.0 ** -16))
    lo, hi = (p.min(axis=0) - pad).astype(np.float32), (p.max(axis=0) + pad).astype(np.float32)
    cam = hippt.build_camera(lookfrom=sc.lookfrom, lookat=sc.lookat, vup=sc.vup, vfov=sc.vfov, aspect=w / h,
                             aperture=sc.aperture, focus=sc.focus)
    x0, y0, x1, y1 = rule(cam, w, h, lo.astype(np.float64), hi.astype(np.float64), float(pad))
    assert outside == w * h - (x1 - x0) * (y1 - y0)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    sky = ~((x >= x0) & (x < x1) & (y >= y0) & (y < y1))
    strips = h // 8 * 8
    tiles = sky[:strips].reshape(strips // 8, 8, w // 8, 8).all(axis=(1, 3)).ravel()
    runs = np.concatenate([tiles, sky[strips:].reshape(-1, 64).all(axis=1)])
    skipped = int(runs.sum()) * 64 * spp
    print(f"{outside} pixels outside, {int(runs.sum())} of {runs.size} runs per frame wholly outside: {skipped} samples; "
          f"nodeVisits {got[0]['nodeVisits']} -> {got[1]['nodeVisits']}")
    assert skipped > 0
    assert got[1]["nodeVisits"] == got[0]["nodeVisits"] - skipped
