"""HIPPT_OPT_RENDER_PAD (GPU): the render megakernel's LDS scene copy trims the node boxes of an
LDS-resident 4-wide float tree to the render pad (hippt_slab.h).  The boxes only cull: with
the default trim and without it every image must be the oracle's, bit for bit, chained and unchained, in
either item order, after a vertex update that changes the pad, and over a scene of grazing rays; the
counted pass must show the triangle tests the trim removes; a camera moved out of the pad's extent and
a scene with sliver triangles keep the builder's pad.  Oracle images are computed once per scene."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime

import chain_audit
import hippt
import pyoracle as po
from hippt import scenes
from refit_util import verts_of, with_verts
from render_pad_scenes import GRAZING_SIZE, grazing_scene

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 36, 8, 8
DEFAULT_PAD = 19
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_BVH_QUANT, -1),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_ITEM_ORDER, -1), (hippt.OPT_COUNT_TRAVERSAL, 0),
        (hippt.OPT_RENDER_PAD, DEFAULT_PAD))


SCENES = {"cornell34": scenes.cornell34, "cornell_mixed": scenes.cornell_mixed, "grazing": grazing_scene}


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
    hippt.load_library().cudaPathTracerShutdown()


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def grown(v):
    """Every coordinate x 1.5: the largest |coordinate| passes the camera's 800, so the pad changes."""
    return np.ascontiguousarray(v * np.float32(1.5), np.float32)


@functools.lru_cache(maxsize=None)
def oracle(name, w=W, h=H, spp=SPP, grow=False):
    sc = scene(name)
    if grow:
        sc = with_verts(sc, grown(verts_of(sc)))
    px, acc, segs, _ = po.MeshScene(sc, w, h).frames(0, spp, DEPTH)
    return px, acc, segs


def assert_image(pt, want, what):
    px, acc = pt.readback()
    diff = int(np.count_nonzero(px != want[0]))
    assert diff == 0 and acc.tobytes() == want[1].tobytes(), f"{what}: {diff} pixels differ"


def render_blocking(pt, spp=SPP):
    pt.setOption(hippt.OPT_CHAIN, 0)
    pt.resetStats()
    assert pt.resetAccumulation() and pt.renderFrames(spp, DEPTH), pt.lastError()


def render_chained(pt, spp=SPP, batches=4):
    """The frames as `batches` asynchronous batches of one chained run, audited."""
    pt.setOption(hippt.OPT_CHAIN, 8)
    hippt.chain_audit()
    assert pt.resetAccumulation(), pt.lastError()
    for _ in range(batches):
        assert pt.renderFramesAsync(spp // batches, DEPTH), pt.lastError()


def audit_ok():
    runs = hippt.chain_audit()
    problems = chain_audit.check(runs)
    assert runs and not problems, f"chain audit: {len(runs)} runs, {problems[:4]}"


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("pad", [DEFAULT_PAD, 0])
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_images_are_the_oracles(pt, name, pad, order):
    pt.setOption(hippt.OPT_RENDER_PAD, pad)
    pt.setOption(hippt.OPT_ITEM_ORDER, order)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    pt.uploadScene(scene(name))
    assert pt.initialize(W, H), pt.lastError()
    want = oracle(name)
    render_blocking(pt)
    assert_image(pt, want, f"{name} pad {pad} order {order} unchained")
    assert pt.stats()["segments"] == want[2]
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == pad
    render_chained(pt)
    assert_image(pt, want, f"{name} pad {pad} order {order} chained")
    audit_ok()
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == pad


@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_refit_changes_the_pad(pt, name):
    """One update grows every coordinate by half: the refit recomputes the pad on the device, and the
    next launches trim by it.  The update's image, chained and unchained, is a fresh upload's: both are
    the oracle's for the new vertices."""
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    pt.uploadScene(scene(name))
    assert pt.initialize(W, H), pt.lastError()
    render_blocking(pt)
    assert_image(pt, oracle(name), f"{name} before the update")
    v = grown(verts_of(scene(name)))
    assert float(np.abs(v).max()) > 800.0
    want = oracle(name, grow=True)
    pt.updateVertices(v)
    render_chained(pt)
    assert_image(pt, want, f"{name} updated, chained")
    audit_ok()
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == DEFAULT_PAD
    render_blocking(pt)
    assert_image(pt, want, f"{name} updated, unchained")
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == DEFAULT_PAD
    updated = pt.readback()
    pt.uploadScene(with_verts(scene(name), v))
    render_blocking(pt)
    fresh = pt.readback()
    assert np.array_equal(updated[0], fresh[0]) and updated[1].tobytes() == fresh[1].tobytes()
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == DEFAULT_PAD


@pytest.mark.parametrize("pad", [DEFAULT_PAD, 0])
def test_grazing_scene(pt, pad):
    pt.setOption(hippt.OPT_RENDER_PAD, pad)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    w, h, spp = GRAZING_SIZE
    pt.uploadMesh(scene("grazing"))
    assert pt.initialize(w, h), pt.lastError()
    want = oracle("grazing", w, h, spp)
    render_blocking(pt, spp)
    assert_image(pt, want, f"grazing pad {pad} unchained")
    assert pt.stats()["segments"] == want[2]
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == pad
    render_chained(pt, spp)
    assert_image(pt, want, f"grazing pad {pad} chained")
    audit_ok()
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == pad


def set_camera(sc, w, h):
    cam = hippt.build_camera(lookfrom=sc.lookfrom, lookat=sc.lookat, vup=sc.vup, vfov=sc.vfov, aspect=w / h,
                             aperture=sc.aperture, focus=sc.focus)
    err = ctypes.c_char_p()
    assert hippt.load_library().hipptSetCamera(ctypes.byref(cam), ctypes.byref(err)), err.value


def test_far_camera_keeps_the_builders_pad(pt):
    """The bound behind the trim needs every ray origin within M, the largest |coordinate| the pad was
    sized from at the upload.  hipptSetCamera can move the camera out of it (here 20 times further, a
    long lens on the room): those launches keep the builder's pad, chained and unchained, the image is the
    oracle's, and the trim is back once the camera is."""
    base = scene("cornell34")
    far = dataclasses.replace(base, lookfrom=(278.0, 278.0, -16000.0), vfov=2.2)
    want = po.MeshScene(far, W, H).frames(0, SPP, DEPTH)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    pt.uploadMesh(base)
    assert pt.initialize(W, H), pt.lastError()
    render_blocking(pt)
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == DEFAULT_PAD
    set_camera(far, W, H)
    render_blocking(pt)
    assert_image(pt, want, "far camera, unchained")
    assert pt.stats()["segments"] == want[2]
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == 0
    render_chained(pt)
    assert_image(pt, want, "far camera, chained")
    audit_ok()
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == 0
    set_camera(base, W, H)
    render_blocking(pt)
    assert_image(pt, oracle("cornell34"), "camera back")
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == DEFAULT_PAD


def test_sliver_triangles_keep_the_builders_pad(pt):
    """The bound also needs every triangle's edges to meet at a sine of at least 0.3 (the error of an
    accepted hit's t grows with 1 / sine): a scene with one thin sliver is not trimmed; once an update
    fattens the sliver it is."""
    base = scene("cornell34")
    sliver = np.asarray([[100, 100, 200, 400, 100, 200, 400, 110, 200]], np.float32)
    fat = np.asarray([[100, 100, 200, 400, 100, 200, 400, 400, 200]], np.float32)
    thin = dataclasses.replace(base, verts=np.concatenate([verts_of(base), sliver]),
                               tri_mat=np.concatenate([base.tri_mat, np.zeros(1, np.int32)]))
    pt.uploadMesh(thin)
    assert pt.initialize(W, H), pt.lastError()
    want = po.MeshScene(thin, W, H).frames(0, SPP, DEPTH)
    render_blocking(pt)
    assert_image(pt, want, "sliver scene")
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == 0
    v = np.concatenate([verts_of(base), fat])
    want = po.MeshScene(with_verts(thin, v), W, H).frames(0, SPP, DEPTH)
    pt.updateVertices(v)
    render_blocking(pt)
    assert_image(pt, want, "sliver fattened")
    assert hippt.load_library().hipptGetOption(hippt.INFO_RENDER_PAD) == DEFAULT_PAD


def test_trim_removes_triangle_tests(pt):
    """A counted pass of cornell34: the same segments and image, fewer triangle tests per segment with the
    trim (a scattered ray's own flat leaf is culled at its parent's visit)."""
    pt.setOption(hippt.OPT_COUNT_TRAVERSAL, 1)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    pt.uploadMesh(scene("cornell34"))
    assert pt.initialize(W, H), pt.lastError()
    want = oracle("cornell34")
    got = {}
    for pad in (0, DEFAULT_PAD):
        pt.setOption(hippt.OPT_RENDER_PAD, pad)
        render_blocking(pt)
        assert_image(pt, want, f"counted pass, pad {pad}")
        got[pad] = pt.stats()
        assert got[pad]["segments"] == want[2]
    per = {pad: (s["triTests"] / s["segments"], s["nodeVisits"] / s["segments"]) for pad, s in got.items()}
    print(f"triTests/segment: {per[0][0]:.4f} without the trim, {per[DEFAULT_PAD][0]:.4f} with it; "
          f"nodeVisits/segment: {per[0][1]:.4f}, {per[DEFAULT_PAD][1]:.4f}")
    assert got[DEFAULT_PAD]["triTests"] < got[0]["triTests"]
    assert got[DEFAULT_PAD]["nodeVisits"] <= got[0]["nodeVisits"]
