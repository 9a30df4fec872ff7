"""hipptUpdateVertices (GPU): in-place vertex updates with the device BVH refit.

"The BVH only culls": after an update every render and ray query must give, bit for bit, what the
oracle gives for the new vertices, and the refitted device trees must be the builder's rule applied
to them (refit_util.check_refit).  Oracle images are computed once per (scene, deformation)."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.updateVertices)

import chain_audit
import hippt
import pyoracle as po
from refit_util import (check_refit, pad_of, scatter, sphere_boxes, refit_scenes, tri_boxes, verts_of, with_verts,
                        wobble)
from test_gpu_ray_query import Ref, camera_rays

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 45, 26, 2, 4
SCENES = refit_scenes()
DEFORMS = ("wobble", "scatter", "restore")
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_BVH_QUANT, -1),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0))
BUFFERS = (hippt.SCENE_NODES2, hippt.SCENE_NODES4, hippt.SCENE_PRIMS, hippt.SCENE_SHADE)


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


@functools.lru_cache(maxsize=None)
def verts(name, deform):
    v0 = verts_of(scene(name))
    return {"wobble": wobble, "scatter": scatter, "restore": lambda v: v, "base": lambda v: v}[deform](v0)


@functools.lru_cache(maxsize=None)
def oracle(name, deform, w=W, h=H):
    """(pixels, accumulation, segments) of frames 0..SPP-1 over the deformed scene."""
    px, acc, segs, _ = po.MeshScene(with_verts(scene(name), verts(name, deform)), w, h).frames(0, SPP, DEPTH)
    return px, acc, segs


def start(pt, name, opts=(), w=W, h=H):
    for k, v in opts:
        pt.setOption(k, v)
    pt.uploadScene(scene(name))
    assert pt.initialize(w, h), pt.lastError()


def render(pt):
    assert pt.resetAccumulation() and pt.renderFrames(SPP, DEPTH), pt.lastError()
    return pt.readback()


def assert_image(got, want, what):
    px, acc = got
    diff = int(np.count_nonzero(px != want[0]))
    assert diff == 0 and acc.tobytes() == want[1].tobytes(), f"{what}: {diff} pixels differ"


def download():
    return [hippt.scene_download(b) for b in BUFFERS]


def check_device_trees(name, v, bufs, before):
    """The downloaded trees against the numpy rule; primitive boxes from v through the records' ids."""
    sc = scene(name)
    n2, n4, prims, _ = bufs
    ids = prims[:, 9].view(np.int32)
    boxes = np.concatenate([tri_boxes(v), sphere_boxes(sc.spheres)])
    assert sorted(ids.tolist()) == list(range(len(boxes)))
    assert np.array_equal(prims[:, 10] == 1, ids >= len(v))
    pbox = boxes[ids]
    pad = pad_of(pbox, float(np.abs(np.asarray(sc.lookfrom, np.float32)).max()))

    def index_codes(nodes4):  # device layout: interior codes are byte offsets
        out = nodes4.copy()
        c = out[:, 24:28].view(np.int32)
        c[c >= 0] >>= 7
        return out
    assert check_refit(n2, 2, pbox, pad, before[0]) > 0
    assert check_refit(index_codes(n4), 4, pbox, pad, index_codes(before[1])) > 0


CONFIGS = {"mega": (), "mega_no_lds": ((hippt.OPT_LDS_SCENE, 0),), "width2": ((hippt.OPT_BVH_WIDTH, 2),),
           "width4": ((hippt.OPT_BVH_WIDTH, 4),), "wavefront": ((hippt.OPT_PATH_MODE, 1),),
           "half": ((hippt.OPT_BVH_QUANT, 3),)}


# ---- 1. parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(SCENES))
def test_parity_after_each_update(pt, name, config):
    start(pt, name, CONFIGS[config])
    first = render(pt)
    assert_image(first, oracle(name, "base"), f"{name} {config} before any update")
    for deform in DEFORMS:
        if deform != "restore":  # (the deformation shows: an update that did nothing would fail below)
            assert oracle(name, deform)[1].tobytes() != oracle(name, "base")[1].tobytes()
        pt.updateVertices(verts(name, deform))
        got = render(pt)
        assert_image(got, oracle(name, deform), f"{name} {config} after {deform}")
    assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()


# ---- 2. tree and records ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_refitted_trees_and_records(pt, name):
    start(pt, name)
    before = download()
    after = {}
    for deform in DEFORMS:
        pt.updateVertices(verts(name, deform))
        after[deform] = download()
        check_device_trees(name, verts(name, deform), after[deform], before)
    assert pt.updateDropped() == 0
    for got, want in zip(after["restore"], before):
        assert got.tobytes() == want.tobytes()
    for deform in ("wobble", "scatter"):  # the records of a fresh upload of the same vertices
        pt.uploadScene(with_verts(scene(name), verts(name, deform)))
        fresh = download()
        for b in (2, 3):
            assert after[deform][b][np.argsort(after[deform][2][:, 9])].tobytes() == \
                fresh[b][np.argsort(fresh[2][:, 9])].tobytes(), (deform, b)


# ---- 3. device vertices -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_mixed", "blob32x17"])
def test_device_vertices(pt, name):
    assert torch.cuda.is_available()
    pt.setDevices([0])
    start(pt, name)
    before = download()
    v1 = verts(name, "wobble")
    pt.updateVertices(v1)
    host_bufs, host_img = download(), render(pt)
    pt.updateVertices(verts(name, "scatter"))  # something else in between
    dv = torch.from_numpy(v1.copy()).to(torch.device("cuda", 0))
    pt.updateVertices(dv)
    dev_bufs, dev_img = download(), render(pt)
    for a, b in zip(dev_bufs, host_bufs):
        assert a.tobytes() == b.tobytes()
    assert_image(dev_img, host_img, f"{name} device vertices")
    assert_image(dev_img, oracle(name, "wobble"), f"{name} device vertices")
    assert pt.updateDropped() == 0
    # a non-finite coordinate the call cannot see: that triangle becomes one no ray hits
    bad = v1.copy()
    k = len(bad) // 2
    bad[k, 4] = np.nan
    pt.updateVertices(torch.from_numpy(bad).to(dv.device))
    got = render(pt)
    assert pt.updateDropped() == 1
    zeroed = v1.copy()
    zeroed[k] = 0.0
    opx, oacc, _, _ = po.MeshScene(with_verts(scene(name), zeroed), W, H).frames(0, SPP, DEPTH)
    assert_image(got, (opx, oacc), f"{name} dropped triangle")
    check_device_trees(name, bad, download(), before)
    # the host copy took the same update: a new Init uploads it
    assert pt.initialize(W, H), pt.lastError()
    assert_image(render(pt), (opx, oacc), f"{name} dropped triangle after a new Init")
    # pointers that are not device memory
    e = ctypes.c_char_p()
    assert not hippt.load_library().hipptUpdateVertices(v1.ctypes.data, len(v1), hippt.VERTS_DEVICE, ctypes.byref(e))
    assert b"device" in e.value
    del dv


# ---- 4. order and pipeline ----------------------------------------------------------------------------
@pytest.mark.parametrize("audit", [0, 1])
@pytest.mark.parametrize("name", ["cornell34", "blob32x17"])
def test_update_between_async_frames_is_in_stream_order(pt, name, audit):
    opts = ((hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 1)) if audit else ()
    start(pt, name, opts)
    hippt.chain_audit()  # (drops records of earlier tests)
    pt.resetStats()
    v1 = verts(name, "wobble")
    for _ in range(3):
        assert pt.renderFramesAsync(1, DEPTH), pt.lastError()
    pt.updateVertices(v1)  # no synchronise
    for _ in range(3):
        assert pt.renderFramesAsync(1, DEPTH), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    px, acc = pt.readback()
    sc = scene(name)
    _, acc0, segs0, _ = po.MeshScene(sc, W, H).frames(0, 3, DEPTH)
    opx, oacc, segs1, _ = po.MeshScene(with_verts(sc, v1), W, H).frames(3, 3, DEPTH, accum=acc0)
    assert_image((px, acc), (opx, oacc), f"{name} frames 0-2 over V0, 3-5 over V1")
    assert pt.stats()["segments"] == segs0 + segs1
    if audit:
        runs = hippt.chain_audit()
        problems = chain_audit.check(runs)
        assert runs and not problems, problems[:6]
        for hdr, _ in runs:  # no run spans the update: frames 0-2 before it, 3-5 after
            first = hdr["firstFrame"]
            last = first + max(hdr["step"], 0) * (hdr["batches"] - 1) + hdr["frames"] - 1
            assert last <= 2 or first >= 3, hdr


# ---- 5. queries and contexts --------------------------------------------------------------------------
def test_ray_queries_see_the_update(pt):
    name = "cornell_mixed"
    start(pt, name)
    v1 = verts(name, "wobble")
    pt.updateVertices(v1)
    sc1 = with_verts(scene(name), v1)
    ref = Ref(sc1)
    rays = camera_rays(sc1, W, H, 0)
    rt, rp = ref.closest(rays)
    assert (rp >= 0).any() and (rp < 0).any()
    t, prim = pt.traceRays(rays)
    assert t.tobytes() == rt.tobytes() and np.array_equal(prim, rp)
    ct, cp = pt.traceCamera(0)
    assert ct.reshape(-1).tobytes() == rt.tobytes() and np.array_equal(cp.reshape(-1), rp)


@pytest.mark.parametrize("name", ["cornell34", "blob32x17"])
def test_contexts_and_the_host_copy(pt, name):
    pt.setDevices([0, 0, 0])
    start(pt, name)
    render(pt)
    pt.updateVertices(verts(name, "scatter"))
    pt.updateVertices(verts(name, "wobble"))
    assert_image(render(pt), oracle(name, "wobble"), f"{name} three contexts")
    # the host copy: a new Init at another size, then other devices, render the updated scene
    w, h = 38, 21
    assert pt.initialize(w, h), pt.lastError()
    assert_image(render(pt), oracle(name, "wobble", w, h), f"{name} after a new Init")
    pt.setDevices([0])
    assert pt.initialize(W, H), pt.lastError()
    assert_image(render(pt), oracle(name, "wobble"), f"{name} after setDevices")
    pt.updateVertices(verts(name, "restore"))
    assert_image(render(pt), oracle(name, "base"), f"{name} restored")
