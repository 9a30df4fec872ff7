"""Host refit (hipptBvhRefit, bvh_builder refit_bvh): new boxes for an unchanged topology by the
builder's own rule, checked against the rule restated in numpy (refit_util.check_refit), and the
argument errors of hipptBvhRefit and hipptUpdateVertices that need no device."""
import ctypes

import numpy as np
import pytest

import hippt
from hippt import scenes
from refit_util import (check_refit, pad_of, scatter, refit_scenes, tri_boxes, verts_of, wobble)

HINT = 800.0
SCENES = dict(refit_scenes(), blob20k=lambda: scenes.blob_scene(137, 73))


@pytest.fixture(scope="module", params=sorted(SCENES))
def built(request):
    v0 = verts_of(SCENES[request.param]())
    bvh = hippt.Bvh(v0, extent_hint=HINT)
    return v0, bvh, (bvh.nodes.copy(), bvh.nodes4.copy(), bvh.nodes4q.copy(), bvh.order.copy())


def _same(bvh, snap):
    return (bvh.nodes.tobytes() == snap[0].tobytes() and bvh.nodes4.tobytes() == snap[1].tobytes() and
            bvh.nodes4q.tobytes() == snap[2].tobytes() and np.array_equal(bvh.order, snap[3]))


def _quantized_contain_float(bvh):
    q, n4 = bvh.nodes4q, bvh.nodes4
    assert q.shape == (len(n4), 16)
    f = n4[:, :24].view(np.float32).reshape(-1, 3, 2, 4).astype(np.float64)  # node, axis, lo/hi, slot
    kids = n4[:, 24:28].view(np.int32)
    assert np.array_equal(q[:, 12:16].view(np.int32), kids)
    origin = q[:, 0:3].view(np.float32).astype(np.float64)
    scale = np.stack([q[:, 3], q[:, 10], q[:, 11]], axis=1).view(np.float32).astype(np.float64)
    planes = q[:, 4:10].view(np.uint8).reshape(-1, 3, 2, 4).astype(np.float64)
    used = (kids != -1)[:, None, :]
    lo = origin[:, :, None] + planes[:, :, 0, :] * scale[:, :, None]
    hi = origin[:, :, None] + planes[:, :, 1, :] * scale[:, :, None]
    assert np.all((lo <= f[:, :, 0, :]) | ~used) and np.all((hi >= f[:, :, 1, :]) | ~used)


def test_refit_to_the_same_vertices_gives_the_builds_bytes(built):
    v0, bvh, snap = built
    bvh.refit(v0)
    assert _same(bvh, snap)


@pytest.mark.parametrize("deform", [wobble, scatter])
def test_refit_boxes_are_the_padded_unions_of_their_subtrees(built, deform):
    v0, bvh, snap = built
    v1 = deform(v0)
    assert not np.array_equal(v0, v1)
    bvh.refit(v1)
    try:
        assert np.array_equal(bvh.order, snap[3])
        pbox = tri_boxes(v1)[bvh.order]
        pad = pad_of(pbox, HINT)
        assert check_refit(bvh.nodes, 2, pbox, pad, snap[0]) > 0
        assert check_refit(bvh.nodes4, 4, pbox, pad, snap[1]) > 0
        _quantized_contain_float(bvh)
    finally:
        bvh.refit(v0)
    assert _same(bvh, snap)  # scatter (or wobble), then restore: the original bytes


def test_refit_argument_errors_leave_the_trees_unchanged(built):
    v0, bvh, snap = built
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    p = v0.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n = len(v0)
    assert not lib.hipptBvhRefit(bvh._h, p, n + 1, HINT, ctypes.byref(e)) and b"numTris" in e.value
    assert not lib.hipptBvhRefit(bvh._h, p, 0, HINT, ctypes.byref(e)) and b"numTris" in e.value
    assert not lib.hipptBvhRefit(bvh._h, None, n, HINT, ctypes.byref(e)) and b"null" in e.value
    assert not lib.hipptBvhRefit(None, p, n, HINT, ctypes.byref(e)) and b"null" in e.value
    for bad in (np.nan, np.inf, -np.inf):
        v = v0.copy()
        v[len(v) // 2, 4] = bad
        with pytest.raises(hippt.HipptError, match="non-finite"):
            bvh.refit(v)
    bvh._read()
    assert _same(bvh, snap)


@pytest.fixture()
def lib():
    L = hippt.load_library()
    L.cudaPathTracerShutdown()  # no Init
    yield L
    hippt.PathTracer().useBuiltinScene(hippt.SCENE_SPHERE4)
    L.cudaPathTracerShutdown()


def _update(L, verts, n, flags=0):
    e = ctypes.c_char_p()
    ok = L.hipptUpdateVertices(verts.ctypes.data if verts is not None else None, n, flags, ctypes.byref(e))
    return ok, (e.value or b"").decode()


def test_update_vertices_errors_that_need_no_device(lib):
    assert "hipptUpdateVertices" in hippt.EXPORTS and "hipptSceneDownload" in hippt.EXPORTS
    assert hippt.VERTS_DEVICE == 1 and hippt.INFO_UPDATE_DROPPED == 104
    sc = scenes.cornell34()
    v = verts_of(sc)
    pt = hippt.PathTracer()
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    ok, msg = _update(lib, v, len(v))
    assert not ok and ("built-in" in msg or "no mesh" in msg)
    pt.uploadMesh(sc)
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    ok, msg = _update(lib, v, len(v))
    assert not ok and "built-in" in msg
    pt.uploadMesh(sc)
    for n in (len(v) - 1, len(v) + 1, 0, -3):
        ok, msg = _update(lib, v, n)
        assert not ok and "numTris" in msg
    ok, msg = _update(lib, None, len(v))
    assert not ok and "null" in msg
    ok, msg = _update(lib, v, len(v), flags=hippt.VERTS_DEVICE)  # no Init yet
    assert not ok and "initialized" in msg
    ok, msg = _update(lib, v, len(v), flags=2)
    assert not ok and "flags" in msg
    bad = v.copy()
    bad[3, 7] = np.nan
    ok, msg = _update(lib, bad, len(v))
    assert not ok and "non-finite" in msg
    # host vertices before an Init are allowed: they update the host copy only
    ok, msg = _update(lib, wobble(v), len(v))
    assert ok, msg
    ok, msg = _update(lib, v, len(v))
    assert ok, msg
    assert lib.hipptGetOption(hippt.INFO_UPDATE_DROPPED) == 0
    # the wrapper validates before any call
    for wrong in (v.astype(np.float64), v.reshape(-1, 3), v[:, ::-1], v.tolist()):
        with pytest.raises(hippt.HipptError, match="verts must"):
            pt.updateVertices(wrong)
    e = ctypes.c_char_p()
    assert lib.hipptSceneDownload(9, None, 0, ctypes.byref(e)) == -1 and b"unknown" in e.value
    assert lib.hipptSceneDownload(hippt.SCENE_PRIMS, None, 0, ctypes.byref(e)) == len(v) * 48
    buf = np.zeros(len(v) * 12, np.uint32)
    assert lib.hipptSceneDownload(hippt.SCENE_PRIMS, buf.ctypes.data, buf.nbytes, ctypes.byref(e)) == -1
    assert b"not initialized" in e.value
