"""Host-only checks of the ray queries (hipptTraceRays, hipptOccluded, hipptTraceCamera): the
exports and their signatures, the slice option, the argument errors (each returns false with a
message before anything touches a device), and the Python wrapper's validation of a ray batch."""
import ctypes
import os
import re

import numpy as np
import pytest

import hippt
from hippt import scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ("hipptTraceRays", "hipptOccluded", "hipptTraceCamera")


def test_exports_signatures_and_option():
    lib = hippt.load_library()
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    for name in QUERIES:
        assert name in hippt.EXPORTS
        assert getattr(lib, name).restype is ctypes.c_bool
    assert ("bool hipptTraceRays(const float *rays, long long numRays, int flags, float *t, int *prim, "
            "const char **errorMessage);") in header
    assert ("bool hipptOccluded(const float *rays, long long numRays, int flags, unsigned char *occluded, "
            "const char **errorMessage);") in header
    assert "bool hipptTraceCamera(int frame, int flags, float *t, int *prim, const char **errorMessage);" in header
    assert re.search(r"enum\s*\{\s*HIPPT_RAYS_DEVICE\s*=\s*1\s*\}", header) and hippt.RAYS_DEVICE == 1
    assert re.search(r"HIPPT_OPT_QUERY_SLICE\s*=\s*33\b", header) and hippt.OPT_QUERY_SLICE == 33
    assert len(lib.hipptTraceRays.argtypes) == 6 and len(lib.hipptOccluded.argtypes) == 5
    assert len(lib.hipptTraceCamera.argtypes) == 5
    assert lib.hipptGetOption(hippt.OPT_QUERY_SLICE) == 0
    try:
        for v in (64, 1000, 1 << 28):
            assert lib.hipptSetOption(hippt.OPT_QUERY_SLICE, v) and lib.hipptGetOption(hippt.OPT_QUERY_SLICE) == v
        for v in (-1, (1 << 28) + 1):
            assert not lib.hipptSetOption(hippt.OPT_QUERY_SLICE, v)
            assert lib.hipptGetOption(hippt.OPT_QUERY_SLICE) == 1 << 28
    finally:
        assert lib.hipptSetOption(hippt.OPT_QUERY_SLICE, 0)


@pytest.fixture()
def lib():
    L = hippt.load_library()
    L.cudaPathTracerShutdown()  # no Init
    yield L
    hippt.PathTracer().useBuiltinScene(hippt.SCENE_SPHERE4)
    L.cudaPathTracerShutdown()


def _calls(L, rays, n, t, prim, occ, flags=0):
    """The three entry points with these buffers: [(name, ok, message)]."""
    out = []
    for name, call in (("trace", lambda e: L.hipptTraceRays(rays, n, flags, t, prim, e)),
                       ("occluded", lambda e: L.hipptOccluded(rays, n, flags, occ, e)),
                       ("camera", lambda e: L.hipptTraceCamera(0, flags, t, prim, e))):
        e = ctypes.c_char_p()
        ok = call(ctypes.byref(e))
        out.append((name, bool(ok), e.value.decode() if e.value else ""))
    return out


def test_argument_errors_return_false_with_a_message(lib):
    rays = np.zeros((4, 8), np.float32)
    t, prim, occ = np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    R, T, P, O = rays.ctypes.data, t.ctypes.data, prim.ctypes.data, occ.ctypes.data
    pt = hippt.PathTracer()
    # the built-in scene has nothing to query
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    for name, ok, msg in _calls(lib, R, 4, T, P, O):
        assert not ok and "scene" in msg, (name, msg)
    # a mesh, but no Init
    pt.uploadMesh(scenes.cornell34())
    for name, ok, msg in _calls(lib, R, 4, T, P, O):
        assert not ok and "not initialized" in msg, (name, msg)
    for name, ok, msg in _calls(lib, R, 4, T, P, O, flags=hippt.RAYS_DEVICE):
        assert not ok and "not initialized" in msg, (name, msg)
    # numRays < 0; null rays with numRays > 0; no output at all (these come before the Init check)
    for name, ok, msg in _calls(lib, R, -1, T, P, O)[:2]:
        assert not ok and "negative" in msg, (name, msg)
    for name, ok, msg in _calls(lib, None, 4, T, P, O)[:2]:
        assert not ok and "null" in msg, (name, msg)
    for name, ok, msg in _calls(lib, R, 4, None, None, None):
        assert not ok and "output" in msg, (name, msg)
    # one of t / prim alone is enough to get past the output check
    for name, ok, msg in _calls(lib, R, 4, T, None, O) + _calls(lib, R, 4, None, P, O):
        assert not ok and "not initialized" in msg, (name, msg)
    e = ctypes.c_char_p()
    assert not lib.hipptTraceCamera(-1, 0, T, P, ctypes.byref(e)) and e.value
    # a null message pointer is allowed, and the message is also hipptLastError's
    assert not lib.hipptTraceRays(R, 4, 0, T, P, None)
    assert b"not initialized" in lib.hipptLastError()


@pytest.mark.parametrize("bad,what", [
    (np.zeros((4, 7), np.float32), "shape"),
    (np.zeros(32, np.float32), "shape"),
    (np.zeros((2, 4, 8), np.float32), "shape"),
    (np.zeros((4, 8), np.float64), "float32"),
    (np.zeros((4, 8), np.int32), "float32"),
    (np.zeros((4, 16), np.float32)[:, ::2], "contiguous"),
    ([[0.0] * 8], "numpy"),
])
def test_wrapper_rejects_a_bad_ray_batch_before_any_call(lib, bad, what):
    pt = hippt.PathTracer()
    pt.uploadMesh(scenes.cornell34())
    for fn in (pt.traceRays, pt.occluded):
        with pytest.raises(hippt.HipptError, match=what):
            fn(bad)
    # a well-formed batch gets as far as the library, which reports the missing Init
    with pytest.raises(hippt.HipptError, match="not initialized"):
        pt.traceRays(np.zeros((4, 8), np.float32))
    with pytest.raises(hippt.HipptError, match="not initialized"):
        pt.traceCamera()


def test_wrapper_takes_a_cpu_tensor_as_numpy(lib):
    torch = pytest.importorskip("torch")
    pt = hippt.PathTracer()
    pt.uploadMesh(scenes.cornell34())
    with pytest.raises(hippt.HipptError, match="float32"):
        pt.traceRays(torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(hippt.HipptError, match="shape"):
        pt.occluded(torch.zeros(8, dtype=torch.float32))
    with pytest.raises(hippt.HipptError, match="contiguous"):
        pt.traceRays(torch.zeros(4, 16, dtype=torch.float32)[:, ::2])
    with pytest.raises(hippt.HipptError, match="not initialized"):
        pt.traceRays(torch.zeros(4, 8, dtype=torch.float32))
