"""Python host mirror of the reference backend interface, over libhippt.so (C ABI).

``PathTracer`` mirrors ``CudaPathTracer`` (CudaPathTracer.h:6-23 / .cpp:14-94): the same
methods (initialize, renderFrame, hostPixels, frameIndex, lastError), the same frame-index
bookkeeping (renderFrame passes the current index and increments it after success,
CudaPathTracer.cpp:41-57) and the same error behaviour (False + lastError()).  Extensions
(scene upload, batched frames, devices, row bands, counters) wrap the hippt* entry points
of include/hippt.h.

The product path is libhippt.so only: if it is missing the import fails loudly — there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

from . import scenes  # noqa: F401  (re-export)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libhippt.so")

SCENE_SPHERE4 = 0
SCENE_MESH = 1

# hipptMaterial kinds (include/hippt.h); MAT_EMISSIVE: albedo holds the emitted radiance
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_EMISSIVE = 0, 1, 2, 3

OPT_COUNT_TRAVERSAL = 1
OPT_WAVE_THRESHOLD = 2
OPT_SCRATCH_MB = 3
OPT_CHUNK = 4
OPT_BLOCKS_PER_CU = 5
OPT_LDS_SCENE = 6
OPT_PATH_MODE = 8
OPT_WAVEFRONT_SLOTS = 9
OPT_BVH_LEAF = 10
OPT_BVH_TRAVERSAL_COST = 11
OPT_BVH_MAX_DEPTH = 12
OPT_DEVICE_ROWS = 13
OPT_LEAF_EXIT = 14
OPT_NODE_EXIT = 15
OPT_BVH_SAH = 16
OPT_BVH_WIDTH = 17
OPT_STACK_CAP = 18
OPT_BVH_QUANT = 19
OPT_LDS_TOP_NODES = 20
OPT_BVH_COLLAPSE = 21
OPT_BVH_NODE_COST = 22
OPT_BVH_LEAF4 = 23
OPT_RNG_TABLE = 24
OPT_CAMERA_POOL = 26
OPT_FUSE_COMBINE = 27
OPT_ITEM_ORDER = 28
OPT_WAVEFRONT_SORT = 29
OPT_CHAIN = 30
OPT_CHAIN_AUDIT = 31
OPT_PIXEL_TILE = 32
OPT_QUERY_SLICE = 33
OPT_RENDER_PAD = 34
OPT_SKY_RECT = 35
OPT_DENOISE_TIMING = 36
OPT_LIGHT_SAMPLING = 37  # next-event estimation at Lambertian vertices (include/hippt.h; 0 default)
OPT_LIGHT_SAMPLING_MODE = 38  # the same word with all its values: 0, 1 and LIGHT_SAMPLING_MIS (37 takes 0 and 1 only)
LIGHT_SAMPLING_MIS = 2  # light sampling with MIS (the power heuristic with the scatter sample)
OPT_LIGHT_SELECT = 39  # how a connection picks its light: 0 (default) uniformly, LIGHT_SELECT_POWER by area x emission
LIGHT_SELECT_POWER = 1
OPT_ENV_SAMPLING = 40  # connect every Lambertian vertex to the environment map by its selection table: 0 (default), 1
OPT_SKY_COMBINE = 41  # sky-certain runs finished by the combine: -1 (default) automatic, 0 off (include/hippt.h)
OPT_PIXEL_FORMAT = 25
PIXEL_ARGB = 0
PIXEL_RGBA8 = 1
INFO_LDS_TOP_BYTES = 100
INFO_BLOCKS_PER_CU = 101
INFO_CHUNK = 102
INFO_CHAIN_CAP = 103
INFO_UPDATE_DROPPED = 104
INFO_RENDER_PAD = 105
INFO_SKY_RECT_PIXELS = 106
INFO_LIGHTS = 107  # emissive primitives in the uploaded scene
INFO_LIGHT_SAMPLING = 108  # OPT_LIGHT_SAMPLING_MODE's value (1 or 2) if the last render took the light-sampling route
INFO_LIGHT_SELECT = 109  # OPT_LIGHT_SELECT's value if the last render took the light-sampling route and applied it
INFO_ENVIRONMENT = 110  # the environment's size as the last render applied it (0: the gradient, or the built-in scene)
INFO_ENV_SAMPLING = 111  # 1 if the last render applied OPT_ENV_SAMPLING
INFO_SKY_COMBINE = 112  # band pixels of the last batch whose samples the combine finished (0: OPT_SKY_COMBINE off)
INFO_DENOISE_NS = 200
RAYS_DEVICE = 1
HIT_SPHERE = 1 << 30
HIT_BACKFACE = -(1 << 31)  # the int's sign bit
HIT_MATERIAL_MASK = (1 << 30) - 1
DENOISE_NO_DEMODULATE = 1
DENOISE_DEVICE = 2
DENOISE_STAGES = ("guides", "prepare", "pass0", "pass1", "pass2", "pass3", "pass4", "pass5", "pass6", "pass7", "finish")
VERTS_DEVICE = 1
ENV_DEVICE = 1
ENV_MAX_SIZE = 4096
SCENE_NODES2 = 0
SCENE_NODES4 = 1
SCENE_PRIMS = 2
SCENE_SHADE = 3
SCENE_LIGHTS = 4  # the light selection table: (prim, q, c, bits of ip) per light
SCENE_ENVIRONMENT = 5  # the environment's texels: (r, g, b, 0) float32 per texel
SCENE_ENV_TABLE = 6  # the environment's selection table: S rows (m, C), then S x S texels (q, c, bits of k)

# Every symbol include/hippt.h declares (checked by tests/test_abi_cpu.py).
EXPORTS = (
    "cudaPathTracerInit", "cudaPathTracerRender", "cudaPathTracerShutdown",
    "hipPathTracerInit", "hipPathTracerRender", "hipPathTracerShutdown",
    "hipptBuildCamera", "hipptUseBuiltinScene", "hipptUploadMesh", "hipptUploadScene", "hipptReadMesh",
    "hipptFreeMesh", "hipptSetCamera",
    "hipptDeviceCount", "hipptSetDevices", "hipptSetRowRange", "hipptSetRowInterleave",
    "hipptRenderFrames", "hipptRenderFramesAsync", "hipptSynchronize", "hipptRenderFramesPresent",
    "hipptLatestFrame", "hipptReadback",
    "hipptResetAccumulation", "hipptGetStats", "hipptResetStats", "hipptGetCounters", "hipptSetOption",
    "hipptGetOption",
    "hipptLastError", "hipptBvhBuild", "hipptBvhNodeCount", "hipptBvhDepth", "hipptBvhCopy", "hipptBvhFree",
    "hipptBvh4NodeCount", "hipptBvh4Depth", "hipptBvh4StackBound", "hipptBvh4Copy", "hipptBvh4QCopy", "hipptBvh4QNodeCount",
    "hipptActiveBvhWidth", "hipptChainAudit",
    "hipptTraceRays", "hipptOccluded", "hipptTraceCamera", "hipptTraceHits", "hipptTraceCameraHits",
    "hipptUpdateVertices", "hipptSceneDownload", "hipptBvhRefit",
    "hipptDenoiseDefaults", "hipptDenoise",
    "hipptTraceRadiance", "hipptCameraRays",
    "hipptSetEnvironment", "hipptEnvLookup", "hipptEnvDirections", "hipptEnvFromEquirect",
)


class HipptError(RuntimeError):
    pass


class Camera(ctypes.Structure):
    """hipptCamera (include/hippt.h), 80 bytes."""
    _fields_ = [("origin", ctypes.c_float * 3), ("llc", ctypes.c_float * 3), ("horizontal", ctypes.c_float * 3),
                ("vertical", ctypes.c_float * 3), ("u", ctypes.c_float * 3), ("v", ctypes.c_float * 3),
                ("lens_radius", ctypes.c_float), ("reserved", ctypes.c_float)]

    def as_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self), dtype=np.float32).copy()


class Mesh(ctypes.Structure):
    """hipptMesh (include/hippt.h)."""
    _fields_ = [("verts", ctypes.POINTER(ctypes.c_float)), ("triGroup", ctypes.POINTER(ctypes.c_int)),
                ("numTris", ctypes.c_int), ("numGroups", ctypes.c_int),
                ("groupNames", ctypes.POINTER(ctypes.c_char_p)), ("owner_", ctypes.c_void_p)]


class Hit(ctypes.Structure):
    """hipptHit (include/hippt.h), 32 bytes."""
    _fields_ = [("t", ctypes.c_float), ("prim", ctypes.c_int), ("normal", ctypes.c_float * 3),
                ("u", ctypes.c_float), ("v", ctypes.c_float), ("matFlags", ctypes.c_int)]


# hipptHit as a numpy record: what traceHits / traceCameraHits return for numpy rays
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("normal", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"),
                      ("matFlags", "<i4")])


def split_hits(hits) -> dict:
    """Views of the (..., 8) float32 tensor traceHits returns for device rays, by hipptHit's fields: t
    (...,) float32, prim (...,) int32, normal (..., 3), u, v, matFlags (...,) int32.  No copy: the
    integer fields are the same bytes seen as int32."""
    import torch
    return {"t": hits[..., 0], "prim": hits[..., 1].view(torch.int32), "normal": hits[..., 2:5],
            "u": hits[..., 5], "v": hits[..., 6], "matFlags": hits[..., 7].view(torch.int32)}


class DenoiseParams(ctypes.Structure):
    """hipptDenoiseParams (include/hippt.h), 32 bytes."""
    _fields_ = [("passes", ctypes.c_int), ("guideFrame", ctypes.c_int), ("normalPower", ctypes.c_int),
                ("flags", ctypes.c_int), ("sigmaColor", ctypes.c_float), ("sigmaDepth", ctypes.c_float),
                ("reserved", ctypes.c_float * 2)]


class Stats(ctypes.Structure):
    _fields_ = [("segments", ctypes.c_ulonglong), ("pixelSamples", ctypes.c_ulonglong),
                ("nodeVisits", ctypes.c_ulonglong), ("triTests", ctypes.c_ulonglong),
                ("traceMs", ctypes.c_double), ("combineMs", ctypes.c_double),
                ("traceLaunches", ctypes.c_int), ("combineLaunches", ctypes.c_int),
                ("bvhNodes", ctypes.c_int), ("bvhDepth", ctypes.c_int), ("numTris", ctypes.c_int),
                ("numDevices", ctypes.c_int)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib: Optional[ctypes.CDLL] = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Loads libhippt.so (or $HIPPT_LIB, for build-variant experiments) and declares the C
    signatures.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("HIPPT_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise HipptError(f"{path} is missing: build it with `make -C qt-raytracer_amd` "
                         "(or __graft_entry__.build()); there is no fallback path")
    lib = ctypes.CDLL(path)
    c_int, c_bool, c_char_p, c_double, c_float = ctypes.c_int, ctypes.c_bool, ctypes.c_char_p, ctypes.c_double, ctypes.c_float
    pp_char = ctypes.POINTER(ctypes.c_char_p)
    p_uint = ctypes.POINTER(ctypes.c_uint)
    pp_uint = ctypes.POINTER(p_uint)
    p_float = ctypes.POINTER(ctypes.c_float)
    p_int = ctypes.POINTER(ctypes.c_int)
    p_double = ctypes.POINTER(ctypes.c_double)

    variant = bool(os.environ.get("HIPPT_LIB"))  # an older build under test may lack newer entry points

    def sig(name, res, *args):
        if variant and not hasattr(lib, name):
            return
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = list(args)

    for pre in ("cuda", "hip"):
        sig(f"{pre}PathTracerInit", c_bool, c_int, c_int, pp_char)
        sig(f"{pre}PathTracerRender", c_bool, c_int, c_int, pp_uint, pp_char)
        sig(f"{pre}PathTracerShutdown", None)
    sig("hipptBuildCamera", None, p_double, p_double, p_double, c_double, c_double, c_double, c_double,
        ctypes.POINTER(Camera))
    sig("hipptUseBuiltinScene", c_bool, c_int, pp_char)
    sig("hipptUploadMesh", c_bool, p_float, p_int, c_int, p_float, c_int, p_double, p_double, p_double,
        c_double, c_double, c_double, pp_char)
    sig("hipptUploadScene", c_bool, p_float, p_int, c_int, p_float, p_int, c_int, ctypes.c_void_p, c_int, p_double,
        p_double, p_double, c_double, c_double, c_double, pp_char)
    sig("hipptReadMesh", c_bool, c_char_p, ctypes.POINTER(Mesh), pp_char)
    sig("hipptFreeMesh", None, ctypes.POINTER(Mesh))
    sig("hipptSetCamera", c_bool, ctypes.POINTER(Camera), pp_char)
    sig("hipptDeviceCount", c_int)
    sig("hipptSetDevices", c_bool, p_int, c_int, pp_char)
    sig("hipptSetRowRange", c_bool, c_int, c_int, pp_char)
    sig("hipptSetRowInterleave", c_bool, c_int, c_int, pp_char)
    sig("hipptRenderFrames", c_bool, c_int, c_int, c_int, pp_uint, pp_char)
    sig("hipptRenderFramesAsync", c_bool, c_int, c_int, c_int, pp_char)
    sig("hipptSynchronize", c_bool, pp_char)
    sig("hipptRenderFramesPresent", c_bool, c_int, c_int, c_int, pp_char)
    sig("hipptLatestFrame", c_bool, pp_uint, ctypes.POINTER(c_int), pp_char)
    sig("hipptReadback", c_bool, p_uint, p_float, pp_char)
    sig("hipptResetAccumulation", c_bool, pp_char)
    sig("hipptGetStats", c_bool, ctypes.POINTER(Stats))
    sig("hipptResetStats", None)
    sig("hipptGetCounters", c_int, ctypes.POINTER(ctypes.c_ulonglong), c_int)
    sig("hipptSetOption", c_bool, c_int, ctypes.c_longlong)
    sig("hipptGetOption", ctypes.c_longlong, c_int)
    sig("hipptLastError", c_char_p)
    sig("hipptBvhBuild", ctypes.c_void_p, p_float, c_int, c_float, pp_char)
    sig("hipptBvhNodeCount", c_int, ctypes.c_void_p)
    sig("hipptBvhDepth", c_int, ctypes.c_void_p)
    sig("hipptBvhCopy", None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), p_int)
    sig("hipptBvhFree", None, ctypes.c_void_p)
    sig("hipptActiveBvhWidth", c_int)
    sig("hipptBvh4NodeCount", c_int, ctypes.c_void_p)
    sig("hipptBvh4Depth", c_int, ctypes.c_void_p)
    sig("hipptBvh4StackBound", c_int, ctypes.c_void_p)
    sig("hipptBvh4Copy", None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32))
    sig("hipptBvh4QCopy", None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32))
    sig("hipptBvh4QNodeCount", c_int, ctypes.c_void_p)
    sig("hipptChainAudit", c_int, p_uint, c_int)
    # ray queries: the buffers as addresses (host arrays or device memory, by the flags)
    c_void_p = ctypes.c_void_p
    sig("hipptTraceRays", c_bool, c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, pp_char)
    sig("hipptOccluded", c_bool, c_void_p, ctypes.c_longlong, c_int, c_void_p, pp_char)
    sig("hipptTraceCamera", c_bool, c_int, c_int, c_void_p, c_void_p, pp_char)
    sig("hipptTraceHits", c_bool, c_void_p, ctypes.c_longlong, c_int, c_void_p, pp_char)
    sig("hipptTraceCameraHits", c_bool, c_int, c_int, c_void_p, pp_char)
    sig("hipptTraceRadiance", c_bool, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p, c_void_p, pp_char)
    sig("hipptCameraRays", c_bool, c_int, c_int, c_void_p, c_void_p, pp_char)
    sig("hipptUpdateVertices", c_bool, c_void_p, c_int, c_int, pp_char)
    sig("hipptSceneDownload", ctypes.c_longlong, c_int, c_void_p, ctypes.c_longlong, pp_char)
    sig("hipptBvhRefit", c_bool, c_void_p, p_float, c_int, c_float, pp_char)
    sig("hipptDenoiseDefaults", None, ctypes.POINTER(DenoiseParams))
    sig("hipptDenoise", c_bool, ctypes.POINTER(DenoiseParams), c_void_p, c_void_p, pp_char)
    sig("hipptSetEnvironment", c_bool, c_void_p, c_int, c_int, pp_char)
    sig("hipptEnvLookup", c_bool, c_void_p, ctypes.c_longlong, c_void_p, pp_char)
    sig("hipptEnvDirections", None, c_int, c_void_p)
    sig("hipptEnvFromEquirect", c_bool, c_void_p, c_int, c_int, c_int, c_void_p, pp_char)
    _lib = lib
    return lib


def _err(e: ctypes.c_char_p, default: str) -> str:
    return e.value.decode() if e.value else default


def _ptr(a: np.ndarray, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def _d3(v) -> ctypes.Array:
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _is_tensor(a) -> bool:
    """A torch tensor, without importing torch for callers that never pass one."""
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


def _query_rays(rays):
    """Validates a ray batch before any call: (N, 8) float32, C-contiguous; a numpy array (a CPU tensor
    is taken as one) or a tensor on the ROCm device.  Returns (array or tensor, on_device)."""
    if _is_tensor(rays):
        import torch
        if rays.dtype != torch.float32:
            raise HipptError(f"rays must be float32, not {rays.dtype}")
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise HipptError(f"rays must have shape (N, 8), not {tuple(rays.shape)}")
        if not rays.is_contiguous():
            raise HipptError("rays must be contiguous")
        if rays.device.type == "cpu":
            return rays.numpy(), False
        if rays.device.type != "cuda":
            raise HipptError(f"rays on an unsupported device {rays.device}")
        return rays, True
    if not isinstance(rays, np.ndarray):
        raise HipptError("rays must be a numpy array or a torch tensor")
    if rays.dtype != np.float32:
        raise HipptError(f"rays must be float32, not {rays.dtype}")
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise HipptError(f"rays must have shape (N, 8), not {rays.shape}")
    if not rays.flags["C_CONTIGUOUS"]:
        raise HipptError("rays must be contiguous")
    return rays, False


def path_seeds(n: int, frame: int = 0, like=None):
    """The renderer's pixel_seed of items 0..n-1 for sample `frame`: i * 9781 + (frame + 1) * 6271 mod
    2^32, the RNG state traceRadiance starts path i with by default.  numpy uint32 (n,); with a tensor
    `like` on the ROCm device, an int32 tensor of the same bits on that device."""
    seeds = (np.arange(int(n), dtype=np.uint64) * 9781 + (int(frame) + 1) * 6271).astype(np.uint32)
    if like is not None and _is_tensor(like) and like.device.type != "cpu":
        import torch
        return torch.from_numpy(seeds.view(np.int32)).to(like.device)
    return seeds


def _path_seeds_arg(seeds, n: int, rays, dev: bool):
    """Validates the seeds of a path query against its rays: (N,) int32 or uint32 state bits, where the
    rays are.  Returns the array or tensor to pass."""
    if seeds is None:
        return path_seeds(n, 0, rays if dev else None)
    if _is_tensor(seeds):
        import torch
        ok = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
        if seeds.dtype not in ok:
            raise HipptError(f"seeds must be int32 or uint32, not {seeds.dtype}")
        if seeds.dim() != 1 or seeds.shape[0] != n or not seeds.is_contiguous():
            raise HipptError(f"seeds must be contiguous with shape ({n},), not {tuple(seeds.shape)}")
        if seeds.device.type == "cpu":
            seeds = seeds.numpy()
        elif not dev or seeds.device != rays.device:
            raise HipptError("seeds must be where the rays are")
        else:
            return seeds
    if not isinstance(seeds, np.ndarray):
        raise HipptError("seeds must be a numpy array or a torch tensor")
    if dev:
        raise HipptError("seeds must be where the rays are")
    if seeds.dtype not in (np.int32, np.uint32):
        raise HipptError(f"seeds must be int32 or uint32, not {seeds.dtype}")
    if seeds.shape != (n,) or not seeds.flags["C_CONTIGUOUS"]:
        raise HipptError(f"seeds must be contiguous with shape ({n},), not {seeds.shape}")
    return seeds


def _update_verts(verts):
    """Validates new vertices before any call: (n, 9) float32, C-contiguous; a numpy array (a CPU tensor
    is taken as one) or a tensor on the ROCm device.  Returns (array or tensor, on_device)."""
    if _is_tensor(verts):
        import torch
        if verts.dtype != torch.float32:
            raise HipptError(f"verts must be float32, not {verts.dtype}")
        if verts.dim() != 2 or verts.shape[1] != 9:
            raise HipptError(f"verts must have shape (n, 9), not {tuple(verts.shape)}")
        if not verts.is_contiguous():
            raise HipptError("verts must be contiguous")
        if verts.device.type == "cpu":
            return verts.numpy(), False
        if verts.device.type != "cuda":
            raise HipptError(f"verts on an unsupported device {verts.device}")
        return verts, True
    if not isinstance(verts, np.ndarray):
        raise HipptError("verts must be a numpy array or a torch tensor")
    if verts.dtype != np.float32:
        raise HipptError(f"verts must be float32, not {verts.dtype}")
    if verts.ndim != 2 or verts.shape[1] != 9:
        raise HipptError(f"verts must have shape (n, 9), not {verts.shape}")
    if not verts.flags["C_CONTIGUOUS"]:
        raise HipptError("verts must be contiguous")
    return verts, False


_SCENE_WORDS = {SCENE_NODES2: 16, SCENE_NODES4: 32, SCENE_PRIMS: 12, SCENE_SHADE: 4, SCENE_LIGHTS: 4,
                SCENE_ENVIRONMENT: 4, SCENE_ENV_TABLE: 1}
ENV_ROW_DTYPE = np.dtype([("m", "<u4"), ("C", "<u4")])
ENV_TEXEL_DTYPE = np.dtype([("q", "<u4"), ("c", "<u4"), ("k", "<f4")])
LIGHT_TABLE_DTYPE = np.dtype([("prim", "<i4"), ("q", "<u4"), ("c", "<u4"), ("ip", "<f4")])


def scene_download(what: int) -> np.ndarray:
    """hipptSceneDownload: context 0's device copy of the 2-wide nodes (N, 16), the 4-wide float nodes
    (M, 32; interior child codes are byte offsets), the primitive records (P, 12; leaf order, id in
    word 9), the shading records (P, 4) or the light selection table (L, 4; PathTracer.lightTable names its
    words) or the environment's texels (S*S, 4: the bits of r, g, b and a zero word), as uint32, after the queued
    work."""
    if what not in _SCENE_WORDS:
        raise HipptError(f"unknown scene buffer {what}")
    lib = load_library()
    e = ctypes.c_char_p()
    need = lib.hipptSceneDownload(int(what), None, 0, ctypes.byref(e))
    if need < 0:
        raise HipptError(_err(e, "scene download failed"))
    out = np.zeros(need // 4, np.uint32)
    if lib.hipptSceneDownload(int(what), out.ctypes.data, need, ctypes.byref(e)) < 0:
        raise HipptError(_err(e, "scene download failed"))
    return out.reshape(-1, _SCENE_WORDS[what])


def _env_size(size) -> int:
    size = int(size)
    if not 1 <= size <= ENV_MAX_SIZE:
        raise HipptError(f"environment size must be in 1..{ENV_MAX_SIZE}, not {size}")
    return size


def env_directions(size: int) -> np.ndarray:
    """hipptEnvDirections: the unit directions (S, S, 3) float32 of the texel centres of an S x S environment
    map, [y, x] as the texels are indexed (+y up; the upper hemisphere is the inner diamond)."""
    size = _env_size(size)
    out = np.zeros((size, size, 3), np.float32)
    load_library().hipptEnvDirections(size, out.ctypes.data)
    return out


def env_from_equirect(img, size: int) -> np.ndarray:
    """hipptEnvFromEquirect: the (S, S, 3) float32 environment map of a lat-long image (H, W, 3) float32 (row 0
    at +y), sampled bilinearly, in double, at the texel-centre directions; no prefilter."""
    size = _env_size(size)
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise HipptError(f"the image must have shape (H, W, 3), not {img.shape}")
    out = np.zeros((size, size, 3), np.float32)
    e = ctypes.c_char_p()
    if not load_library().hipptEnvFromEquirect(img.ctypes.data, int(img.shape[1]), int(img.shape[0]), size,
                                               out.ctypes.data, ctypes.byref(e)):
        raise HipptError(_err(e, "environment resampling failed"))
    return out


def env_lookup(dirs) -> np.ndarray:
    """hipptEnvLookup: env(d) of the library's host copy of the environment for directions (..., 3) float32 of any
    length, by the text the kernels compile; float32, the shape of `dirs`.  Raises without an environment."""
    d = np.ascontiguousarray(dirs, np.float32)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise HipptError(f"directions must have shape (..., 3), not {d.shape}")
    out = np.zeros(d.shape, np.float32)
    e = ctypes.c_char_p()
    if not load_library().hipptEnvLookup(d.ctypes.data, d.size // 3, out.ctypes.data, ctypes.byref(e)):
        raise HipptError(_err(e, "environment lookup failed"))
    return out


def read_mesh(path: str):
    """hipptReadMesh: (verts (n, 9) float32, tri_group (n,) int32, group names) of an OBJ/PLY file."""
    lib = load_library()
    m = Mesh()
    e = ctypes.c_char_p()
    if not lib.hipptReadMesh(os.fsencode(path), ctypes.byref(m), ctypes.byref(e)):
        raise HipptError(_err(e, f"cannot read {path}"))
    try:
        n = m.numTris
        verts = np.ctypeslib.as_array(m.verts, shape=(n * 9,)).reshape(n, 9).copy()
        groups = np.ctypeslib.as_array(m.triGroup, shape=(n,)).copy()
        names = [m.groupNames[g].decode() for g in range(m.numGroups)]
    finally:
        lib.hipptFreeMesh(ctypes.byref(m))
    return verts, groups, names


def build_camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus) -> Camera:
    lib = load_library()
    cam = Camera()
    lib.hipptBuildCamera(_d3(lookfrom), _d3(lookat), _d3(vup), float(vfov), float(aspect), float(aperture),
                         float(focus), ctypes.byref(cam))
    return cam


class Bvh:
    """Host BVH built by libhippt (hipptBvhBuild): nodes (N,16) uint32 and triangle order; the
    4-wide tree collapsed from it: nodes4 (M,32) uint32, depth4, stack_bound4."""

    def __init__(self, verts: np.ndarray, extent_hint: float = 0.0):
        lib = load_library()
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        e = ctypes.c_char_p()
        self._h = lib.hipptBvhBuild(_ptr(v, ctypes.c_float), int(v.shape[0]), float(extent_hint), ctypes.byref(e))
        if not self._h:
            raise HipptError(_err(e, "BVH build failed"))
        self._tris = int(v.shape[0])
        self._extent = float(extent_hint)
        self._read()

    def _read(self) -> None:
        lib, h = load_library(), self._h
        n = lib.hipptBvhNodeCount(h)
        self.depth = lib.hipptBvhDepth(h)
        self.nodes = np.zeros((n, 16), dtype=np.uint32)
        self.order = np.zeros(self._tris, dtype=np.int32)
        lib.hipptBvhCopy(h, _ptr(self.nodes, ctypes.c_uint32), _ptr(self.order, ctypes.c_int))
        self.depth4 = lib.hipptBvh4Depth(h)
        self.stack_bound4 = lib.hipptBvh4StackBound(h)
        self.nodes4 = np.zeros((lib.hipptBvh4NodeCount(h), 32), dtype=np.uint32)
        lib.hipptBvh4Copy(h, _ptr(self.nodes4, ctypes.c_uint32))
        self.nodes4q = np.zeros((lib.hipptBvh4QNodeCount(h), 16), dtype=np.uint32)
        lib.hipptBvh4QCopy(h, _ptr(self.nodes4q, ctypes.c_uint32))

    def refit(self, verts: np.ndarray, extent_hint: Optional[float] = None) -> None:
        """hipptBvhRefit: new boxes for the same topology (nodes, nodes4, nodes4q are read again; codes
        and order stay).  extent_hint defaults to the build's.  Raises and leaves the trees unchanged
        on a count mismatch or a non-finite coordinate."""
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        e = ctypes.c_char_p()
        hint = self._extent if extent_hint is None else float(extent_hint)
        if not load_library().hipptBvhRefit(self._h, _ptr(v, ctypes.c_float), int(v.shape[0]), hint, ctypes.byref(e)):
            raise HipptError(_err(e, "BVH refit failed"))
        self._read()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                load_library().hipptBvhFree(self._h)
                self._h = None
        except Exception:
            pass


class PathTracer:
    """Mirror of CudaPathTracer (CudaPathTracer.h:6-23) over the HIP backend."""

    def __init__(self):
        self._lib = load_library()
        self._width = 0
        self._height = 0
        self._frame_index = 0
        self._pixels: Optional[ctypes.POINTER] = None
        self._last_error = ""
        self._albedo: Optional[np.ndarray] = None  # (materials, 3) of the scene uploaded last (gbuffer)
        self._devices: list = []  # of the last setDevices (denoise: where its tensors go)

    def __del__(self):  # ~CudaPathTracer -> cudaPathTracerShutdown (CudaPathTracer.cpp:14-18)
        try:
            self._lib.cudaPathTracerShutdown()
        except Exception:
            pass

    # --- CudaPathTracer interface -------------------------------------------------------------
    def initialize(self, width: int, height: int) -> bool:
        self._width, self._height = int(width), int(height)
        self._frame_index = 0
        self._pixels = None
        e = ctypes.c_char_p()
        if not self._lib.cudaPathTracerInit(self._width, self._height, ctypes.byref(e)):
            self._last_error = _err(e, "HIP initialization failed")
            return False
        return True

    def renderFrame(self, maxDepth: int) -> bool:  # noqa: N802 (reference name)
        e = ctypes.c_char_p()
        px = ctypes.POINTER(ctypes.c_uint)()
        if not self._lib.cudaPathTracerRender(self._frame_index, int(maxDepth), ctypes.byref(px), ctypes.byref(e)):
            self._last_error = _err(e, "HIP render failed")
            return False
        self._pixels = px
        self._frame_index += 1
        return True

    def hostPixels(self) -> Optional[np.ndarray]:  # noqa: N802
        """Copy of the library-owned W*H ARGB frame (row 0 = v = 0), or None before a render."""
        if not self._pixels:
            return None
        n = self._width * self._height
        return np.ctypeslib.as_array(self._pixels, shape=(n,)).reshape(self._height, self._width).copy()

    def frameIndex(self) -> int:  # noqa: N802
        return self._frame_index

    def lastError(self) -> str:  # noqa: N802
        return self._last_error

    # --- GpuPathTracer-shaped extensions (GpuPathTracer.h:9-38) -------------------------------
    def renderFrames(self, samplesPerFrame: int, maxDepth: int, copy: bool = True) -> bool:  # noqa: N802
        """Renders samplesPerFrame frames at once, continuing the frame index."""
        e = ctypes.c_char_p()
        px = ctypes.POINTER(ctypes.c_uint)()
        ok = self._lib.hipptRenderFrames(self._frame_index, int(samplesPerFrame), int(maxDepth),
                                         ctypes.byref(px) if copy else None, ctypes.byref(e))
        if not ok:
            self._last_error = _err(e, "HIP render failed")
            return False
        if copy:
            self._pixels = px
        self._frame_index += int(samplesPerFrame)
        return True

    def renderFramesAsync(self, samplesPerFrame: int, maxDepth: int) -> bool:  # noqa: N802
        e = ctypes.c_char_p()
        if not self._lib.hipptRenderFramesAsync(self._frame_index, int(samplesPerFrame), int(maxDepth), ctypes.byref(e)):
            self._last_error = _err(e, "HIP render failed")
            return False
        self._frame_index += int(samplesPerFrame)
        return True

    def renderFramesPresent(self, samplesPerFrame: int, maxDepth: int) -> bool:  # noqa: N802
        """Enqueues frames plus a copy into the next pinned hand-off frame; does not wait."""
        e = ctypes.c_char_p()
        if not self._lib.hipptRenderFramesPresent(self._frame_index, int(samplesPerFrame), int(maxDepth),
                                                  ctypes.byref(e)):
            self._last_error = _err(e, "HIP render failed")
            return False
        self._frame_index += int(samplesPerFrame)
        return True

    def latestFrame(self):  # noqa: N802
        """Non-blocking: (ARGB (H, W) copy or None, frames accumulated in it)."""
        e = ctypes.c_char_p()
        px = ctypes.POINTER(ctypes.c_uint)()
        n = ctypes.c_int()
        if not self._lib.hipptLatestFrame(ctypes.byref(px), ctypes.byref(n), ctypes.byref(e)):
            raise HipptError(_err(e, "latest frame failed"))
        if not px:
            return None, 0
        h, w = self._height, self._width
        return np.ctypeslib.as_array(px, shape=(h * w,)).reshape(h, w).copy(), n.value

    def synchronize(self) -> bool:
        e = ctypes.c_char_p()
        if not self._lib.hipptSynchronize(ctypes.byref(e)):
            self._last_error = _err(e, "HIP synchronize failed")
            return False
        return True

    def resetAccumulation(self) -> bool:  # noqa: N802
        e = ctypes.c_char_p()
        if not self._lib.hipptResetAccumulation(ctypes.byref(e)):
            self._last_error = _err(e, "reset failed")
            return False
        self._frame_index = 0
        return True

    def readback(self, y0: int = 0, y1: Optional[int] = None):
        """(pixels (H,W) uint32, accum (H,W,4) float32) of the current image; rows outside this
        process's row range are zero."""
        pixels = np.zeros((self._height, self._width), dtype=np.uint32)
        accum = np.zeros((self._height, self._width, 4), dtype=np.float32)
        e = ctypes.c_char_p()
        if not self._lib.hipptReadback(_ptr(pixels, ctypes.c_uint), _ptr(accum, ctypes.c_float), ctypes.byref(e)):
            raise HipptError(_err(e, "readback failed"))
        y1 = self._height if y1 is None else y1
        return pixels[y0:y1], accum[y0:y1]

    # --- scene / devices / counters -------------------------------------------------------------
    def useBuiltinScene(self, scene_id: int = SCENE_SPHERE4) -> None:  # noqa: N802
        e = ctypes.c_char_p()
        if not self._lib.hipptUseBuiltinScene(int(scene_id), ctypes.byref(e)):
            raise HipptError(_err(e, "bad scene"))

    def uploadScene(self, scene) -> None:  # noqa: N802
        """hipptUploadScene: triangles + spheres + materials (hippt.scenes.Scene)."""
        v = np.ascontiguousarray(scene.verts, dtype=np.float32).reshape(-1, 9)
        m = np.ascontiguousarray(scene.tri_mat, dtype=np.int32)
        sp = np.ascontiguousarray(scene.spheres, dtype=np.float32).reshape(-1, 4)
        sm = np.ascontiguousarray(scene.sph_mat, dtype=np.int32)
        mats = np.ascontiguousarray(scene.materials())
        e = ctypes.c_char_p()
        ok = self._lib.hipptUploadScene(_ptr(v, ctypes.c_float), _ptr(m, ctypes.c_int), int(v.shape[0]),
                                        _ptr(sp, ctypes.c_float), _ptr(sm, ctypes.c_int), int(sp.shape[0]),
                                        mats.ctypes.data_as(ctypes.c_void_p), int(mats.shape[0]),
                                        _d3(scene.lookfrom), _d3(scene.lookat), _d3(scene.vup), float(scene.vfov),
                                        float(scene.aperture), float(scene.focus), ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "scene upload failed"))
        self._albedo = np.array(mats["albedo"], np.float32).reshape(-1, 3)

    def uploadMesh(self, scene) -> None:  # noqa: N802
        """hipptUploadMesh for Lambertian triangle scenes; other scenes go through uploadScene."""
        if not getattr(scene, "lambertian_triangles", True):
            return self.uploadScene(scene)
        v = np.ascontiguousarray(scene.verts, dtype=np.float32).reshape(-1, 9)
        m = np.ascontiguousarray(scene.tri_mat, dtype=np.int32)
        a = np.ascontiguousarray(scene.albedo, dtype=np.float32).reshape(-1, 3)
        e = ctypes.c_char_p()
        ok = self._lib.hipptUploadMesh(_ptr(v, ctypes.c_float), _ptr(m, ctypes.c_int), int(v.shape[0]),
                                       _ptr(a, ctypes.c_float), int(a.shape[0]), _d3(scene.lookfrom),
                                       _d3(scene.lookat), _d3(scene.vup), float(scene.vfov),
                                       float(scene.aperture), float(scene.focus), ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "mesh upload failed"))
        self._albedo = a.copy()

    def updateVertices(self, verts) -> None:  # noqa: N802
        """hipptUpdateVertices: new vertices (n, 9) float32 for the uploaded scene's n triangles, in place
        and in stream order (renders and queries enqueued later see them; nothing is drained or
        reallocated; the BVH is refitted, not rebuilt: uploadScene is the rebuild).  A numpy array is
        copied before the call returns.  A tensor on the ROCm device is read from where it is, after
        torch's current stream is synchronised (see traceRays on sharing one HIP runtime with torch):
        keep it unchanged until the next synchronize() or blocking render."""
        v, dev = _update_verts(verts)
        e = ctypes.c_char_p()
        if dev:
            import torch
            torch.cuda.current_stream(v.device).synchronize()
            ok = self._lib.hipptUpdateVertices(v.data_ptr(), int(v.shape[0]), VERTS_DEVICE, ctypes.byref(e))
        else:
            ok = self._lib.hipptUpdateVertices(v.ctypes.data, int(v.shape[0]), 0, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "vertex update failed"))

    def setEnvironment(self, texels) -> None:  # noqa: N802
        """hipptSetEnvironment: an (S, S, 3) float32 octahedral environment map (texels[y, x]; finite, >= 0, may
        exceed 1; env_directions(S) gives the texels' directions, env_from_equirect a map from a lat-long image)
        in place of the sky gradient for every uploaded scene, in stream order: renders and path queries
        enqueued later see it.  None removes it.  It stays across uploads and initialize() until removed.  A
        numpy array is validated and copied before the call returns; a tensor on the ROCm device is fetched
        from where it is, uninspected, after torch's current stream is synchronised."""
        e = ctypes.c_char_p()
        if texels is None:
            ok = self._lib.hipptSetEnvironment(None, 0, 0, ctypes.byref(e))
        else:
            dev = _is_tensor(texels) and texels.device.type != "cpu"
            if _is_tensor(texels):
                import torch
                if texels.dtype != torch.float32:
                    raise HipptError(f"texels must be float32, not {texels.dtype}")
                if not texels.is_contiguous():
                    raise HipptError("texels must be contiguous")
                if not dev:
                    texels = texels.numpy()
            elif not isinstance(texels, np.ndarray):
                raise HipptError("texels must be a numpy array or a torch tensor")
            elif texels.dtype != np.float32:
                raise HipptError(f"texels must be float32, not {texels.dtype}")
            elif not texels.flags["C_CONTIGUOUS"]:
                raise HipptError("texels must be contiguous")
            shape = tuple(texels.shape)
            if len(shape) != 3 or shape[0] != shape[1] or shape[2] != 3:
                raise HipptError(f"texels must have shape (S, S, 3), not {shape}")
            if dev:
                import torch
                torch.cuda.current_stream(texels.device).synchronize()
                ok = self._lib.hipptSetEnvironment(texels.data_ptr(), int(shape[0]), ENV_DEVICE, ctypes.byref(e))
            else:
                ok = self._lib.hipptSetEnvironment(texels.ctypes.data, int(shape[0]), 0, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "setting the environment failed"))

    def environment(self) -> Optional[np.ndarray]:
        """The environment as context 0 holds it after the queued work, (S, S, 3) float32; None without one."""
        t = scene_download(SCENE_ENVIRONMENT)
        if t.size == 0:
            return None
        size = int(round(t.shape[0] ** 0.5))
        return np.ascontiguousarray(t.view(np.float32).reshape(size, size, 4)[:, :, :3])

    def envTable(self) -> Optional[dict]:  # noqa: N802
        """The environment's selection table as the device built it (include/hippt.h HIPPT_OPT_ENV_SAMPLING), after
        the queued work: {"rows": structured (S,) with m (the row's integer weight) and C (its inclusive sum),
        "texels": structured (S, S) with q (the texel's integer weight within its row), c (its inclusive sum along
        the row) and k (float32: the draw's density per unit of (u, w) area)}.  None without an environment."""
        t = scene_download(SCENE_ENV_TABLE).reshape(-1)
        if t.size == 0:
            return None
        size = int(round((-2 + (4 + 12 * t.size) ** 0.5) / 6))
        assert 2 * size + 3 * size * size == t.size
        return {"rows": t[:2 * size].view(ENV_ROW_DTYPE), "texels": t[2 * size:].view(ENV_TEXEL_DTYPE).reshape(size, size)}

    def lightTable(self) -> np.ndarray:  # noqa: N802
        """The light selection table as the device built it (include/hippt.h HIPPT_OPT_LIGHT_SELECT), after the
        queued work: a structured array with one entry per light in ascending primitive id: `prim` the id as
        uploaded, `q` the light's integer weight, `c` the inclusive sum of q, `ip` the inverse of its selection
        probability (float32; 0 for a light that is never selected).  Empty for a scene without lights."""
        return scene_download(SCENE_LIGHTS).reshape(-1).view(LIGHT_TABLE_DTYPE)

    def updateDropped(self) -> int:  # noqa: N802
        """Triangles the last device-memory update dropped for a non-finite coordinate (synchronises)."""
        return int(self._lib.hipptGetOption(INFO_UPDATE_DROPPED))

    def setDevices(self, device_ids: Sequence[int]) -> None:  # noqa: N802
        arr = (ctypes.c_int * max(1, len(device_ids)))(*device_ids)
        e = ctypes.c_char_p()
        if not self._lib.hipptSetDevices(arr, len(device_ids), ctypes.byref(e)):
            raise HipptError(_err(e, "bad devices"))
        self._devices = [int(d) for d in device_ids]

    def setRowRange(self, y0: int, y1: int) -> None:  # noqa: N802
        e = ctypes.c_char_p()
        if not self._lib.hipptSetRowRange(int(y0), int(y1), ctypes.byref(e)):
            raise HipptError(_err(e, "bad row range"))

    def setRowInterleave(self, phase: int, stride: int) -> None:  # noqa: N802
        """Render rows phase, phase+stride, ... (one process per GPU: phase=rank, stride=world)."""
        e = ctypes.c_char_p()
        if not self._lib.hipptSetRowInterleave(int(phase), int(stride), ctypes.byref(e)):
            raise HipptError(_err(e, "bad row interleave"))

    def setOption(self, key: int, value: int) -> None:  # noqa: N802
        if not self._lib.hipptSetOption(int(key), int(value)):
            raise HipptError(f"invalid option {key}={value}")

    def stats(self) -> dict:
        s = Stats()
        if not self._lib.hipptGetStats(ctypes.byref(s)):
            raise HipptError("hipptGetStats failed")
        return s.as_dict()

    PHASES = ("outer", "camera", "traversal_round", "node", "leaf", "triangle", "shade", "sphere_reject")

    def counters(self) -> dict:
        """Raw device counters incl. per-phase SIMD efficiency (counting builds)."""
        buf = (ctypes.c_ulonglong * 32)()
        n = self._lib.hipptGetCounters(buf, 32)
        v = list(buf)[:n]
        out = {"segments": v[0], "pixelSamples": v[1], "nodeVisits": v[2], "triTests": v[3]}
        for k, name in enumerate(self.PHASES):
            w, l = v[4 + 2 * k], v[5 + 2 * k]
            out[name] = {"wave": w, "lane": l, "simd_eff": round(l / (64 * w), 4) if w else None}
        # 4-wide node visits by number of hit children (0..4)
        out["hit_children"] = v[20:25]
        # of the visits with none hit: those with a child box hit before the closest-hit cut
        out["culled_by_best_t"] = v[25]
        # node visits served by the LDS copy of the top of a global-memory tree
        out["lds_top_visits"] = v[26] if len(v) > 26 else 0
        # shadow rays among `segments` (renders under OPT_LIGHT_SAMPLING)
        out["shadow_rays"] = v[27] if len(v) > 27 else 0
        return out

    def resetStats(self) -> None:  # noqa: N802
        self._lib.hipptResetStats()

    # --- ray queries (include/hippt.h "ray queries") ----------------------------------------------------
    def traceRays(self, rays):  # noqa: N802
        """Closest hit of each ray (origin xyz, tmin, direction xyz, tmax): (t float32 (N,), prim int32
        (N,)); a miss is (inf, -1).  numpy in, numpy out; a tensor on the ROCm device in, tensors on
        that device out (torch's current stream is synchronised first; nothing is staged).  Device
        tensors need torch and libhippt.so on one HIP runtime: import torch before the first hippt
        call, so that the library binds to the runtime torch has loaded; otherwise the library does not
        know torch's allocations and reports them as not device memory."""
        r, dev = _query_rays(rays)
        n = int(r.shape[0])
        e = ctypes.c_char_p()
        if dev:
            import torch
            t = torch.empty(n, dtype=torch.float32, device=r.device)
            prim = torch.empty(n, dtype=torch.int32, device=r.device)
            torch.cuda.current_stream(r.device).synchronize()
            ok = self._lib.hipptTraceRays(r.data_ptr(), n, RAYS_DEVICE, t.data_ptr(), prim.data_ptr(), ctypes.byref(e))
        else:
            t = np.empty(n, np.float32)
            prim = np.empty(n, np.int32)
            ok = self._lib.hipptTraceRays(r.ctypes.data, n, 0, t.ctypes.data, prim.ctypes.data, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "ray query failed"))
        return t, prim

    def occluded(self, rays):
        """1 where any primitive is hit within [tmin, tmax), else 0: uint8 (N,), numpy or tensor as the rays."""
        r, dev = _query_rays(rays)
        n = int(r.shape[0])
        e = ctypes.c_char_p()
        if dev:
            import torch
            occ = torch.empty(n, dtype=torch.uint8, device=r.device)
            torch.cuda.current_stream(r.device).synchronize()
            ok = self._lib.hipptOccluded(r.data_ptr(), n, RAYS_DEVICE, occ.data_ptr(), ctypes.byref(e))
        else:
            occ = np.empty(n, np.uint8)
            ok = self._lib.hipptOccluded(r.ctypes.data, n, 0, occ.ctypes.data, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "occlusion query failed"))
        return occ

    def traceCamera(self, frame: int = 0):  # noqa: N802
        """First hit of sample `frame`'s camera ray of every pixel: (t float32 (H, W), prim int32 (H, W)),
        row 0 = v = 0; a miss is (inf, -1)."""
        t = np.empty((self._height, self._width), np.float32)
        prim = np.empty((self._height, self._width), np.int32)
        e = ctypes.c_char_p()
        if not self._lib.hipptTraceCamera(int(frame), 0, t.ctypes.data, prim.ctypes.data, ctypes.byref(e)):
            raise HipptError(_err(e, "camera query failed"))
        return t, prim

    def pick(self, x: int, y: int, frame: int = 0):
        """(prim, t) under pixel (x, y) (row y = 0 is v = 0) for sample `frame`'s camera ray; (-1, inf)
        over the sky."""
        if not (0 <= int(x) < self._width and 0 <= int(y) < self._height):
            raise HipptError(f"pixel ({x}, {y}) outside the {self._width}x{self._height} image")
        t, prim = self.traceCamera(frame)
        return int(prim[int(y), int(x)]), float(t[int(y), int(x)])

    def traceHits(self, rays):  # noqa: N802
        """The hit record of each ray's closest hit (hipptHit: t and prim as traceRays, the renderer's
        shading normal faced against the ray, the barycentrics u, v of a triangle hit, matFlags = material
        index | HIT_SPHERE | HIT_BACKFACE); a miss is (inf, -1, 0, 0, 0, 0, 0, -1).  numpy rays in: a
        structured array (N,) of HIT_DTYPE.  A tensor on the ROCm device in (as for traceRays): an
        (N, 8) float32 tensor on that device, one record per row; split_hits() gives the fields as views."""
        r, dev = _query_rays(rays)
        n = int(r.shape[0])
        e = ctypes.c_char_p()
        if dev:
            import torch
            hits = torch.empty((n, 8), dtype=torch.float32, device=r.device)
            torch.cuda.current_stream(r.device).synchronize()
            ok = self._lib.hipptTraceHits(r.data_ptr(), n, RAYS_DEVICE, hits.data_ptr(), ctypes.byref(e))
        else:
            hits = np.empty(n, HIT_DTYPE)
            ok = self._lib.hipptTraceHits(r.ctypes.data, n, 0, hits.ctypes.data, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "hit query failed"))
        return hits

    def traceCameraHits(self, frame: int = 0):  # noqa: N802
        """The hit record of sample `frame`'s camera ray of every pixel: HIT_DTYPE (H, W), row 0 = v = 0."""
        hits = np.empty((self._height, self._width), HIT_DTYPE)
        e = ctypes.c_char_p()
        if not self._lib.hipptTraceCameraHits(int(frame), 0, hits.ctypes.data, ctypes.byref(e)):
            raise HipptError(_err(e, "camera hit query failed"))
        return hits

    # --- path queries (include/hippt.h "path queries") ---------------------------------------------------
    def traceRadiance(self, rays, seeds=None, max_depth: int = 8):  # noqa: N802
        """The renderer's path from each ray (as traceRays: origin xyz, tmin, direction xyz, tmax; tmin and
        tmax hold for the first segment only) with RNG state seeds[i] (int32 or uint32 bits, where the rays
        are; None: path_seeds(N, 0)): (radiance float32 (N, 4): rgb and 1.0 where the first segment hit,
        segments int32 (N,): closest-hit queries made).  numpy in, numpy out; tensors on the ROCm device in,
        tensors on that device out (see traceRays on sharing one HIP runtime with torch)."""
        r, dev = _query_rays(rays)
        n = int(r.shape[0])
        sd = _path_seeds_arg(seeds, n, r, dev)
        e = ctypes.c_char_p()
        if dev:
            import torch
            rad = torch.empty((n, 4), dtype=torch.float32, device=r.device)
            segs = torch.empty(n, dtype=torch.int32, device=r.device)
            torch.cuda.current_stream(r.device).synchronize()
            ok = self._lib.hipptTraceRadiance(r.data_ptr(), sd.data_ptr(), n, int(max_depth), RAYS_DEVICE, rad.data_ptr(),
                                              segs.data_ptr(), ctypes.byref(e))
        else:
            rad = np.empty((n, 4), np.float32)
            segs = np.empty(n, np.int32)
            ok = self._lib.hipptTraceRadiance(r.ctypes.data, sd.ctypes.data, n, int(max_depth), 0, rad.ctypes.data,
                                              segs.ctypes.data, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "path query failed"))
        return rad, segs

    def cameraRays(self, frame: int = 0, device: bool = False):  # noqa: N802
        """The rays renderFrames starts sample `frame` of every pixel with and the RNG state each is left
        with after the camera sample: (rays float32 (H*W, 8), seeds (H*W,)), row 0 = v = 0, so that
        traceRadiance(*cameraRays(f)) is sample f of the renderer.  numpy (seeds uint32), or with
        device=True tensors on the context's device (seeds int32, the same bits)."""
        n = self._height * self._width
        e = ctypes.c_char_p()
        if device:
            import torch
            dev = torch.device("cuda", self._devices[0] if self._devices else torch.cuda.current_device())
            rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
            seeds = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ok = self._lib.hipptCameraRays(int(frame), RAYS_DEVICE, rays.data_ptr(), seeds.data_ptr(), ctypes.byref(e))
        else:
            rays = np.empty((n, 8), np.float32)
            seeds = np.empty(n, np.uint32)
            ok = self._lib.hipptCameraRays(int(frame), 0, rays.ctypes.data, seeds.ctypes.data, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "camera rays failed"))
        return rays, seeds

    def gbuffer(self, frame: int = 0) -> dict:
        """The guide buffers of sample `frame`'s camera rays, each (H, W) with row 0 = v = 0: depth (t;
        inf over the sky), prim (-1), normal (H, W, 3) faced towards the camera (0), albedo (H, W, 3)
        of the hit's material as uploaded (0 over the sky; of a MAT_EMISSIVE hit its emission, which may
        exceed 1), material (the index; -1)."""
        if self._albedo is None:
            raise HipptError("gbuffer: no scene uploaded through this PathTracer")
        hits = self.traceCameraHits(frame)
        hit = hits["prim"] >= 0
        material = np.where(hit, hits["matFlags"] & HIT_MATERIAL_MASK, -1).astype(np.int32)
        albedo = np.zeros(hit.shape + (3,), np.float32)
        albedo[hit] = self._albedo[material[hit]]
        return {"depth": hits["t"].copy(), "prim": hits["prim"].copy(), "normal": hits["normal"].copy(),
                "albedo": albedo, "material": material}

    # --- denoiser (include/hippt.h "denoiser") ----------------------------------------------------------
    def denoise(self, passes: int = 5, sigma_color: float = 1.0, sigma_depth: float = 0.05, normal_power: int = 6,
                guide_frame: int = 0, demodulate: bool = True, tensors: bool = False):
        """hipptDenoise: the accumulation filtered on the device by the edge-avoiding A-trous wavelet of
        include/hippt.h, guided by sample `guide_frame`'s hit records: (pixels (H, W) uint32 in the current
        pixel format, rgba (H, W, 4) float32, linear, alpha 1), row 0 = v = 0.  The accumulation, the image
        and the counters stay as they are.  tensors=True: both are torch tensors on the context's device,
        written there (see traceRays on sharing one HIP runtime with torch)."""
        p = DenoiseParams()
        self._lib.hipptDenoiseDefaults(ctypes.byref(p))
        p.passes, p.guideFrame, p.normalPower = int(passes), int(guide_frame), int(normal_power)
        p.sigmaColor, p.sigmaDepth = float(sigma_color), float(sigma_depth)
        p.flags = 0 if demodulate else DENOISE_NO_DEMODULATE
        h, w = self._height, self._width
        e = ctypes.c_char_p()
        if tensors:
            import torch
            dev = torch.device("cuda", self._devices[0] if self._devices else torch.cuda.current_device())
            pixels = torch.empty((h, w), dtype=torch.int32, device=dev)
            rgba = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            p.flags |= DENOISE_DEVICE
            ok = self._lib.hipptDenoise(ctypes.byref(p), pixels.data_ptr(), rgba.data_ptr(), ctypes.byref(e))
            pixels = pixels.view(torch.uint32) if hasattr(torch, "uint32") else pixels
        else:
            pixels = np.empty((h, w), np.uint32)
            rgba = np.empty((h, w, 4), np.float32)
            ok = self._lib.hipptDenoise(ctypes.byref(p), pixels.ctypes.data, rgba.ctypes.data, ctypes.byref(e))
        if not ok:
            raise HipptError(_err(e, "denoise failed"))
        return pixels, rgba

    def denoiseTimes(self) -> dict:  # noqa: N802
        """Device milliseconds per stage of the last denoise() made under OPT_DENOISE_TIMING (stages that
        did not run are left out)."""
        ns = {name: int(self._lib.hipptGetOption(INFO_DENOISE_NS + k)) for k, name in enumerate(DENOISE_STAGES)}
        return {name: v / 1e6 for name, v in ns.items() if v > 0}

    def pickHit(self, x: int, y: int, frame: int = 0) -> dict:  # noqa: N802
        """The hit record under pixel (x, y) (row y = 0 is v = 0) for sample `frame`'s camera ray, as a
        dict: t, prim, normal (3 floats), u, v, material (-1 over the sky), sphere, backface."""
        if not (0 <= int(x) < self._width and 0 <= int(y) < self._height):
            raise HipptError(f"pixel ({x}, {y}) outside the {self._width}x{self._height} image")
        h = self.traceCameraHits(frame)[int(y), int(x)]
        hit, mf = int(h["prim"]) >= 0, int(h["matFlags"])
        return {"t": float(h["t"]), "prim": int(h["prim"]), "normal": tuple(float(c) for c in h["normal"]),
                "u": float(h["u"]), "v": float(h["v"]), "material": mf & HIT_MATERIAL_MASK if hit else -1,
                "sphere": hit and bool(mf & HIT_SPHERE), "backface": hit and mf < 0}


AUDIT_MAGIC = 0xC4A1D17
AUDIT_BATCHES = 256


def chain_audit() -> list:
    """The chained runs closed since the last call (HIPPT_OPT_CHAIN_AUDIT, include/hippt.h
    hipptChainAudit): a list of (header dict, records uint32 array [batches + 1, 16]).  Synchronises."""
    lib = load_library()
    runs = []
    while True:
        buf = np.zeros(1 << 22, np.uint32)
        n = lib.hipptChainAudit(_ptr(buf, ctypes.c_uint), buf.size)
        if n < 0:
            raise HipptError("hipptChainAudit failed")
        if n == 0:
            return runs
        k = 0
        while k < n:
            h = buf[k:k + 16]
            assert h[0] == AUDIT_MAGIC, "audit stream out of step"
            hdr = dict(run=int(h[1]), device=int(h[2]), firstFrame=int(h[3].astype(np.int32)),
                       step=int(h[4].astype(np.int32)), frames=int(h[5]), bandPixels=int(h[6]), totalItems=int(h[7]),
                       batches=int(h[8]), launches=int(h[9]), slots=int(h[10]), overflow=int(h[11]))
            recs = min(hdr["batches"], AUDIT_BATCHES) + 1
            runs.append((hdr, buf[k + 16:k + 16 + recs * 16].reshape(recs, 16).copy()))
            k += 16 + recs * 16


def device_count() -> int:
    return int(load_library().hipptDeviceCount())


def row_band(rank: int, world: int, height: int):
    """Contiguous row band of rank in [0, world): rows [floor(r*H/N), floor((r+1)*H/N))."""
    return (rank * height) // world, ((rank + 1) * height) // world
