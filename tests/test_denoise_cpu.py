"""The denoiser without a GPU: the numpy model of its contract (tests/denoise_ref.py) denoises, keeps what
the contract says it keeps, and the C ABI of hipptDenoise (struct size, defaults, every argument error
before any device call).

"Denoises" is a condition, not a tuned number: against the converged reference means of tests/golden the
mean squared error of the colours clamped to [0, 1] must fall below half the noisy image's."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import denoise_ref as dr
import hippt
import pyoracle as po
from hippt import scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cornell34": (64, 64, 4096), "cornell_mixed": (48, 48, 2048)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, guide records of sample 0, materials, {spp: oracle accumulation}); computed once, never modified."""
    w, h, _ = CASES[name]
    sc = scenes.get_scene(name)
    hits = dr.guides(sc, w, h, 0)
    acc = {spp: po.MeshScene(sc, w, h).frames(0, spp, 8)[1] for spp in (1, 4)}
    for a in (hits, *acc.values()):
        a.setflags(write=False)
    return sc, hits, sc.materials(), acc


def mse(img, ref):
    d = np.clip(img[..., :3].astype(np.float64), 0.0, 1.0) - np.clip(ref.astype(np.float64), 0.0, 1.0)
    return float((d * d).mean())


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_the_model_denoises(golden_dir, name, spp):
    w, h, n = CASES[name]
    ref = np.load(os.path.join(golden_dir, f"ref_converge_{name}_{w}x{h}_{n}.npy"))[..., :3]
    _, hits, mats, acc = case(name)
    rgba = dr.filtered(acc[spp], hits, mats)
    noisy, clean = mse(acc[spp], ref), mse(rgba, ref)
    print(f"{name} {spp} spp: mse noisy {noisy:.6f} denoised {clean:.6f} ratio {clean / noisy:.3f}")
    assert clean < 0.5 * noisy, (noisy, clean)


@pytest.mark.parametrize("name", list(CASES))
def test_no_passes_without_demodulation_is_the_identity(name):
    _, hits, mats, acc = case(name)
    px, rgba = dr.denoise(acc[4], hits, mats, passes=0, demodulate=False)
    assert rgba[..., :3].tobytes() == np.ascontiguousarray(acc[4][..., :3]).tobytes()
    assert np.all(rgba[..., 3] == 1.0)
    sc = case(name)[0]
    w, h, _ = CASES[name]
    opx = po.MeshScene(sc, w, h).frames(0, 4, 8)[0]
    assert np.array_equal(px, opx)  # the model's ARGB word is the renderer's
    assert np.array_equal(dr.pack_pixel(acc[4], dr.PIXEL_RGBA8), po.rgba8(acc[4]))


@pytest.mark.parametrize("name", list(CASES))
def test_sky_is_unchanged_and_the_output_is_finite(name):
    _, hits, mats, acc = case(name)
    sky = hits["prim"] < 0
    if name == "cornell_mixed":
        assert sky.any() and not sky.all()
    want = np.ascontiguousarray(acc[1][..., :3])[sky].tobytes()
    for passes in (0, 1, 3, 5, 8):
        rgba = dr.filtered(acc[1], hits, mats, passes=passes)
        assert rgba.dtype == np.float32 and np.isfinite(rgba).all(), passes
        assert rgba[..., :3][sky].tobytes() == want, passes


def test_demodulation_uses_lambertian_albedo_only():
    sc, hits, mats, _ = case("cornell_mixed")
    ap = dr.albedo_prime(hits, mats)
    hit = hits["prim"] >= 0
    idx = hits["matFlags"] & hippt.HIT_MATERIAL_MASK
    lamb = hit & (mats["kind"][np.where(hit, idx, 0)] == 0)
    assert lamb.any() and (hit & ~lamb).any()  # the condition: both kinds of hit are in the image
    assert np.all(ap[~lamb] == 1.0)
    assert np.all((ap[lamb] == mats["albedo"][idx[lamb]]) | (ap[lamb] == 1.0))
    assert np.all(dr.albedo_prime(hits, mats, demodulate=False) == 1.0)


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_params_struct_and_defaults():
    assert ctypes.sizeof(hippt.DenoiseParams) == 32
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    assert re.search(r"HIPPT_DENOISE_NO_DEMODULATE\s*=\s*1\b", header) and hippt.DENOISE_NO_DEMODULATE == 1
    assert re.search(r"HIPPT_DENOISE_DEVICE\s*=\s*2\b", header) and hippt.DENOISE_DEVICE == 2
    p = hippt.DenoiseParams()
    hippt.load_library().hipptDenoiseDefaults(ctypes.byref(p))
    assert (p.passes, p.guideFrame, p.normalPower, p.flags) == (5, 0, 6, 0)
    assert (p.sigmaColor, p.sigmaDepth) == (1.0, float(np.float32(0.05))) and tuple(p.reserved) == (0.0, 0.0)
    hippt.load_library().hipptDenoiseDefaults(None)  # ignored


def test_timing_option_round_trips():
    lib = hippt.load_library()
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    assert re.search(r"HIPPT_OPT_DENOISE_TIMING\s*=\s*36\b", header) and hippt.OPT_DENOISE_TIMING == 36
    assert re.search(r"HIPPT_INFO_DENOISE_NS\s*=\s*200\b", header) and hippt.INFO_DENOISE_NS == 200
    assert lib.hipptGetOption(hippt.OPT_DENOISE_TIMING) == 0
    assert lib.hipptSetOption(hippt.OPT_DENOISE_TIMING, 1) and lib.hipptGetOption(hippt.OPT_DENOISE_TIMING) == 1
    assert not lib.hipptSetOption(hippt.OPT_DENOISE_TIMING, 2) and lib.hipptGetOption(hippt.OPT_DENOISE_TIMING) == 1
    assert lib.hipptSetOption(hippt.OPT_DENOISE_TIMING, 0)
    for k in range(len(hippt.DENOISE_STAGES)):
        assert lib.hipptGetOption(hippt.INFO_DENOISE_NS + k) >= 0  # (0 until a timed call ran the stage)
    assert lib.hipptGetOption(hippt.INFO_DENOISE_NS + len(hippt.DENOISE_STAGES)) == -1
    assert not lib.hipptSetOption(hippt.INFO_DENOISE_NS, 1)


def test_argument_errors_come_before_any_device_call():
    lib = hippt.load_library()
    lib.cudaPathTracerShutdown()
    pt = hippt.PathTracer()
    pt.uploadMesh(scenes.cornell34())  # a scene, no Init
    px = np.zeros(16, np.uint32)
    rgba = np.zeros(64, np.float32)

    def call(pixels=px, out=rgba, **fields):
        p = hippt.DenoiseParams()
        lib.hipptDenoiseDefaults(ctypes.byref(p))
        for k, v in fields.items():
            if k == "reserved":
                p.reserved[v[0]] = v[1]
            else:
                setattr(p, k, v)
        e = ctypes.c_char_p()
        ok = lib.hipptDenoise(ctypes.byref(p), pixels.ctypes.data if pixels is not None else None,
                              out.ctypes.data if out is not None else None, ctypes.byref(e))
        return ok, (e.value or b"").decode()

    bad = [({"passes": -1}, "passes"), ({"passes": 9}, "passes"), ({"normalPower": -1}, "normal power"),
           ({"normalPower": 11}, "normal power"), ({"guideFrame": -1}, "guide frame"),
           ({"sigmaColor": 0.0}, "sigmaColor"), ({"sigmaColor": -1.0}, "sigmaColor"),
           ({"sigmaColor": float("inf")}, "sigmaColor"), ({"sigmaColor": float("nan")}, "sigmaColor"),
           ({"sigmaDepth": 0.0}, "sigmaDepth"), ({"sigmaDepth": float("inf")}, "sigmaDepth"),
           ({"sigmaDepth": float("nan")}, "sigmaDepth"), ({"flags": 4}, "unknown flags"),
           ({"reserved": (0, 1.0)}, "reserved"), ({"reserved": (1, -2.0)}, "reserved")]
    for fields, word in bad:
        ok, msg = call(**fields)
        assert not ok and word in msg, (fields, msg)
    ok, msg = call(pixels=None, out=None)
    assert not ok and "no output buffer" in msg
    ok, msg = call()  # everything valid but no Init
    assert not ok and "not initialized" in msg
    e = ctypes.c_char_p()
    assert not lib.hipptDenoise(None, px.ctypes.data, None, ctypes.byref(e)) and b"not initialized" in e.value
    assert not lib.hipptDenoise(None, px.ctypes.data, None, None)  # a null message pointer is allowed
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    ok, msg = call()
    assert not ok and "built-in scene" in msg
    with pytest.raises(hippt.HipptError, match="built-in scene"):
        pt.denoise()
    lib.cudaPathTracerShutdown()
