"""The combine's running average with the shared reciprocal (hippt_trace.h avg_div; DESIGN.md §5 "Exact division")
end to end on the GPU: accumulation and packed pixels word for word against oracle/pyoracle.py's MeshScene.frames,
which keeps plain division.

Images of 64x36 and 50x34 (the second no multiple of 64 pixels per row: runs end mid-row).  Cornell-34 with the sky
combine automatic and off (the camera of tests/sky_combine_cam.py, which leaves sky runs to the combine), chained
and unchained; cornell_mixed (spheres, the general kernel); blob70k (a tree in global memory); and Cornell-34 with
materials that have a zero albedo channel, so that the average divides exact zeros.  Three frame ranges, each as two
batches: from frame 0 (ff = 0, fc = 1); seven frames split 5 + 2; and from frame 16,777,213, where float(f + 1)
crosses 2^24 and stops being exact.  Depth 4."""
import dataclasses
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime

import hippt
import pyoracle as po
import sky_combine_cam as scc
from hippt import scenes

pytestmark = pytest.mark.gpu

DEPTH = 4
SIZES = [(64, 36), (50, 34)]
RANGES = {"from_0": ((0, 2), (2, 2)), "seven_5_2": ((2, 5), (7, 2)), "across_2p24": ((16777213, 3), (16777216, 2))}
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
    hippt.load_library().cudaPathTracerShutdown()


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "cornell34":
        return scc.pulled_back()
    if name == "cornell_mixed":
        return scc.pulled_back(scenes.cornell_mixed)
    if name == "cornell34_zero_channels":
        # white without green, red without blue: every path that leaves a wall carries an exact zero
        sc = scc.pulled_back()
        alb = np.array(sc.albedo, np.float32, copy=True)
        alb[0, 1] = 0.0
        alb[2, 2] = 0.0
        return dataclasses.replace(sc, albedo=alb)
    return scenes.get_scene(name)


@functools.lru_cache(maxsize=None)
def oracle(name, w, h, rng):
    (f0, n0), (f1, n1) = RANGES[rng]
    assert f1 == f0 + n0
    px, acc, _, _ = po.MeshScene(scene(name), w, h).frames(f0, n0 + n1, DEPTH)
    return px, acc


def render(pt, name, w, h, rng, chain, sky):
    lib = hippt.load_library()
    pt.setOption(hippt.OPT_CHAIN, chain)
    pt.setOption(hippt.OPT_SKY_COMBINE, sky)
    pt.setOption(hippt.OPT_ITEM_ORDER, 1)  # the item table at once: the sky combine needs it
    pt.uploadScene(scene(name))
    assert pt.initialize(w, h), pt.lastError()
    for first, n in RANGES[rng]:
        assert lib.hipptRenderFramesAsync(first, n, DEPTH, None), pt.lastError()
    return pt.readback()


def check(pt, name, w, h, skies):
    for rng in RANGES:
        want_px, want_acc = oracle(name, w, h, rng)
        for chain in (0, 8):
            for sky in skies:
                px, acc = render(pt, name, w, h, rng, chain, sky)
                where = f"{name} {w}x{h} {rng} chain {chain} sky combine {sky}"
                diff = int(np.count_nonzero(acc.view(np.uint32) != want_acc.view(np.uint32)))
                assert diff == 0, f"{where}: {diff} accumulation words differ"
                assert np.array_equal(px, want_px), f"{where}: {int(np.count_nonzero(px != want_px))} pixels differ"


@pytest.mark.parametrize("w,h", SIZES)
def test_cornell_sky_combine_on_and_off(pt, w, h):
    check(pt, "cornell34", w, h, skies=(-1, 0))


@pytest.mark.parametrize("w,h", SIZES)
def test_cornell_mixed_spheres(pt, w, h):
    check(pt, "cornell_mixed", w, h, skies=(-1,))


@pytest.mark.parametrize("w,h", SIZES)
def test_tree_in_global_memory(pt, w, h):
    check(pt, "blob70k", w, h, skies=(-1,))


@pytest.mark.parametrize("w,h", SIZES)
def test_zero_albedo_channels(pt, w, h):
    sc = scene("cornell34_zero_channels")
    assert np.count_nonzero(np.asarray(sc.albedo) == 0.0) == 2
    check(pt, "cornell34_zero_channels", w, h, skies=(-1, 0))
    _, acc = oracle("cornell34_zero_channels", w, h, "from_0")
    assert np.count_nonzero(acc[..., :3] == 0.0) > 0  # the average did divide zeros
