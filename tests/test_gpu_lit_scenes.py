"""Emissive materials and light sampling beyond the Cornell box (GPU): the scenes of tests/lit_scenes.py through
hipptTraceRadiance, the render calls and hipptUpdateVertices against the references of tests/nee_ref.py and
tests/emit_ref.py, bit for bit.

blob64x34_lit is a deep tree in global memory with 273 lights scattered through leaf order (8 of zero area);
random_scene_lit has 69 sphere lights among Metal, Dielectric and Lambertian spheres under a lens camera (the
render route's camera sample draws the lens before the path); light_edges holds a black light, a 1e30 light, a
zero-area light and a light 1e-3 above a face, light_edges_one exactly one light.
tests/test_lit_scenes_cpu.py asserts on the references alone that these ray sets meet every case of the rule.
Every comparison is exact: the radiance words and segment counts of every ray, the accumulation's bytes, the
pixel words, the segment and shadow-ray totals.  A scene's rays, seeds and references are computed once."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import hippt
import lit_scenes as ls
import nee_ref as nr
import path_ref as pr
from refit_util import verts_of, with_verts, wobble
from test_gpu_light_sampling import assert_image, info
from test_gpu_ray_query import Ref, degenerate_rays, upload

pytestmark = pytest.mark.gpu

OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_SKY_RECT, 1),
        (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB), (hippt.OPT_LIGHT_SAMPLING, 0))
# (scene, HIPPT_OPT_LDS_SCENE): the blob with the scene copy asked for and not, the small scenes with it
SCENE_LDS = [("blob64x34_lit", 0), ("blob64x34_lit", 1), ("random_scene_lit", 1), ("light_edges", 1),
             ("light_edges_one", 1)]
RENDERED = [("blob64x34_lit", 0), ("blob64x34_lit", 1), ("random_scene_lit", 1), ("light_edges", 1)]


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    for k, v in OPTS:
        t.setOption(k, v)
    t.setOption(hippt.OPT_LIGHT_SAMPLING, 1)
    yield t
    for k, v in OPTS:
        t.setOption(k, v)
    hippt.load_library().cudaPathTracerShutdown()


# ---- 1. traceRadiance against the references -------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("name,lds", SCENE_LDS)
def test_radiance_with_light_sampling_matches_nee_ref(pt, name, lds, width):
    sc, rays, seeds, rad, segs = ls.nee_case(name)[:5]
    upload(pt, sc, lds, width)
    assert info(hippt.INFO_LIGHTS) == len(ls.scene_refs(name)[1].lights)
    full = len(rays)
    for n in (1, 65, full):
        got, gs = pt.traceRadiance(np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n]), 8)
        pr.assert_paths(got, gs, rad[:n], segs[:n], f"{name} lds={lds} width={width} n={n}")
    # finite, or infinite exactly where the reference is
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes() and not np.isnan(got).any()


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("name,lds", SCENE_LDS)
def test_radiance_without_light_sampling_matches_emit_ref(pt, name, lds, width):
    sc, rays, seeds, rad, segs = ls.emit_case(name)[:5]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING, 0)
    upload(pt, sc, lds, width)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name} lds={lds} width={width}, option off")


# ---- 2. the render route ----------------------------------------------------------------------------------
def render_and_compare(pt, name, what, asynchronous=False):
    sc, acc, px, total, shadow = ls.nee_render(name)
    w, h, frames = ls.SETS[name][1]
    pt.uploadMesh(sc)
    assert pt.initialize(w, h), pt.lastError()
    pt.resetStats()
    if asynchronous:
        for _ in range(frames):
            assert pt.renderFramesAsync(1, 8), pt.lastError()
        assert pt.synchronize(), pt.lastError()
    else:
        assert pt.renderFrames(frames, 8), pt.lastError()
    assert_image(pt.readback(), (px, acc), f"{name} {what}")
    st = pt.stats()
    assert st["segments"] == total and st["pixelSamples"] == w * h * frames, f"{name} {what}"
    assert 0 < shadow < total and pt.counters()["shadow_rays"] == shadow, f"{name} {what}"
    assert info(hippt.INFO_LIGHT_SAMPLING) == 1


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("name,lds", RENDERED)
def test_blocking_render_matches_the_render_reference(pt, name, lds, width):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    render_and_compare(pt, name, f"lds={lds} width={width}")
    assert np.array_equal(pt.hostPixels(), ls.nee_render(name)[2])


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("name,lds", RENDERED)
def test_asynchronous_single_frames_match_the_render_reference(pt, name, lds, width):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    render_and_compare(pt, name, f"asynchronous single frames, lds={lds} width={width}", asynchronous=True)


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_emissive_render_without_light_sampling_on_the_blob(pt, mode, width):
    """The EMIT megakernel (HIPPT_OPT_PATH_MODE 0) and the wavefront's shade kernel (1) on a real tree."""
    name = "blob64x34_lit"
    sc, acc, px, total = ls.emit_render(name)
    w, h, frames = ls.SETS[name][1]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING, 0)
    pt.setOption(hippt.OPT_PATH_MODE, mode)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    pt.uploadMesh(sc)
    assert pt.initialize(w, h), pt.lastError()
    pt.resetStats()
    assert pt.renderFrames(frames, 8), pt.lastError()
    assert_image(pt.readback(), (px, acc), f"{name} option off, path mode {mode} width={width}")
    assert pt.stats()["segments"] == total and info(hippt.INFO_LIGHT_SAMPLING) == 0


# ---- 3. animated mesh ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moved_blob():
    """(moved vertices, moved scene, rays, seeds, reference radiance and segments of the first 513 rays)."""
    sc, rays, seeds = ls.nee_case("blob64x34_lit")[:3]
    n = len(rays) - degenerate_rays().shape[0]
    rays, seeds = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n])
    v1 = wobble(verts_of(sc))
    sc1 = with_verts(sc, v1)
    rad, segs = nr.NeeRef(sc1, Ref(sc1)).paths(rays[:513], seeds[:513], 8)[:2]
    for a in (v1, rays, seeds, rad, segs):
        a.setflags(write=False)
    return v1, sc1, rays, seeds, rad, segs


@pytest.mark.parametrize("lds", [1, 0])
def test_results_after_a_vertex_update_equal_a_fresh_upload(pt, lds):
    sc = ls.scene_refs("blob64x34_lit")[0]
    v1, sc1, rays, seeds, rad, segs = moved_blob()
    w, h, frames = ls.SETS["blob64x34_lit"][1]
    upload(pt, sc, lds, w=w, h=h)
    before, _ = pt.traceRadiance(rays, seeds, 8)
    pt.updateVertices(np.array(v1))
    got, gs = pt.traceRadiance(rays, seeds, 8)
    assert pt.renderFrames(frames, 8), pt.lastError()
    img = pt.readback()
    upload(pt, sc1, lds, w=w, h=h)
    assert info(hippt.INFO_LIGHTS) == 273
    want, ws = pt.traceRadiance(rays, seeds, 8)
    assert pt.renderFrames(frames, 8), pt.lastError()
    fresh = pt.readback()
    # the update moves every light and changes what most paths return; the light list needs no rebuild
    assert np.count_nonzero((got != before).any(axis=1)) > len(rays) // 2
    pr.assert_paths(got, gs, want, ws, f"after updateVertices, lds={lds}")
    assert_image(img, fresh, f"render after updateVertices, lds={lds}")
    # and the fresh upload is the reference's (the first 513 rays: the reference is per ray, in Python)
    pr.assert_paths(want[:513], ws[:513], rad, segs, "fresh upload of the moved scene")
