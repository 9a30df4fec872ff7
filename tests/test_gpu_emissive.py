"""Emissive materials (GPU): HIPPT_MAT_EMISSIVE in hipptTraceRadiance, the render paths and the denoiser
against the reference of tests/emit_ref.py, bit for bit.

The reference is path_ref.PathRef with the emissive rule (pinned by tests/test_emit_ref_cpu.py, which also
asserts on the reference alone that the ray sets and camera samples end on lights at segment 0, at later
segments and on the last segment the depth allows).  Every comparison is exact: the radiance words and
segment counts of every ray, the accumulation's bytes, the pixel words and the segment totals.  A scene's
rays, seeds and references are computed once and shared by its tests."""
import os
import subprocess

import numpy as np
import pytest
import torch# before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import chain_audit
import denoise_ref as dr
import emit_ref as er
import hippt
import path_ref as pr
from hippt import scenes
from refit_util import verts_of, with_verts, wobble
from test_gpu_ray_query import N, Ref, degenerate_rays, upload

pytestmark = pytest.mark.gpu

W, H, FRAMES = 32, 24, 3
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_SKY_RECT, 1),
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


# ---- 1. traceRadiance against the reference ---------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", list(er.LIT))
def test_radiance_and_segments_match_the_reference(pt, name, lds, width):
    sc, rays, seeds, rad, segs = er.emit_case(name)[:5]
    upload(pt, sc, lds, width)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name} lds={lds} width={width}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depth_limits(pt, depth):
    sc, rays, seeds, rad, segs, ends = er.emit_case("cornell_mixed_lit", depth)[:6]
    lit = ends == er.EMITTED
    # conditions on the reference alone: lights end paths on the last segment the depth allows
    assert segs.max() == depth and np.count_nonzero(lit & (segs == depth)) >= 10
    if depth == 1:  # lights are lit, every other hit is black
        assert rad[lit, :3].all() and not rad[ends == er.DEPTH, :3].any() and np.count_nonzero(ends == er.DEPTH) > 1000
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, depth)
    pr.assert_paths(got, gs, rad, segs, f"maxDepth {depth}")


def test_device_memory_gives_the_same_bytes(pt):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs = er.emit_case("cornell_mixed_lit")[:5]
    pt.setDevices([0])
    upload(pt, sc)
    dev = torch.device("cuda", 0)
    dr_ = torch.from_numpy(np.array(rays)).to(dev)
    ds = torch.from_numpy(np.array(seeds).view(np.int32)).to(dev)
    r, s = pt.traceRadiance(dr_, ds, 8)
    assert r.device == dr_.device and s.device == dr_.device
    assert r.cpu().numpy().tobytes() == rad.tobytes() and s.cpu().numpy().tobytes() == segs.tobytes()
    del dr_, ds, r, s
    pt.setDevices([])


# ---- 2. the render paths ------------------------------------------------------------------------------
def render_and_compare(pt, name, what, chained=False):
    sc, acc, px, total = er.render_case(name)[:4]
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    if chained:
        for _ in range(FRAMES):
            assert pt.renderFramesAsync(1, 8), pt.lastError()
        assert pt.synchronize(), pt.lastError()
    else:
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
    gpx, gacc = pt.readback()
    bad = np.argwhere((gacc.view(np.uint32) != acc.view(np.uint32)).any(axis=-1))
    assert bad.size == 0, f"{name} {what}: {len(bad)} of {W * H} pixels differ, first (y, x) {bad[:4].tolist()}: " \
                          f"{gacc[tuple(bad[0])]} vs {acc[tuple(bad[0])]}"
    assert gacc.tobytes() == acc.tobytes() and np.array_equal(gpx, px), f"{name} {what}"
    assert pt.stats()["segments"] == total, f"{name} {what}"


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_blocking_megakernel_matches_the_render_reference(pt, name, lds, width):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    render_and_compare(pt, name, f"lds={lds} width={width}")


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_counting_kernels_match_the_render_reference(pt, name):
    pt.setOption(hippt.OPT_COUNT_TRAVERSAL, 1)
    render_and_compare(pt, name, "counting")
    assert pt.stats()["nodeVisits"] > 0


@pytest.mark.parametrize("sky_rect", [0, 1])
@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_sky_rectangle_on_and_off(pt, name, sky_rect):
    pt.setOption(hippt.OPT_SKY_RECT, sky_rect)
    render_and_compare(pt, name, f"sky rectangle {sky_rect}")


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_chained_async_frames_match_the_render_reference(pt, name):
    pt.setOption(hippt.OPT_CHAIN, 8)
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    hippt.chain_audit()  # (drops records of earlier tests)
    render_and_compare(pt, name, "three chained async frames", chained=True)
    runs = hippt.chain_audit()
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 0)
    problems = chain_audit.check(runs)
    assert runs and not problems, problems[:6]


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_wavefront_matches_the_render_reference(pt, name):
    pt.setOption(hippt.OPT_PATH_MODE, 1)
    render_and_compare(pt, name, "wavefront")


def test_cpp_host_emit_option_renders_the_lit_mesh(tmp_path):
    """hippt_render --emit: the OBJ's `usemtl` group of the lamp made emissive by HipPathTracer::loadMeshFile."""
    name = "cornell34_lit_tris"
    sc, acc, px = er.render_case(name)[:3]
    obj, out = tmp_path / "lit.obj", tmp_path / "frame.bin"
    scenes.write_obj(sc, str(obj), style="plain")  # groups m0..m3 in order of first use: the materials' order
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    r = subprocess.run([exe, "--mesh", str(obj), "--albedo", albedo, "--emit", "m3=15,15,15", "--width", str(W),
                        "--height", str(H), "--spp", str(FRAMES), "--depth", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(str(out), "<u4").reshape(H, W), px)


# ---- 3. animated mesh: the refit keeps the material word ---------------------------------------------
@pytest.mark.parametrize("move", ["shift", "wobble"])
def test_radiance_follows_a_vertex_update(pt, move):
    sc, rays, seeds, rad0, segs0 = er.emit_case("cornell_mixed_lit")[:5]
    n = N - degenerate_rays().shape[0]
    rays, seeds = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n])
    upload(pt, sc)
    # a small uniform shift of every triangle (the spheres stay), or refit_util's deformation
    v1 = np.ascontiguousarray(verts_of(sc) + np.float32(3.0)) if move == "shift" else wobble(verts_of(sc))
    pt.updateVertices(v1)
    sc1 = with_verts(sc, v1)
    rad, segs, ends, _ = er.EmitRef(sc1, Ref(sc1)).paths(rays, seeds, 8)
    # conditions on the reference alone: the update changes what paths return (a shift keeps every normal,
    # and a Lambertian bounce's direction does not depend on where it happens: far fewer paths change than
    # under the deformation, which changes most), and paths still end on the moved lamp and on the sphere
    assert np.count_nonzero((rad != rad0[:n]).any(axis=1)) > (n // 8 if move == "shift" else n // 2)
    assert np.count_nonzero(ends == er.EMITTED) >= 100
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, "after updateVertices")


# ---- 4. the denoiser -------------------------------------------------------------------------------
def test_denoise_matches_the_model(pt):
    name = "cornell_mixed_lit"
    sc, acc, px = er.render_case(name)[:3]
    render_and_compare(pt, name, "before the denoiser")
    g0 = dr.guides(sc, W, H, 0)
    mats = sc.materials()
    # conditions on the model alone: light pixels are in the image, and they are not demodulated
    m = np.where(g0["prim"] >= 0, g0["matFlags"] & hippt.HIT_MATERIAL_MASK, 0)
    light = (g0["prim"] >= 0) & (mats["kind"][m] == scenes.MAT_EMISSIVE)
    assert np.count_nonzero(light) >= 5 and np.all(dr.albedo_prime(g0, mats)[light] == 1.0)
    gpx, grgba = pt.denoise(passes=2)
    wpx, wrgba = dr.denoise(np.array(acc), g0, mats, passes=2)
    assert gpx.dtype == np.uint32 and grgba.dtype == np.float32 and grgba.shape == wrgba.shape
    bad = np.argwhere((grgba.view(np.uint32) != wrgba.view(np.uint32)).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} of {W * H} pixels differ, first (y, x) {bad[:4].tolist()}"
    assert np.array_equal(gpx, wpx)
    # the guide buffer's albedo of a light is its emission
    g = pt.gbuffer(0)
    assert np.array_equal(g["material"], np.where(g0["prim"] >= 0, m, -1))
    assert g["albedo"][light].tobytes() == mats["albedo"][m[light]].tobytes() and float(g["albedo"][light].max()) == 15.0
