"""Light sampling with MIS (GPU): HIPPT_OPT_LIGHT_SAMPLING_MODE = HIPPT_LIGHT_SAMPLING_MIS in hipptTraceRadiance and the
render calls against the reference of tests/mis_ref.py, bit for bit; the near-field scene's bound; and the
estimator's expectation and variance against the option-off paths.

The reference is nee_ref.NeeRef with the power heuristic (pinned by tests/test_mis_ref_cpu.py, which also asserts
on the reference alone that the ray sets meet every case of the rule).  Every comparison but the last test's is
exact.  A scene's rays, seeds and references are computed once and shared by its tests."""
import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import emit_ref as er
import hippt
import lit_scenes as ls
import mis_ref as mr
import mis_scenes as ms
import nee_ref as nr
import path_ref as pr
from refit_util import verts_of, with_verts, wobble
from test_gpu_light_sampling import FRAMES, OPTS, H, W, assert_image, info
from test_gpu_ray_query import N, Ref, degenerate_rays, upload

pytestmark = pytest.mark.gpu

MIS = 2


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    for k, v in OPTS:
        t.setOption(k, v)
    t.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, MIS)
    yield t
    for k, v in OPTS:
        t.setOption(k, v)
    hippt.load_library().cudaPathTracerShutdown()


# ---- 1. traceRadiance against the reference ---------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", list(er.LIT) + list(ls.SETS))
def test_radiance_and_segments_match_the_reference(pt, name, lds, width):
    sc, rays, seeds, rad, segs = mr.mis_case(name)[:5]
    upload(pt, sc, lds, width)
    for n in (1, 65, len(rays)):
        got, gs = pt.traceRadiance(np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n]), 8)
        pr.assert_paths(got, gs, rad[:n], segs[:n], f"{name} lds={lds} width={width} n={n}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depth_limits(pt, depth):
    sc, rays, seeds, rad, segs = mr.mis_case("cornell_mixed_lit", depth)[:5]
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, depth)
    pr.assert_paths(got, gs, rad, segs, f"maxDepth {depth}")


def test_device_memory_gives_the_same_bytes(pt):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs = mr.mis_case("cornell_mixed_lit")[:5]
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


# ---- 2. the render route ------------------------------------------------------------------------------
def render_and_compare(pt, name, what, asynchronous=False):
    sc, acc, px, total, shadow = mr.render_case(name)
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    if asynchronous:
        for _ in range(FRAMES):
            assert pt.renderFramesAsync(1, 8), pt.lastError()
        assert pt.synchronize(), pt.lastError()
    else:
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert_image(pt.readback(), (px, acc), f"{name} {what}")
    st = pt.stats()
    assert st["segments"] == total and st["pixelSamples"] == W * H * FRAMES, f"{name} {what}"
    assert 0 < shadow < total and pt.counters()["shadow_rays"] == shadow, f"{name} {what}"
    assert info(hippt.INFO_LIGHT_SAMPLING) == MIS
    assert info(hippt.INFO_CHAIN_CAP) == 0 and info(hippt.INFO_RENDER_PAD) == 0 and info(hippt.INFO_SKY_RECT_PIXELS) == 0


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", list(er.LIT))
def test_blocking_render_matches_the_render_reference(pt, name, lds, width):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    render_and_compare(pt, name, f"lds={lds} width={width}")
    assert np.array_equal(pt.hostPixels(), mr.render_case(name)[2])


@pytest.mark.parametrize("name", list(er.LIT))
def test_three_asynchronous_single_frames_match_the_render_reference(pt, name):
    render_and_compare(pt, name, "three asynchronous frames", asynchronous=True)


def test_the_render_is_another_image_than_option_1s():
    """Conditions on the references alone: the MIS render differs from the plain light-sampling render."""
    for name in er.LIT:
        assert not np.array_equal(mr.render_case(name)[1], nr.render_case(name)[1])


def test_two_row_ranges_give_the_whole_image(pt):
    name = "cornell_mixed_lit"
    sc, acc, px = mr.render_case(name)[:3]
    pt.uploadMesh(sc)
    for y0, y1 in ((0, 11), (11, H)):
        pt.setRowRange(y0, y1)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert_image(pt.readback(y0, y1), (px[y0:y1], acc[y0:y1]), f"{name} rows {y0}..{y1}")
    pt.setRowRange(0, 0)


def test_row_interleave_gives_the_whole_image(pt):
    name = "cornell34_lit"
    sc, acc, px = mr.render_case(name)[:3]
    pt.uploadMesh(sc)
    for phase in (0, 1):
        pt.setRowInterleave(phase, 2)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        gpx, gacc = pt.readback()
        assert_image((gpx[phase::2], gacc[phase::2]), (px[phase::2], acc[phase::2]), f"{name} rows {phase}::2")
    pt.setRowInterleave(0, 1)


def test_two_contexts_on_one_device_give_the_whole_image(pt):
    name = "cornell_mixed_lit"
    sc, acc, px, total, shadow = mr.render_case(name)
    pt.setDevices([0, 0])
    pt.setOption(hippt.OPT_BVH_WIDTH, 4)
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    for _ in range(FRAMES):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    assert_image(pt.readback(), (px, acc), f"{name} two contexts")
    assert pt.stats()["segments"] == total and pt.counters()["shadow_rays"] == shadow
    assert info(hippt.INFO_LIGHT_SAMPLING) == MIS
    pt.setDevices([])


def test_present_frames_match_the_render_reference(pt):
    name = "cornell34_lit"
    sc, acc, px = mr.render_case(name)[:3]
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    for _ in range(FRAMES):
        assert pt.renderFramesPresent(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    frame, n = pt.latestFrame()
    assert n == FRAMES and np.array_equal(frame, px)
    assert_image(pt.readback(), (px, acc), f"{name} present")


def test_cpp_host_mis_flag_renders_the_reference(tmp_path):
    """hippt_render --emit ... --mis: the option's value through the C++ host and the CLI; it implies light
    sampling."""
    import os
    import subprocess

    from hippt import scenes
    name = "cornell34_lit_tris"
    sc, acc, px = mr.render_case(name)[:3]
    obj, out = tmp_path / "lit.obj", tmp_path / "frame.bin"
    scenes.write_obj(sc, str(obj), style="plain")  # groups m0..m3 in order of first use: the materials' order
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    r = subprocess.run([exe, "--mesh", str(obj), "--albedo", albedo, "--emit", "m3=15,15,15", "--mis",
                        "--width", str(W), "--height", str(H), "--spp", str(FRAMES), "--depth", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(str(out), "<u4").reshape(H, W), px)
    assert not np.array_equal(px, nr.render_case(name)[2])  # (option 1's image is another one)


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_camera_rays_through_the_path_query_are_the_renders_samples(pt, name):
    import ctypes

    import pyoracle as po
    sc, acc, px = mr.render_case(name)[:3]
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    L = po.lib()
    PF = ctypes.POINTER(ctypes.c_float)
    a = np.zeros((H * W, 4), np.float32)
    words = np.zeros(H * W, np.uint32)
    for f in range(FRAMES):
        rays, seeds = pt.cameraRays(f)
        rad, _ = pt.traceRadiance(rays, seeds, 8)
        rgb = np.ascontiguousarray(rad[:, :3])
        for i in range(H * W):
            words[i] = L.po_accumulate(a[i].ctypes.data_as(PF), rgb[i].ctypes.data_as(PF), f)
    assert a.reshape(H, W, 4).tobytes() == acc.tobytes() and np.array_equal(words.reshape(H, W), px)


# ---- 3. animated mesh ------------------------------------------------------------------------------------
def test_results_after_a_vertex_update_equal_a_fresh_upload(pt):
    sc, rays, seeds = mr.mis_case("cornell_mixed_lit")[:3]
    n = N - degenerate_rays().shape[0]
    rays, seeds = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n])
    v1 = wobble(verts_of(sc))
    sc1 = with_verts(sc, v1)
    upload(pt, sc)
    before, _ = pt.traceRadiance(rays, seeds, 8)
    pt.updateVertices(v1)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    img = pt.readback()
    upload(pt, sc1)
    want, ws = pt.traceRadiance(rays, seeds, 8)
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    fresh = pt.readback()
    assert np.count_nonzero((got != before).any(axis=1)) > n // 2
    pr.assert_paths(got, gs, want, ws, "after updateVertices")
    assert_image(img, fresh, "render after updateVertices")
    # and the fresh upload is the reference's (the first 513 rays: the reference is per ray, in Python)
    rad, segs, _, _ = mr.MisRef(sc1, Ref(sc1)).paths(rays[:513], seeds[:513], 8)
    pr.assert_paths(want[:513], ws[:513], rad, segs, "fresh upload of the moved scene")


# ---- 4. the option ---------------------------------------------------------------------------------------
def test_switching_2_1_0_2_gives_each_modes_bytes(pt):
    name = "cornell_mixed_lit"
    sc, rays, seeds = er.emit_case(name)[:3]
    want = {2: mr.mis_case(name)[3:5], 1: nr.nee_case(name)[3:5], 0: er.emit_case(name)[3:5]}
    images = {2: mr.render_case(name), 1: nr.render_case(name), 0: er.render_case(name)}
    upload(pt, sc, w=W, h=H)
    assert info(hippt.INFO_LIGHTS) == 3
    for mode in (2, 1, 0, 2):
        pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)  # takes effect at the next call, without a new upload
        assert info(hippt.OPT_LIGHT_SAMPLING_MODE) == mode
        got, gs = pt.traceRadiance(rays, seeds, 8)
        pr.assert_paths(got, gs, want[mode][0], want[mode][1], f"option {mode}")
        assert pt.initialize(W, H), pt.lastError()
        pt.resetStats()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert info(hippt.INFO_LIGHT_SAMPLING) == mode
        _, acc, px, total = images[mode][:4]
        assert_image(pt.readback(), (px, acc), f"render with option {mode}")
        assert pt.stats()["segments"] == total


@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_option_2_without_a_light_gives_path_refs_bytes(pt, name):
    sc, rays, seeds, rad, segs = pr.path_case(name)[:5]
    upload(pt, sc, w=W, h=H)
    assert info(hippt.INFO_LIGHTS) == 0 and info(hippt.OPT_LIGHT_SAMPLING_MODE) == MIS
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name}: option 2, no light")
    _, acc, px, total = er.render_case(name)[:4]  # (without a light EmitRef's render is the oracle's)
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert info(hippt.INFO_LIGHT_SAMPLING) == 0
    assert_image(pt.readback(), (px, acc), f"{name}: render with option 2, no light")
    assert pt.stats()["segments"] == total


# ---- 5. the near field ---------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
def test_near_field_bytes_and_bound(pt, lds, width):
    sc = ms.scene_refs()[0]
    rays, seeds = ms.rays_seeds()
    rad, segs = ms.case(True)[:2]
    upload(pt, sc, lds, width)
    got, gs = pt.traceRadiance(rays, seeds, ms.MAX_DEPTH)
    pr.assert_paths(got, gs, rad, segs, f"near field lds={lds} width={width}")
    print(f"near field, option 2: largest channel {float(got[:, :3].max()):.4f}, bound {ms.BOUND:.4f}")
    assert float(got[:, :3].max()) <= ms.BOUND
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 1)
    got1, gs1 = pt.traceRadiance(rays, seeds, ms.MAX_DEPTH)
    nrad, nsegs = ms.case(False)[:2]
    pr.assert_paths(got1, gs1, nrad, nsegs, f"near field, option 1, lds={lds} width={width}")
    above = int(np.count_nonzero(got1[:, :3].max(axis=1) > ms.BOUND))
    print(f"near field, option 1: {above} of {len(rays)} paths above the bound, largest {float(got1[:, :3].max()):.1f}")
    assert above >= len(rays) // 100 + 1


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
def test_hits_that_count_whole_under_the_huge_lamp(pt, lds, width):
    """wb = 1 after a Lambertian vertex (gh^2 overflows): 61 of the 128 paths; 67 end on a weighted hit."""
    sc, rays, seeds, rad, segs = ms.huge_case()[:5]
    upload(pt, sc, lds, width)
    got, gs = pt.traceRadiance(rays, seeds, ms.MAX_DEPTH)
    pr.assert_paths(got, gs, rad, segs, f"huge lamp lds={lds} width={width}")


# ---- 6. same expectation, less noise --------------------------------------------------------------------
def test_same_expectation_and_less_noise_than_option_off(pt):
    """cornell34_lit_tris, 32x24, depth 8, 256 frames through cameraRays + traceRadiance, options 0 and 2.  Per
    channel the two overall means differ by at most 5 standard errors of their difference (each standard error
    from the 256 per-frame image means themselves), and the mean per-pixel sample variance is lower with option
    2.  (2 against 1 is not asserted on this scene: the near-field scene tests that.)"""
    frames = 256
    sc = er.lit_scene("cornell34_lit_tris")
    dev = torch.device("cuda", 0)
    pt.setDevices([0])
    upload(pt, sc, w=W, h=H)
    samples = {}
    for mode in (0, MIS):
        pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
        out = torch.empty((frames, H * W, 3), dtype=torch.float64, device=dev)
        for f in range(frames):
            rays, seeds = pt.cameraRays(f, device=True)
            rad, _ = pt.traceRadiance(rays, seeds, 8)
            out[f] = rad[:, :3].double()
        samples[mode] = out.cpu().numpy()
    pt.setDevices([])
    for c, channel in enumerate("rgb"):
        off, on = samples[0][:, :, c], samples[MIS][:, :, c]
        m_off, m_on = off.mean(axis=1), on.mean(axis=1)  # the per-frame image means
        se_off = m_off.std(ddof=1) / np.sqrt(frames)
        se_on = m_on.std(ddof=1) / np.sqrt(frames)
        diff = abs(m_off.mean() - m_on.mean())
        bound = 5.0 * np.sqrt(se_off ** 2 + se_on ** 2)
        v_off, v_on = off.var(axis=0, ddof=1).mean(), on.var(axis=0, ddof=1).mean()
        print(f"{channel}: mean 0 {m_off.mean():.6f} (se {se_off:.6f}), 2 {m_on.mean():.6f} (se {se_on:.6f}), "
              f"difference {diff:.6f} <= {bound:.6f}; mean per-pixel variance 0 {v_off:.5f}, 2 {v_on:.5f}")
        assert diff <= bound, (channel, diff, bound)
        assert v_on < v_off, (channel, v_on, v_off)
