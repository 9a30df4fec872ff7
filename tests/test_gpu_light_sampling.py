"""Light sampling (GPU): HIPPT_OPT_LIGHT_SAMPLING in hipptTraceRadiance and the render calls against the reference
of tests/nee_ref.py, bit for bit, and the estimator's expectation and variance against the option-off paths.

The reference is emit_ref.EmitRef with the light-sampling rule (pinned by tests/test_nee_ref_cpu.py, which also
asserts on the reference alone that the ray sets meet every case of the rule).  Every comparison but the last
test's is exact: the radiance words and segment counts of every ray, the accumulation's bytes, the pixel words
and the segment totals.  A scene's rays, seeds and references are computed once and shared by its tests."""
import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import emit_ref as er
import hippt
import nee_ref as nr
import path_ref as pr
from refit_util import verts_of, with_verts, wobble
from test_gpu_ray_query import N, Ref, degenerate_rays, upload

pytestmark = pytest.mark.gpu

W, H, FRAMES = 32, 24, 3
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_SKY_RECT, 1),
        (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB), (hippt.OPT_LIGHT_SAMPLING, 0))


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


def info(key):
    return int(hippt.load_library().hipptGetOption(key))


# ---- 1. traceRadiance against the reference ---------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", list(er.LIT))
def test_radiance_and_segments_match_the_reference(pt, name, lds, width):
    sc, rays, seeds, rad, segs = nr.nee_case(name)[:5]
    upload(pt, sc, lds, width)
    for n in (1, 65, N):
        got, gs = pt.traceRadiance(np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n]), 8)
        pr.assert_paths(got, gs, rad[:n], segs[:n], f"{name} lds={lds} width={width} n={n}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depth_limits(pt, depth):
    sc, rays, seeds, rad, segs = nr.nee_case("cornell_mixed_lit", depth)[:5]
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, depth)
    pr.assert_paths(got, gs, rad, segs, f"maxDepth {depth}")


def test_device_memory_gives_the_same_bytes(pt):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs = nr.nee_case("cornell_mixed_lit")[:5]
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
def assert_image(got, want, what):
    (gpx, gacc), (px, acc) = got, want
    bad = np.argwhere((gacc.view(np.uint32) != acc.view(np.uint32)).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} of {gacc.shape[0] * gacc.shape[1]} pixels differ, first (y, x) " \
                          f"{bad[:4].tolist()}: {gacc[tuple(bad[0])]} vs {acc[tuple(bad[0])]}"
    assert gacc.tobytes() == acc.tobytes() and np.array_equal(gpx, px), what


def render_and_compare(pt, name, what, asynchronous=False):
    sc, acc, px, total, shadow = nr.render_case(name)
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
    assert info(hippt.INFO_LIGHT_SAMPLING) == 1
    assert info(hippt.INFO_CHAIN_CAP) == 0 and info(hippt.INFO_RENDER_PAD) == 0 and info(hippt.INFO_SKY_RECT_PIXELS) == 0


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", list(er.LIT))
def test_blocking_render_matches_the_render_reference(pt, name, lds, width):
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    render_and_compare(pt, name, f"lds={lds} width={width}")
    # the blocking call's host frame is the image too
    assert np.array_equal(pt.hostPixels(), nr.render_case(name)[2])


@pytest.mark.parametrize("name", list(er.LIT))
def test_three_asynchronous_single_frames_match_the_render_reference(pt, name):
    render_and_compare(pt, name, "three asynchronous frames", asynchronous=True)


def test_a_query_between_asynchronous_frames_leaves_them_alone(pt):
    """The route's counters and spill area are its own: a path query made while frames are in flight (it
    grows the queries' spill area on first use) neither waits for them nor changes what they render."""
    name = "cornell_mixed_lit"
    sc, acc, px, total = nr.render_case(name)[:4]
    _, rays, seeds, rad, segs = nr.nee_case(name)[:5]
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    for f in range(FRAMES):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
        if f == 0:
            got, gs = pt.traceRadiance(rays[:257], seeds[:257], 8)
            pr.assert_paths(got, gs, rad[:257], segs[:257], "query between frames")
    assert pt.synchronize(), pt.lastError()
    assert_image(pt.readback(), (px, acc), "frames around a query")
    assert pt.stats()["segments"] == total


@pytest.mark.parametrize("name", ["cornell_mixed_lit"])
def test_two_row_ranges_give_the_whole_image(pt, name):
    sc, acc, px = nr.render_case(name)[:3]
    pt.uploadMesh(sc)
    for y0, y1 in ((0, 11), (11, H)):
        pt.setRowRange(y0, y1)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert_image(pt.readback(y0, y1), (px[y0:y1], acc[y0:y1]), f"{name} rows {y0}..{y1}")
    pt.setRowRange(0, 0)


def test_row_interleave_gives_the_whole_image(pt):
    name = "cornell34_lit"
    sc, acc, px = nr.render_case(name)[:3]
    pt.uploadMesh(sc)
    for phase in (0, 1):
        pt.setRowInterleave(phase, 2)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        gpx, gacc = pt.readback()
        assert_image((gpx[phase::2], gacc[phase::2]), (px[phase::2], acc[phase::2]), f"{name} rows {phase}::2")
    pt.setRowInterleave(0, 1)


def test_two_contexts_on_one_device_give_the_whole_image(pt):
    """The several-devices path (each context its rows, its own counters and spill area), on one GPU."""
    name = "cornell_mixed_lit"
    sc, acc, px, total, shadow = nr.render_case(name)
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
    pt.setDevices([])


def test_present_frames_match_the_render_reference(pt):
    name = "cornell34_lit"
    sc, acc, px = nr.render_case(name)[:3]
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    for _ in range(FRAMES):
        assert pt.renderFramesPresent(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    frame, n = pt.latestFrame()
    assert n == FRAMES and np.array_equal(frame, px)
    assert_image(pt.readback(), (px, acc), f"{name} present")


def test_cpp_host_light_sampling_flag_renders_the_reference(tmp_path):
    """hippt_render --emit ... --light-sampling: the option through the C++ host and the CLI."""
    import os
    import subprocess

    from hippt import scenes
    name = "cornell34_lit_tris"
    sc, acc, px = nr.render_case(name)[:3]
    obj, out = tmp_path / "lit.obj", tmp_path / "frame.bin"
    scenes.write_obj(sc, str(obj), style="plain")  # groups m0..m3 in order of first use: the materials' order
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    r = subprocess.run([exe, "--mesh", str(obj), "--albedo", albedo, "--emit", "m3=15,15,15", "--light-sampling",
                        "--width", str(W), "--height", str(H), "--spp", str(FRAMES), "--depth", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(str(out), "<u4").reshape(H, W), px)
    assert not np.array_equal(px, er.render_case(name)[2])  # (the option-off image is another one)


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_camera_rays_through_the_path_query_are_the_renders_samples(pt, name):
    """traceRadiance(cameraRays(f)) is sample f of the render: fed through the oracle's accumulation, the
    three samples give the render's bytes."""
    import ctypes

    import pyoracle as po
    sc, acc, px = nr.render_case(name)[:3]
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
    sc, rays, seeds = nr.nee_case("cornell_mixed_lit")[:3]
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
    # the update moves the lamp and changes what most paths return; the light list needs no rebuild
    assert np.count_nonzero((got != before).any(axis=1)) > n // 2
    pr.assert_paths(got, gs, want, ws, "after updateVertices")
    assert_image(img, fresh, "render after updateVertices")
    # and the fresh upload is the reference's (the first 513 rays: the reference is per ray, in Python)
    rad, segs, _, _ = nr.NeeRef(sc1, Ref(sc1)).paths(rays[:513], seeds[:513], 8)
    pr.assert_paths(want[:513], ws[:513], rad, segs, "fresh upload of the moved scene")


# ---- 4. the option ---------------------------------------------------------------------------------------
def test_option_off_after_on_gives_the_parents_bytes(pt):
    name = "cornell_mixed_lit"
    sc, rays, seeds, rad, segs = er.emit_case(name)[:5]
    _, acc, px, total = er.render_case(name)[:4]
    nrad, nsegs = nr.nee_case(name)[3:5]
    upload(pt, sc, w=W, h=H)
    assert info(hippt.INFO_LIGHTS) == 3
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, nrad, nsegs, "option on")
    assert pt.renderFrames(1, 8), pt.lastError()
    assert info(hippt.INFO_LIGHT_SAMPLING) == 1
    pt.setOption(hippt.OPT_LIGHT_SAMPLING, 0)  # takes effect at the next call, without a new upload
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, "option off after on")
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert info(hippt.INFO_LIGHT_SAMPLING) == 0
    assert_image(pt.readback(), (px, acc), "render with the option off after on")
    assert pt.stats()["segments"] == total
    # and on again
    pt.setOption(hippt.OPT_LIGHT_SAMPLING, 1)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, nrad, nsegs, "option on again")


@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_option_on_without_a_light_gives_path_refs_bytes(pt, name):
    sc, rays, seeds, rad, segs = pr.path_case(name)[:5]
    upload(pt, sc, w=W, h=H)
    assert info(hippt.INFO_LIGHTS) == 0
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name}: option on, no light")
    _, acc, px, total = er.render_case(name)[:4]  # (without a light EmitRef's render is the oracle's)
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert info(hippt.INFO_LIGHT_SAMPLING) == 0
    assert_image(pt.readback(), (px, acc), f"{name}: render with the option on, no light")
    assert pt.stats()["segments"] == total


# ---- 5. same expectation, less noise --------------------------------------------------------------------
def test_same_expectation_and_less_noise(pt):
    """cornell34_lit_tris, 32x24, depth 8, 256 frames through cameraRays + traceRadiance, option off and on.  Per
    channel the two overall means differ by at most 5 standard errors of their difference (each standard error
    from the 256 per-frame image means themselves), and the mean per-pixel sample variance is lower with the
    option on."""
    frames = 256
    sc = er.lit_scene("cornell34_lit_tris")
    dev = torch.device("cuda", 0)
    pt.setDevices([0])
    upload(pt, sc, w=W, h=H)
    samples = {}
    for on in (0, 1):
        pt.setOption(hippt.OPT_LIGHT_SAMPLING, on)
        out = torch.empty((frames, H * W, 3), dtype=torch.float64, device=dev)
        for f in range(frames):
            rays, seeds = pt.cameraRays(f, device=True)
            rad, _ = pt.traceRadiance(rays, seeds, 8)
            out[f] = rad[:, :3].double()
        samples[on] = out.cpu().numpy()
    pt.setDevices([])
    for c, channel in enumerate("rgb"):
        off, on = samples[0][:, :, c], samples[1][:, :, c]
        m_off, m_on = off.mean(axis=1), on.mean(axis=1)  # the per-frame image means
        se_off = m_off.std(ddof=1) / np.sqrt(frames)
        se_on = m_on.std(ddof=1) / np.sqrt(frames)
        diff = abs(m_off.mean() - m_on.mean())
        bound = 5.0 * np.sqrt(se_off ** 2 + se_on ** 2)
        v_off, v_on = off.var(axis=0, ddof=1).mean(), on.var(axis=0, ddof=1).mean()
        print(f"{channel}: mean off {m_off.mean():.6f} (se {se_off:.6f}), on {m_on.mean():.6f} (se {se_on:.6f}), "
              f"difference {diff:.6f} <= {bound:.6f}; mean per-pixel variance off {v_off:.5f}, on {v_on:.5f}")
        assert diff <= bound, (channel, diff, bound)
        assert v_on < v_off, (channel, v_on, v_off)
