"""Light selection by power (GPU): HIPPT_OPT_LIGHT_SELECT = HIPPT_LIGHT_SELECT_POWER.  The table the device builds
against tests/select_ref.py word for word; hipptTraceRadiance and the render route against its references bit for
bit (pinned by tests/test_select_ref_cpu.py, which also asserts that the ray sets meet every case of the rule); the
table behind vertex updates in stream order; switching the option; and the estimator's expectation and noise
against the uniform choice.  Every comparison but the last test's is exact.  A scene's rays, seeds and references
are computed once and shared by its tests."""
import os
import subprocess

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import hippt
import mis_ref as mr
import path_ref as pr
import select_ref as sr
import select_scenes as ss
from hippt import scenes
from refit_util import verts_of, with_verts, wobble
from test_gpu_light_sampling import FRAMES, OPTS, H, W, assert_image, info
from test_gpu_ray_query import Ref, upload

pytestmark = pytest.mark.gpu

POWER = hippt.LIGHT_SELECT_POWER


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    for k, v in OPTS:
        t.setOption(k, v)
    t.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 2)
    t.setOption(hippt.OPT_LIGHT_SELECT, POWER)
    yield t
    for k, v in OPTS:
        t.setOption(k, v)
    t.setOption(hippt.OPT_LIGHT_SELECT, 0)
    hippt.load_library().cudaPathTracerShutdown()


def assert_table(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    for field in ("prim", "q", "c"):
        bad = np.flatnonzero(got[field] != want[field])
        assert bad.size == 0, f"{what}: {field} differs at {bad[:4].tolist()}: {got[field][bad[:4]]} vs {want[field][bad[:4]]}"
    assert got["ip"].tobytes() == want["ip"].tobytes(), what
    assert got.tobytes() == want.tobytes(), what


# ---- 1. the table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 65537])
def test_the_devices_table_is_the_references_word_for_word(pt, n):
    sc = ss.many_lights(n)
    want = sr.table(sc)
    assert len(want) == n
    upload(pt, sc, w=W, h=H)
    assert info(hippt.INFO_LIGHTS) == n
    assert_table(pt.lightTable(), want, f"{n} lights")
    raw = hippt.scene_download(hippt.SCENE_LIGHTS)
    assert raw.shape == (n, 4) and raw.dtype == np.uint32


@pytest.mark.parametrize("name", ["uneven_lamps", "all_unlit", "light_edges", "blob64x34_lit"])
def test_the_tables_of_the_test_scenes(pt, name):
    sc = sr.scene_refs(name)[0]
    upload(pt, sc, w=W, h=H)
    assert_table(pt.lightTable(), sr.table(sc), name)


def test_no_table_without_lights(pt):
    upload(pt, scenes.cornell34(), w=W, h=H)
    tab = pt.lightTable()
    assert tab.shape == (0,) and tab.dtype == hippt.LIGHT_TABLE_DTYPE


# ---- 2. traceRadiance against the reference ---------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["uneven_lamps", "light_edges", "blob64x34_lit"])
def test_radiance_and_segments_match_the_reference(pt, name, mode, lds, width):
    sc, rays, seeds, rad, segs = sr.case(name, mode)[:5]
    assert len(rays) <= 1025
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    upload(pt, sc, lds, width)
    for n in (1, 65, len(rays)):
        got, gs = pt.traceRadiance(np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n]), 8)
        pr.assert_paths(got, gs, rad[:n], segs[:n], f"{name} mode={mode} lds={lds} width={width} n={n}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()


@pytest.mark.parametrize("mode", [1, 2])
def test_device_memory_gives_the_same_bytes(pt, mode):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs = sr.case("uneven_lamps", mode)[:5]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
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


# ---- 3. trivial tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_one_light_gives_the_uniform_options_bytes(pt, mode):
    sc, rays, seeds, rad, segs = sr.case("light_edges_one", mode)[:5]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pt.setOption(hippt.OPT_LIGHT_SELECT, 0)
    uni, us = pt.traceRadiance(rays, seeds, 8)
    assert got.tobytes() == uni.tobytes() and gs.tobytes() == us.tobytes()
    pr.assert_paths(got, gs, rad, segs, f"light_edges_one mode={mode}")


@pytest.mark.parametrize("mode", [1, 2])
def test_a_scene_whose_lights_add_nothing_matches_the_reference(pt, mode):
    sc, rays, seeds, rad, segs = sr.case("all_unlit", mode)[:5]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    upload(pt, sc, w=W, h=H)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"all_unlit mode={mode}")
    pt.resetStats()
    assert pt.renderFrames(1, 8), pt.lastError()
    assert pt.counters()["shadow_rays"] == 0 and info(hippt.INFO_LIGHT_SELECT) == POWER


@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_without_a_light_the_option_changes_nothing(pt, name):
    sc, rays, seeds, rad, segs = pr.path_case(name)[:5]
    upload(pt, sc, w=W, h=H)
    assert info(hippt.INFO_LIGHTS) == 0 and info(hippt.OPT_LIGHT_SELECT) == POWER
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name}: selection on, no light")
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert info(hippt.INFO_LIGHT_SAMPLING) == 0 and info(hippt.INFO_LIGHT_SELECT) == 0


# ---- 4. the render route ------------------------------------------------------------------------------
def check_render(pt, name, mode, what, total=True):
    sc, acc, px, segs, shadow = sr.render_case(name, mode)
    assert_image(pt.readback(), (px, acc), f"{name} {what}")
    if total:
        st = pt.stats()
        assert st["segments"] == segs and st["pixelSamples"] == W * H * FRAMES, f"{name} {what}"
        assert 0 < shadow < segs and pt.counters()["shadow_rays"] == shadow, f"{name} {what}"
    assert info(hippt.INFO_LIGHT_SAMPLING) == mode and info(hippt.INFO_LIGHT_SELECT) == POWER


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("mode", [1, 2])
def test_blocking_render_matches_the_render_reference(pt, mode, lds, width):
    name = "uneven_lamps"
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    pt.setOption(hippt.OPT_LDS_SCENE, lds)
    pt.setOption(hippt.OPT_BVH_WIDTH, width)
    pt.uploadMesh(sr.render_case(name, mode)[0])
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    check_render(pt, name, mode, f"mode={mode} lds={lds} width={width}")
    assert np.array_equal(pt.hostPixels(), sr.render_case(name, mode)[2])


def test_three_asynchronous_single_frames_match_the_render_reference(pt):
    name = "uneven_lamps"
    pt.uploadMesh(sr.render_case(name, 2)[0])
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    for _ in range(FRAMES):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    check_render(pt, name, 2, "three asynchronous frames")


def test_two_row_ranges_give_the_whole_image(pt):
    name = "uneven_lamps"
    sc, acc, px = sr.render_case(name, 2)[:3]
    pt.uploadMesh(sc)
    for y0, y1 in ((0, 11), (11, H)):
        pt.setRowRange(y0, y1)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert_image(pt.readback(y0, y1), (px[y0:y1], acc[y0:y1]), f"{name} rows {y0}..{y1}")
        assert info(hippt.INFO_LIGHT_SELECT) == POWER
    pt.setRowRange(0, 0)


def test_two_contexts_on_one_device_give_the_whole_image(pt):
    name = "uneven_lamps"
    pt.setDevices([0, 0])
    pt.setOption(hippt.OPT_BVH_WIDTH, 4)
    pt.uploadMesh(sr.render_case(name, 2)[0])
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    for _ in range(FRAMES):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    check_render(pt, name, 2, "two contexts")
    pt.setDevices([])


def test_the_render_is_another_image_than_the_uniform_choices():
    """A condition on the references alone."""
    sc, acc = sr.render_case("uneven_lamps", 2)[:2]
    uni = sr.render(sr.scene_refs("uneven_lamps")[4], sc, W, H, FRAMES)[0]
    assert acc.tobytes() != uni.tobytes()


# ---- 5. vertex updates -------------------------------------------------------------------------------------
def moved(sc):
    """The scene's vertices wobbled, and the big lamp (the two triangles behind the box's twelve) scaled by 3
    about its centre."""
    v = wobble(verts_of(sc)).astype(np.float64)
    lamp = v[12:14].reshape(-1, 3)
    centre = lamp.mean(axis=0)
    v[12:14] = (centre + 3.0 * (lamp - centre)).reshape(2, 9)
    return np.ascontiguousarray(v, np.float32)


@pytest.mark.parametrize("device", [False, True])
def test_after_a_vertex_update_the_table_and_the_results_are_a_fresh_uploads(pt, device):
    sc, rays, seeds = sr.case("uneven_lamps", 2)[:3]
    rays, seeds = np.ascontiguousarray(rays[:513]), np.ascontiguousarray(seeds[:513])
    v1 = moved(sc)
    sc1 = with_verts(sc, v1)
    want_tab = sr.table(sc1)
    assert not np.array_equal(want_tab["q"], sr.table(sc)["q"])
    pt.setDevices([0])
    upload(pt, sc, w=W, h=H)
    before = pt.lightTable()
    dv = torch.from_numpy(v1.copy()).to(torch.device("cuda", 0)) if device else v1
    pt.updateVertices(dv)
    tab = pt.lightTable()
    got, gs = pt.traceRadiance(rays, seeds, 8)
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    img = pt.readback()
    upload(pt, sc1, w=W, h=H)
    fresh_tab = pt.lightTable()
    want, ws = pt.traceRadiance(rays, seeds, 8)
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    fresh = pt.readback()
    del dv
    pt.setDevices([])
    assert_table(before, sr.table(sc), "before the update")
    assert_table(tab, fresh_tab, "after updateVertices against a fresh upload")
    assert_table(tab, want_tab, "after updateVertices against the reference")
    pr.assert_paths(got, gs, want, ws, "after updateVertices")
    assert_image(img, fresh, "render after updateVertices")
    rad, segs = sr.SelectMisRef(sc1, Ref(sc1)).paths_events(rays[:257], seeds[:257], 8)[:2]
    pr.assert_paths(want[:257], ws[:257], rad, segs, "fresh upload of the moved scene")


def test_an_update_between_asynchronous_frames_is_in_stream_order(pt):
    sc, sel = sr.scene_refs("uneven_lamps")[0], sr.scene_refs("uneven_lamps")[2]
    v1 = moved(sc)
    sc1 = with_verts(sc, v1)
    acc = np.zeros((H * W, 4), np.float32)
    sr.render(sel, sc, W, H, 1, first=0, acc=acc)
    acc1, px1, _, _ = sr.render(sr.SelectMisRef(sc1, Ref(sc1)), sc1, W, H, 1, first=1, acc=acc)
    upload(pt, sc, w=W, h=H)
    assert pt.renderFramesAsync(1, 8), pt.lastError()
    pt.updateVertices(v1)  # no synchronise
    assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    assert_image(pt.readback(), (px1, acc1), "frame 0 on the old scene, frame 1 on the new one")


# ---- 6. the option ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_switching_1_0_1_gives_each_ones_bytes(pt, mode):
    name = "uneven_lamps"
    sc, rays, seeds = sr.case(name, mode)[:3]
    want = {1: sr.case(name, mode, 1)[3:5], 0: sr.case(name, mode, 0)[3:5]}
    refs = sr.scene_refs(name)
    images = {1: sr.render_case(name, mode)[1:3], 0: sr.render(refs[mode + 2], sc, W, H, FRAMES)[:2]}
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    upload(pt, sc, w=W, h=H)
    for select in (1, 0, 1):
        pt.setOption(hippt.OPT_LIGHT_SELECT, select)  # takes effect at the next call, without a new upload
        got, gs = pt.traceRadiance(rays, seeds, 8)
        pr.assert_paths(got, gs, want[select][0], want[select][1], f"mode {mode} selection {select}")
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert info(hippt.INFO_LIGHT_SAMPLING) == mode and info(hippt.INFO_LIGHT_SELECT) == select
        acc, px = images[select]
        assert_image(pt.readback(), (px, acc), f"render with mode {mode} selection {select}")


def test_with_light_sampling_off_the_option_changes_nothing(pt):
    import emit_ref as er
    sc, rays, seeds = sr.case("uneven_lamps", 2)[:3]
    rad, segs = er.EmitRef(sc, sr.scene_refs("uneven_lamps")[1].ref).paths(rays, seeds, 8)[:2]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 0)
    upload(pt, sc, w=W, h=H)
    out = {}
    for select in (1, 0):
        pt.setOption(hippt.OPT_LIGHT_SELECT, select)
        got, gs = pt.traceRadiance(rays, seeds, 8)
        pr.assert_paths(got, gs, rad, segs, f"mode 0 selection {select}")
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert info(hippt.INFO_LIGHT_SAMPLING) == 0 and info(hippt.INFO_LIGHT_SELECT) == 0
        out[select] = pt.readback()
    assert_image(out[1], out[0], "mode 0: selection 1 against 0")


# ---- 7. same expectation, less noise --------------------------------------------------------------------
def test_same_expectation_and_less_noise_than_the_uniform_choice(pt):
    """uneven_lamps, 32x24, depth 8, 256 frames through cameraRays + traceRadiance on the device, MIS with
    selection 0 against 1.  Per channel the two overall means differ by at most 5 standard errors of their
    difference (each standard error from the 256 per-frame image means themselves: test_gpu_mis.py's criterion),
    and the mean per-pixel sample variance is lower with 1."""
    frames = 256
    sc = sr.scene_refs("uneven_lamps")[0]
    dev = torch.device("cuda", 0)
    pt.setDevices([0])
    upload(pt, sc, w=W, h=H)
    samples = {}
    for select in (0, POWER):
        pt.setOption(hippt.OPT_LIGHT_SELECT, select)
        out = torch.empty((frames, H * W, 3), dtype=torch.float64, device=dev)
        for f in range(frames):
            rays, seeds = pt.cameraRays(f, device=True)
            rad, _ = pt.traceRadiance(rays, seeds, 8)
            out[f] = rad[:, :3].double()
        samples[select] = out.cpu().numpy()
    pt.setDevices([])
    for c, channel in enumerate("rgb"):
        off, on = samples[0][:, :, c], samples[POWER][:, :, c]
        m_off, m_on = off.mean(axis=1), on.mean(axis=1)  # the per-frame image means
        se_off = m_off.std(ddof=1) / np.sqrt(frames)
        se_on = m_on.std(ddof=1) / np.sqrt(frames)
        diff = abs(m_off.mean() - m_on.mean())
        bound = 5.0 * np.sqrt(se_off ** 2 + se_on ** 2)
        v_off, v_on = off.var(axis=0, ddof=1).mean(), on.var(axis=0, ddof=1).mean()
        print(f"{channel}: mean 0 {m_off.mean():.6f} (se {se_off:.6f}), 1 {m_on.mean():.6f} (se {se_on:.6f}), "
              f"difference {diff:.6f} <= {bound:.6f}; mean per-pixel variance 0 {v_off:.5f}, 1 {v_on:.5f}")
        assert diff <= bound, (channel, diff, bound)
        assert v_on < v_off, (channel, v_on, v_off)


# ---- 8. the command line ---------------------------------------------------------------------------------
def test_cpp_host_light_select_flag_renders_the_reference(tmp_path):
    """hippt_render --emit ... --mis --light-select power: the option through the C++ host and the CLI, on the
    Cornell box with the small dim lights (triangles only: an OBJ file holds no sphere)."""
    sc = scenes.cornell_lamps("cornell34", sphere=False)
    ref = Ref(sc)
    acc, px = sr.render(sr.SelectMisRef(sc, ref), sc, W, H, FRAMES)[:2]
    uni = sr.render(mr.MisRef(sc, ref), sc, W, H, FRAMES)[1]
    assert not np.array_equal(px, uni)  # (the uniform choice's image is another one)
    obj, out = tmp_path / "lamps.obj", tmp_path / "frame.bin"
    scenes.write_obj(sc, str(obj), style="plain")  # groups m0.. in order of first use: the materials' order
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    emit = ";".join(f"m{m}=" + ",".join(f"{c:.9g}" for c in sc.albedo[m])
                    for m in np.flatnonzero(np.asarray(sc.mat_kind) == scenes.MAT_EMISSIVE))
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    r = subprocess.run([exe, "--mesh", str(obj), "--albedo", albedo, "--emit", emit, "--mis", "--light-select", "power",
                        "--width", str(W), "--height", str(H), "--spp", str(FRAMES), "--depth", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(str(out), "<u4").reshape(H, W), px)
    bad = subprocess.run([exe, "--light-select", "brightest"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2
