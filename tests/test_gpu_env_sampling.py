"""Environment sampling (GPU): HIPPT_OPT_ENV_SAMPLING in hipptTraceRadiance and the render calls against the
references of tests/envs_ref.py, bit for bit, and the device-built selection table against envs_ref.table, word for
word.

tests/test_envs_ref_cpu.py pins the header's arithmetic to the restatement and asserts on the references alone that
these ray sets meet every case of the rule.  Every comparison but the last test's statistics is exact."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import env_ref as ev
import envs_ref as es
import hippt
import mis_ref as mr
import nee_ref as nr
import path_ref as pr
import select_ref as sr
from hippt import scenes
from test_gpu_ray_query import upload

pytestmark = pytest.mark.gpu

F = np.float32
W, H, FRAMES = 32, 24, 3
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_SKY_RECT, 1),
        (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB), (hippt.OPT_LIGHT_SAMPLING_MODE, 0), (hippt.OPT_LIGHT_SELECT, 0),
        (hippt.OPT_ENV_SAMPLING, 0))
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "qt-raytracer_amd", "hippt_render")


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    for k, v in OPTS:
        t.setOption(k, v)
    t.setEnvironment(None)
    yield t
    t.setEnvironment(None)  # later files see the gradient
    for k, v in OPTS:
        t.setOption(k, v)
    t.setDevices([])
    t.setRowRange(0, 0)
    hippt.load_library().cudaPathTracerShutdown()


def info(key):
    return int(hippt.load_library().hipptGetOption(key))


def sampling(pt, mode, select=False, on=1):
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    pt.setOption(hippt.OPT_LIGHT_SELECT, hippt.LIGHT_SELECT_POWER if select else 0)
    pt.setOption(hippt.OPT_ENV_SAMPLING, on)


def assert_table(got, want, what):
    assert got is not None, what
    for part in ("rows", "texels"):
        g, w = got[part], want[part]
        assert g.shape == w.shape, (what, part)
        for name in w.dtype.names:
            a, b = np.ascontiguousarray(g[name]).view(np.uint32), np.ascontiguousarray(w[name]).view(np.uint32)
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"{what}: {part}.{name} differs in {len(bad)} words, first at {bad[0].tolist()}: " \
                                  f"{g[name][tuple(bad[0])]} vs {w[name][tuple(bad[0])]}"


def assert_image(got, want, what):
    (gpx, gacc), (px, acc) = got, want
    bad = np.argwhere((gacc.view(np.uint32) != acc.view(np.uint32)).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} of {gacc.shape[0] * gacc.shape[1]} pixels differ, first (y, x) " \
                          f"{bad[:4].tolist()}: {gacc[tuple(bad[0])]} vs {acc[tuple(bad[0])]}"
    assert gacc.tobytes() == acc.tobytes() and np.array_equal(gpx, px), what


# ---- 1. the table ------------------------------------------------------------------------------------------
def decades_env(size, seed=0):
    """env_ref.random_env's recipe (five decades per channel, 5 % of the texels exactly 0), drawn in float32 so
    that S = 4096 stays cheap."""
    rng = np.random.default_rng(7000 + size + seed)
    e = np.exp2(rng.uniform(-10.0, 6.6, size=(size, size, 3)).astype(F)).astype(F)
    e[rng.uniform(size=(size, size)) < 0.05] = 0.0
    return np.ascontiguousarray(e)


@pytest.fixture()
def ready(pt):
    pt.setDevices([0])
    pt.uploadMesh(scenes.get_scene("cornell34"))
    assert pt.initialize(W, H), pt.lastError()
    return pt


# (the sizes at which the row kernel's run length per thread and its blocks' last thread change: 255, 256, 257 are one
# texel per thread with and without an idle tail and the first two-texel runs; 1000 four per thread; 4096 sixteen)
@pytest.mark.parametrize("size", [1, 2, 5, 64, 255, 256, 257, 1000, 4096])
def test_the_device_table_equals_the_restatement(ready, size):
    E = decades_env(size)
    ready.setEnvironment(E)
    assert_table(ready.envTable(), es.table(E), f"S = {size}")


def test_tables_of_black_one_bright_and_uninspected_maps(ready):
    black = np.zeros((33, 33, 3), F)
    ready.setEnvironment(black)
    tab = ready.envTable()
    assert_table(tab, es.table(black), "black")
    assert (tab["texels"]["q"] == 1).all() and (tab["rows"]["m"] == 1).all()
    one = np.full((300, 300, 3), 0.01, F)
    one[170, 41] = 1000.0
    ready.setEnvironment(one)
    assert_table(ready.envTable(), es.table(one), "one bright texel")
    # NaN, infinite and negative texels: only device memory brings them in (host memory is validated)
    bad = decades_env(70, 1)
    bad[0, :3], bad[5], bad[69, 69] = [[np.nan] * 3, [-1.0] * 3, [np.inf] * 3], np.nan, [3.0e38, 3.0e38, 3.0e38]
    dev = torch.from_numpy(bad).to(torch.device("cuda", 0))
    ready.setEnvironment(dev)
    tab = ready.envTable()
    assert_table(tab, es.table(bad), "NaN, inf and negative texels")
    assert (tab["texels"]["q"][5] == 1).all() and tab["rows"]["m"][5] == 1
    del dev
    ready.setEnvironment(None)
    assert ready.envTable() is None


# ---- 2. path queries ---------------------------------------------------------------------------------------
def check_paths(pt, case, mode, lds=1, width=0, prefixes=True):
    name, size, kind, select = case
    sc, E, rays, seeds, rad, segs = es.case(name, mode, size, kind, select)[:6]
    sampling(pt, mode, select)
    pt.setEnvironment(E)
    upload(pt, sc, lds, width)
    for n in ((1, 65, len(rays)) if prefixes else (len(rays),)):
        got, gs = pt.traceRadiance(np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n]), 8)
        pr.assert_paths(got, gs, rad[:n], segs[:n], f"{es.case_id(case)} mode {mode} lds={lds} width={width} n={n}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", es.PATH_CASES, ids=es.case_id)
def test_radiance_and_segments_match_the_reference(pt, case, mode):
    check_paths(pt, case, mode)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("lds,width", [(1, 2), (0, 4), (0, 2)])
@pytest.mark.parametrize("case", [es.PATH_CASES[1], es.PATH_CASES[7], es.PATH_CASES[9]], ids=es.case_id)
def test_other_layouts(pt, case, lds, width, mode):
    check_paths(pt, case, mode, lds, width, prefixes=False)


def test_the_option_changes_the_paths_with_a_lambertian_vertex_only(pt):
    sc, E, rays, seeds, rad, segs, ends, kinds = es.case("cornell_mixed", 2, 5)[:8]
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 2)
    pt.setEnvironment(E)
    upload(pt, sc)
    off, osegs = pt.traceRadiance(rays, seeds, 8)
    differ = (off.view(np.uint32) != rad.view(np.uint32)).any(axis=1)
    plain = (kinds & (1 << scenes.MAT_LAMBERTIAN)) == 0
    assert differ.any() and plain.any() and not differ[plain].any() and np.array_equal(osegs[plain], segs[plain])


@pytest.mark.parametrize("mode", [1, 2])
def test_device_tensors_give_the_same_bytes(pt, mode):
    assert torch.cuda.is_available()
    sc, E, rays, seeds, rad, segs = es.case("cornell34_lit", mode, 5)[:6]
    pt.setDevices([0])
    sampling(pt, mode)
    pt.setEnvironment(E)
    upload(pt, sc)
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(np.array(rays)).to(dev)
    ds = torch.from_numpy(np.array(seeds).view(np.int32)).to(dev)
    r, s = pt.traceRadiance(dr, ds, 8)
    assert r.device == dr.device and s.device == dr.device
    assert r.cpu().numpy().tobytes() == rad.tobytes() and s.cpu().numpy().tobytes() == segs.tobytes()
    del dr, ds, r, s


def test_depth_one_makes_no_connection(pt):
    sc, E, rays, seeds, rad, segs = es.case("cornell34", 2, 5, "random", False, 1)[:6]
    sampling(pt, 2)
    pt.setEnvironment(E)
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, 1)
    pr.assert_paths(got, gs, rad, segs, "maxDepth 1")
    assert (gs <= 1).all()


# ---- 3. the render route ------------------------------------------------------------------------------------
def check_route(mode, size):
    assert info(hippt.INFO_ENV_SAMPLING) == 1 and info(hippt.INFO_ENVIRONMENT) == size
    assert info(hippt.INFO_LIGHT_SAMPLING) == mode
    assert info(hippt.INFO_CHAIN_CAP) == 0 and info(hippt.INFO_RENDER_PAD) == 0 and info(hippt.INFO_SKY_RECT_PIXELS) == 0


@pytest.mark.parametrize("how", ["blocking", "async", "two_contexts"])
@pytest.mark.parametrize("name,mode", [("open_box", 2), ("open_box", 1), ("cornell34_lit", 2)])
def test_render_matches_the_render_reference(pt, name, mode, how):
    size, kind = (64, "block") if name == "open_box" else (5, "random")
    sc, E, acc, px, total, shadow = es.render_case(name, mode, size, kind)
    sampling(pt, mode)
    pt.setEnvironment(E)
    if how == "two_contexts":
        pt.setDevices([0, 0])
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    if how in ("async", "two_contexts"):
        for _ in range(FRAMES):
            assert pt.renderFramesAsync(1, 8), pt.lastError()
        assert pt.synchronize(), pt.lastError()
    else:
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert np.array_equal(pt.hostPixels(), px)
    assert_image(pt.readback(), (px, acc), f"{name} mode {mode} {how}")
    st = pt.stats()
    assert st["segments"] == total and st["pixelSamples"] == W * H * FRAMES
    assert 0 < shadow < total and pt.counters()["shadow_rays"] == shadow
    check_route(mode, size)


def test_two_row_ranges_give_the_whole_image(pt):
    sc, E, acc, px, _, _ = es.render_case("open_box", 2, 64, "block")
    sampling(pt, 2)
    pt.setEnvironment(E)
    pt.uploadMesh(sc)
    for y0, y1 in ((0, 11), (11, H)):
        pt.setRowRange(y0, y1)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert_image(pt.readback(y0, y1), (px[y0:y1], acc[y0:y1]), f"rows {y0}..{y1}")
        check_route(2, 64)


# ---- 4. ordering and state -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_under(envs, mode=2):
    """(scene, accumulation, pixel words, segments, shadow rays) of the open box's W x H render, frame f with the
    option on under the map envs[f] = (size, kind)."""
    sc, ref = es.scene_of("open_box")
    acc = np.zeros((H * W, 4), F)
    total = shadow = 0
    for f, e in enumerate(envs):
        r = es.ref_class(mode)(sc, ref, es.test_env(*e))
        a, px, t, s = sr.render(r, sc, W, H, 1, first=f, acc=acc)
        total, shadow = total + t, shadow + s
    return sc, a.copy(), px, total, shadow


def test_stream_order_each_frame_under_its_own_map_and_table(pt):
    """A, frame 0, B of A's size, frame 1, C of another size, frame 2, all asynchronous."""
    envs = ((64, "block"), (64, "random"), (5, "random"))
    sc, acc, px, total, shadow = frames_under(envs)
    sampling(pt, 2)
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    for e in envs:
        pt.setEnvironment(es.test_env(*e))
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    assert_image(pt.readback(), (px, acc), "A, frame, B, frame, C, frame")
    assert pt.stats()["segments"] == total and pt.counters()["shadow_rays"] == shadow
    assert_table(pt.envTable(), es.table(es.test_env(5)), "the last map's table")


@pytest.mark.parametrize("mode", [1, 2])
def test_on_off_on_without_a_new_environment(pt, mode):
    name = "cornell34_lit"
    sc, E, rays, seeds, rad, segs = es.case(name, mode, 5)[:6]
    off_ref = (mr.MisRef if mode == 2 else nr.NeeRef)(sc, es.scene_of(name)[1])
    want_off, wsegs_off = ev.paths_under(off_ref, E, rays, seeds)
    pt.setEnvironment(E)
    sampling(pt, mode)
    upload(pt, sc, w=W, h=H)
    for on in (1, 0, 1):
        pt.setOption(hippt.OPT_ENV_SAMPLING, on)
        got, gs = pt.traceRadiance(rays, seeds, 8)
        pr.assert_paths(got, gs, rad if on else want_off, segs if on else wsegs_off, f"mode {mode} option {on}")
        assert pt.renderFrames(1, 8), pt.lastError()
        assert info(hippt.INFO_ENV_SAMPLING) == on and info(hippt.INFO_LIGHT_SAMPLING) == mode


def test_where_the_option_does_not_apply_it_changes_no_byte(pt):
    sc, E, rays, seeds = es.case("cornell34", 2, 5)[:4]
    plain = pr.PathRef(sc, es.scene_of("cornell34")[1])
    want_env, wsegs_env = ev.paths_under(plain, E, rays, seeds)
    want_sky, wsegs_sky = pr.path_case("cornell34")[3:5]
    upload(pt, sc, w=W, h=H)
    pt.setOption(hippt.OPT_ENV_SAMPLING, 1)
    # mode 0 under a map: the plain paths under the map
    pt.setEnvironment(E)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, want_env, wsegs_env, "mode 0")
    assert pt.renderFrames(1, 8) and info(hippt.INFO_ENV_SAMPLING) == 0 and info(hippt.INFO_ENVIRONMENT) == 5
    # a mode without an environment, before one is set and after its removal: the gradient's paths
    pt.setEnvironment(None)
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 2)
    n = len(want_sky)
    sky_rays, sky_seeds = pr.path_case("cornell34")[1:3]
    got, gs = pt.traceRadiance(sky_rays, sky_seeds, 8)
    pr.assert_paths(got, gs, want_sky, wsegs_sky, f"no environment ({n} rays)")
    assert pt.renderFrames(1, 8) and info(hippt.INFO_ENV_SAMPLING) == 0 and info(hippt.INFO_LIGHT_SAMPLING) == 0


def test_the_table_outlives_uploads_and_initializations(pt):
    E = es.test_env(64, "block")
    pt.setEnvironment(E)  # before any Init: the host copy alone
    sampling(pt, 2)
    check = es.PATH_CASES[4]
    sc, _, rays, seeds, rad, segs = es.case(check[0], 2, check[1], check[2])[:6]
    upload(pt, scenes.get_scene("cornell34"))
    assert_table(pt.envTable(), es.table(E), "set before the Init")
    upload(pt, sc, w=W, h=H)  # another scene, a re-Init at another size
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, "after another upload and a re-Init")
    assert_table(pt.envTable(), es.table(E), "after another upload and a re-Init")


def test_the_builtin_scene_ignores_the_option(pt):
    import pyoracle as po
    pt.setEnvironment(es.test_env(5))
    sampling(pt, 2)
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    assert pt.initialize(64, 48), pt.lastError()
    assert pt.renderFrame(8), pt.lastError()
    spx, _ = po.sphere4(64, 48, 0, 1, 8)
    assert np.array_equal(pt.hostPixels(), spx) and info(hippt.INFO_ENV_SAMPLING) == 0


# ---- 5. the command-line tool ------------------------------------------------------------------------------
def test_cli_env_sampling(tmp_path):
    sc, ref = es.scene_of("cornell34")
    c = np.array([0.2, 0.3, 0.4], F).reshape(1, 1, 3)
    _, px, _, shadow = sr.render(es.EnvMisRef(sc, ref, c), sc, W, H, FRAMES)
    assert shadow > 0
    obj, out = tmp_path / "scene.obj", tmp_path / "frame.bin"
    scenes.write_obj(sc, str(obj), style="plain")
    albedo = ";".join(",".join(f"{v:.9g}" for v in a) for a in sc.albedo)
    base = [EXE, "--mesh", str(obj), "--albedo", albedo, "--width", str(W), "--height", str(H), "--spp", str(FRAMES),
            "--depth", "8", "--out", str(out)]
    r = subprocess.run(base + ["--background", "0.2,0.3,0.4", "--mis", "--env-sampling"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(str(out), "<u4").reshape(H, W), px)
    # it implies neither a map nor a mode
    for args in (["--env-sampling"], ["--background", "0.2,0.3,0.4", "--env-sampling"], ["--mis", "--env-sampling"]):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--env-sampling needs" in r.stderr, args


# ---- 6. same expectation, less noise, on the device -----------------------------------------------------------
def test_same_mean_and_less_variance_over_256_frames(pt):
    """The open box under hippt.scenes.sun_sky(64) with a small sun, 32x24, depth 8, 256 frames through cameraRays +
    traceRadiance on the device, MIS with the option 0 against 1.  Per channel the two overall means differ by at most
    5 standard errors of their difference (each standard error from the 256 per-frame image means themselves:
    test_gpu_mis.py's criterion), and the mean per-pixel sample variance is lower with 1.  Both are printed."""
    frames = 256
    sc = es.open_box()
    E = scenes.sun_sky(64, sun_dir=(0.1, 0.95, 0.2), sun_radiance=3000.0, sun_cos=0.9995)
    assert 1 <= np.count_nonzero(E[..., 0] > 100) <= 8
    dev = torch.device("cuda", 0)
    pt.setDevices([0])
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 2)
    pt.setEnvironment(E)
    upload(pt, sc, w=W, h=H)
    samples = {}
    for on in (0, 1):
        pt.setOption(hippt.OPT_ENV_SAMPLING, on)
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
        print(f"{channel}: mean 0 {m_off.mean():.6f} (se {se_off:.6f}), 1 {m_on.mean():.6f} (se {se_on:.6f}), "
              f"difference {diff:.6f} <= {bound:.6f}; mean per-pixel variance 0 {v_off:.5f}, 1 {v_on:.5f}")
        assert diff <= bound, (channel, diff, bound)
        assert v_on < v_off, (channel, v_on, v_off)
