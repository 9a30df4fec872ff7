"""The environment map (GPU): hipptSetEnvironment in hipptTraceRadiance and the render calls against the references
under tests/env_ref.py's rule, bit for bit.

The references are path_ref.PathRef (traced once per ray set and replayed per map, env_ref.record / replay) and
the light-sampling references (nee_ref, mis_ref, select_ref) run under env_ref.swap; tests/test_env_ref_cpu.py pins
the rule's host text and the replay, and asserts on the reference alone that these ray sets look the map up in
every way.  Every comparison is exact: the radiance words and segment counts of every ray, the accumulation's
bytes, the pixel words and the segment totals."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import env_ref as ev
import hippt
import path_ref as pr
import pyoracle as po
from hippt import scenes
from test_gpu_ray_query import N, degenerate_rays, upload

pytestmark = pytest.mark.gpu

F = np.float32
W, H, FRAMES = 32, 24, 3
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_SKY_RECT, 1),
        (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB), (hippt.OPT_LIGHT_SAMPLING_MODE, 0), (hippt.OPT_LIGHT_SELECT, 0))
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


@functools.lru_cache(maxsize=None)
def want_paths(name, size, seed=0, depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments) of a ray set under env_of(size, seed); computed once."""
    sc, rays, seeds, rec = ev.path_case(name, depth)
    rad, segs = ev.replay(rec, ev.env_of(size, seed))
    rad.setflags(write=False)
    return sc, rays, seeds, rad, segs


@functools.lru_cache(maxsize=None)
def want_image(envs, name="cornell34"):
    """(scene, accumulation, pixel words, segments) of the W x H render of FRAMES frames, frame f under the map
    env_of(*envs[f]) (None: the gradient)."""
    sc, recs = ev.camera_case(name, W, H, FRAMES)
    acc, px, total = ev.render_replay(recs, [None if e is None else ev.env_of(*e) for e in envs], W, H)
    acc.setflags(write=False)
    px.setflags(write=False)
    return sc, acc, px, total


E5 = ((5, 0),) * FRAMES


def assert_image(got, want, what):
    (gpx, gacc), (px, acc) = got, want
    bad = np.argwhere((gacc.view(np.uint32) != acc.view(np.uint32)).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} of {gacc.shape[0] * gacc.shape[1]} pixels differ, first (y, x) " \
                          f"{bad[:4].tolist()}: {gacc[tuple(bad[0])]} vs {acc[tuple(bad[0])]}"
    assert gacc.tobytes() == acc.tobytes() and np.array_equal(gpx, px), what


# ---- 1. path queries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed", "blob64x34", "random_scene"])
def test_radiance_and_segments_match_the_reference(pt, name, lds, width):
    sc, rays, seeds, rad, segs = want_paths(name, 5)
    pt.setEnvironment(ev.env_of(5))
    upload(pt, sc, lds, width)
    for n in (1, 65, len(rays)):
        got, gs = pt.traceRadiance(np.ascontiguousarray(rays[:n]), np.ascontiguousarray(seeds[:n]), 8)
        pr.assert_paths(got, gs, rad[:n], segs[:n], f"{name} lds={lds} width={width} n={n}")
    assert got.tobytes() == rad.tobytes() and gs.tobytes() == segs.tobytes()
    # (the gradient's radiance is another: the map is what the misses returned)
    missed = ev.path_case(name)[3]["missed"]
    assert (rad[missed][:, :3] != pr.path_case(name)[3][missed][:, :3]).any(axis=1).mean() > 0.9


@pytest.mark.parametrize("size", [1, 2, 64])
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_other_sizes(pt, name, size):
    sc, rays, seeds, rad, segs = want_paths(name, size)
    pt.setEnvironment(ev.env_of(size))
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"{name} S={size}")


def test_device_tensors_give_the_same_bytes(pt):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs = want_paths("cornell_mixed", 5)
    pt.setDevices([0])
    pt.setEnvironment(ev.env_of(5))
    upload(pt, sc)
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(np.array(rays)).to(dev)
    ds = torch.from_numpy(np.array(seeds).view(np.int32)).to(dev)
    r, s = pt.traceRadiance(dr, ds, 8)
    assert r.device == dr.device and s.device == dr.device
    assert r.cpu().numpy().tobytes() == rad.tobytes() and s.cpu().numpy().tobytes() == segs.tobytes()
    del dr, ds, r, s


def test_depth_one_has_the_environment_behind_and_hits_black(pt):
    sc, rays, seeds, rad, segs = want_paths("cornell34", 5, 0, 1)
    hit = rad[:, 3] == 1.0
    assert 1000 < hit.sum() < N - 100 and not rad[hit, :3].any() and (rad[~hit][:, :3] > 0).any(axis=1).sum() > 400
    pt.setEnvironment(ev.env_of(5))
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, 1)
    pr.assert_paths(got, gs, rad, segs, "maxDepth 1")


@functools.lru_cache(maxsize=None)
def scaled_case(exponent):
    """cornell34's rays (every fourth, without the degenerate tail), first-segment directions scaled by
    2^exponent, tmin 0 (with a long direction every t is below 0.001): (rays, seeds, radiance, segments) under
    env_of(5), the oracle's own paths of the scaled rays."""
    sc, ref = ev._path_ref_of("cornell34")
    rays = np.array(ev.path_case("cornell34")[1][:N - degenerate_rays().shape[0]:4])
    rays[:, 4:7] *= F(2.0) ** F(exponent)
    rays[:, 3] = 0.0
    assert np.isfinite(rays[:, 4:7]).all() and (np.abs(rays[:, 4:7]).max(axis=1) > 0).all()
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    rec = ev.record(ref, rays, seeds)
    primary = rec["missed"] & (rec["segs"] == 1)
    assert primary.sum() >= 30 and (rec["missed"] & (rec["segs"] > 1)).sum() >= 100  # (the map is looked up both ways)
    rad, segs = ev.replay(rec, ev.env_of(5))
    return rays, seeds, rad, segs


@pytest.mark.parametrize("exponent", [-100, 80])
def test_first_segment_directions_of_extreme_length(pt, exponent):
    rays, seeds, rad, segs = scaled_case(exponent)
    pt.setEnvironment(ev.env_of(5))
    upload(pt, ev.path_case("cornell34")[0])
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, f"directions x 2^{exponent}")


# ---- 2. light sampling under an environment -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lit_case(name, mode, select):
    """(scene, rays, seeds, radiance, segments) of every fourth ray of the lit scene's set under light-sampling
    `mode` (uniform or power selection) and env_of(5): the reference of that mode under the swap."""
    import emit_ref as er
    import mis_ref as mr
    import nee_ref as nr
    import select_ref as sr
    from test_gpu_ray_query import Ref, make_rays
    sc = er.lit_scene(name)
    cls = {(1, 0): nr.NeeRef, (2, 0): mr.MisRef, (1, 1): sr.SelectNeeRef, (2, 1): sr.SelectMisRef}[(mode, select)]
    ref = cls(sc, Ref(sc))
    rays = np.ascontiguousarray(make_rays(sc, N)[::4])
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    log = []
    with ev.swap(ev.env_of(5), log):
        rad, segs = ref.paths(rays, seeds, 8)[:2]
    assert len(log) >= 100  # (paths that end on the map, after connections or not)
    return sc, rays, seeds, rad, segs


@pytest.mark.parametrize("mode,select", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_light_sampling_modes_under_an_environment(pt, name, mode, select):
    sc, rays, seeds, rad, segs = lit_case(name, mode, select)
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, mode)
    pt.setOption(hippt.OPT_LIGHT_SELECT, hippt.LIGHT_SELECT_POWER if select else 0)
    pt.setEnvironment(ev.env_of(5))
    for lds, width in ((1, 4), (0, 2)):
        upload(pt, sc, lds, width)
        got, gs = pt.traceRadiance(rays, seeds, 8)
        pr.assert_paths(got, gs, rad, segs, f"{name} mode {mode} select {select} lds={lds} width={width}")


# ---- 3. the render route ------------------------------------------------------------------------------------
def check_route(what, size=5):
    assert info(hippt.INFO_ENVIRONMENT) == size, what
    assert info(hippt.INFO_CHAIN_CAP) == 0 and info(hippt.INFO_RENDER_PAD) == 0 and info(hippt.INFO_SKY_RECT_PIXELS) == 0


@pytest.mark.parametrize("how", ["blocking", "async", "path_mode_1", "two_contexts", "lds0_width2"])
def test_render_matches_the_render_reference(pt, how):
    sc, acc, px, total = want_image(E5)
    pt.setEnvironment(ev.env_of(5))
    if how == "path_mode_1":
        pt.setOption(hippt.OPT_PATH_MODE, 1)
    if how == "two_contexts":
        pt.setDevices([0, 0])
    if how == "lds0_width2":
        pt.setOption(hippt.OPT_LDS_SCENE, 0)
        pt.setOption(hippt.OPT_BVH_WIDTH, 2)
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
    assert_image(pt.readback(), (px, acc), how)
    st = pt.stats()
    assert st["segments"] == total and st["pixelSamples"] == W * H * FRAMES, how
    check_route(how)
    assert info(hippt.INFO_LIGHT_SAMPLING) == 0
    # (another image than the gradient's)
    assert not np.array_equal(px, want_image((None,) * FRAMES)[2])


def test_two_row_ranges_give_the_whole_image(pt):
    sc, acc, px, _ = want_image(E5)
    pt.setEnvironment(ev.env_of(5))
    pt.uploadMesh(sc)
    for y0, y1 in ((0, 11), (11, H)):
        pt.setRowRange(y0, y1)
        assert pt.initialize(W, H), pt.lastError()
        assert pt.renderFrames(FRAMES, 8), pt.lastError()
        assert_image(pt.readback(y0, y1), (px[y0:y1], acc[y0:y1]), f"rows {y0}..{y1}")
        check_route(f"rows {y0}..{y1}")


def test_rgba8_words(pt):
    sc, acc, px, _ = want_image(E5)
    pt.setEnvironment(ev.env_of(5))
    pt.setOption(hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_RGBA8)
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    gpx, gacc = pt.readback()
    assert gacc.tobytes() == acc.tobytes()
    assert np.array_equal(gpx, po.rgba8(np.array(acc)))
    check_route("rgba8")


@functools.lru_cache(maxsize=None)
def mis_image():
    import emit_ref as er
    import mis_ref as mr
    import select_ref as sr
    from test_gpu_ray_query import Ref
    sc = er.lit_scene("cornell34_lit")
    with ev.swap(ev.env_of(5)):
        acc, px, total, shadow = sr.render(mr.MisRef(sc, Ref(sc)), sc, W, H, FRAMES)
    return sc, acc, px, total, shadow


def test_render_with_mis_under_an_environment(pt):
    sc, acc, px, total, shadow = mis_image()
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, hippt.LIGHT_SAMPLING_MIS)
    pt.setEnvironment(ev.env_of(5))
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert_image(pt.readback(), (px, acc), "mode 2")
    assert pt.stats()["segments"] == total and 0 < shadow < total and pt.counters()["shadow_rays"] == shadow
    check_route("mode 2")
    assert info(hippt.INFO_LIGHT_SAMPLING) == 2


def test_camera_rays_traced_are_one_render_sample(pt):
    sc, recs = ev.camera_case("cornell34", W, H, FRAMES)
    want, _ = ev.replay(recs[0], ev.env_of(5))
    pt.setEnvironment(ev.env_of(5))
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    assert pt.renderFrames(1, 8), pt.lastError()
    _, acc = pt.readback()  # frame 0 alone: by po_accumulate its average is the sample itself
    rays, seeds = pt.cameraRays(0)
    rad, segs = pt.traceRadiance(rays, seeds, 8)
    assert np.ascontiguousarray(rad[:, :3]).tobytes() == np.ascontiguousarray(acc.reshape(-1, 4)[:, :3]).tobytes()
    assert rad.tobytes() == want.tobytes() and segs.tobytes() == recs[0]["segs"].tobytes()


# ---- 4. stream order, remove, lifetime -----------------------------------------------------------------------
def test_stream_order(pt):
    """A, frame 0, B of A's size, frame 1, C of another size, frame 2, all asynchronous: each frame under the map
    that was set when it was enqueued."""
    envs = ((5, 0), (5, 1), (2, 0))
    sc, acc, px, total = want_image(envs)
    pt.uploadMesh(sc)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    for e in envs:
        pt.setEnvironment(ev.env_of(*e))
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    assert_image(pt.readback(), (px, acc), "A, frame, B, frame, C, frame")
    assert pt.stats()["segments"] == total and info(hippt.INFO_ENVIRONMENT) == 2
    assert not np.array_equal(px, want_image(E5)[2])


def test_remove_gives_the_gradients_bytes(pt):
    sc, rays, seeds, grad, gsegs = pr.path_case("cornell34")[:5]
    upload(pt, sc, w=W, h=H)
    pt.setEnvironment(ev.env_of(5))
    _, _, _, rad5, segs5 = want_paths("cornell34", 5)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad5, segs5, "set")
    assert pt.renderFrames(1, 8), pt.lastError()
    assert info(hippt.INFO_ENVIRONMENT) == 5 and pt.environment().shape == (5, 5, 3)
    pt.setEnvironment(None)
    assert pt.environment() is None
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, grad, gsegs, "set, remove")
    opx, oacc, osegs, _ = po.MeshScene(sc, W, H).frames(0, FRAMES, 8)
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert_image(pt.readback(), (opx, oacc), "render after remove")
    assert pt.stats()["segments"] == osegs and info(hippt.INFO_ENVIRONMENT) == 0
    assert np.array_equal(opx, want_image((None,) * FRAMES)[2])  # (the replayed gradient is the oracle's too)
    pt.setEnvironment(ev.env_of(2))
    _, _, _, rad2, segs2 = want_paths("cornell34", 2)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad2, segs2, "set, remove, set")
    assert pt.initialize(W, H), pt.lastError()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    _, acc, px, _ = want_image(((2, 0),) * FRAMES)
    assert_image(pt.readback(), (px, acc), "render after set, remove, set")
    assert info(hippt.INFO_ENVIRONMENT) == 2


def test_the_environment_outlives_uploads_and_initializations(pt):
    pt.setEnvironment(ev.env_of(5))  # before any Init: the host copy alone
    sc, rays, seeds, rad, segs = want_paths("cornell_mixed", 5)
    upload(pt, sc)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, "set before the Init")
    sc2, acc, px, total = want_image(E5)
    pt.uploadMesh(sc2)  # another scene
    assert pt.initialize(W, H), pt.lastError()  # a re-Init at another size
    pt.resetStats()
    assert pt.renderFrames(FRAMES, 8), pt.lastError()
    assert_image(pt.readback(), (px, acc), "after another upload and a re-Init")
    assert pt.stats()["segments"] == total and info(hippt.INFO_ENVIRONMENT) == 5
    assert pt.environment().tobytes() == ev.env_of(5).tobytes()


def test_the_builtin_scene_ignores_the_environment(pt):
    pt.setEnvironment(ev.env_of(5))
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    assert pt.initialize(64, 48), pt.lastError()
    assert pt.renderFrame(8), pt.lastError()
    spx, _ = po.sphere4(64, 48, 0, 1, 8)
    assert np.array_equal(pt.hostPixels(), spx) and info(hippt.INFO_ENVIRONMENT) == 0


# ---- 5. device memory ----------------------------------------------------------------------------------
def test_a_device_tensor_environment_gives_the_host_ones_bytes(pt):
    assert torch.cuda.is_available()
    sc, rays, seeds, rad, segs = want_paths("cornell34", 5)
    pt.setDevices([0])
    upload(pt, sc, w=W, h=H)
    dev = torch.device("cuda", 0)
    E = torch.from_numpy(np.array(ev.env_of(5))).to(dev)
    pt.setEnvironment(E)
    got, gs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(got, gs, rad, segs, "device-memory environment")
    assert hippt.env_lookup(rays[:64, 4:7]).tobytes() == ev.lookups(ev.env_of(5), rays[:64, 4:7]).tobytes()  # (fetched)
    # environment(): the texels after the queued work
    assert pt.renderFramesAsync(1, 8), pt.lastError()
    pt.setEnvironment(ev.env_of(5, 1))
    assert pt.environment().tobytes() == ev.env_of(5, 1).tobytes()
    pt.setEnvironment(ev.env_of(64))
    assert pt.environment().tobytes() == ev.env_of(64).tobytes()
    # a host pointer under the device flag
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    host = np.array(ev.env_of(5))
    assert not lib.hipptSetEnvironment(host.ctypes.data, 5, hippt.ENV_DEVICE, ctypes.byref(e))
    assert b"needs device memory pointers" in e.value
    assert pt.environment().tobytes() == ev.env_of(64).tobytes()  # (the rejected call changed nothing)
    del E


# ---- 6. the command-line tool ------------------------------------------------------------------------------
def run_cli(tmp_path, sc, *args):
    obj, out = tmp_path / "scene.obj", tmp_path / "frame.bin"
    scenes.write_obj(sc, str(obj), style="plain")
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    r = subprocess.run([EXE, "--mesh", str(obj), "--albedo", albedo, *args, "--width", str(W), "--height", str(H),
                        "--spp", str(FRAMES), "--depth", "8", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(str(out), "<u4").reshape(H, W)


def test_cli_background_and_env(tmp_path):
    sc, recs = ev.camera_case("cornell34", W, H, FRAMES)
    c = np.array([0.2, 0.3, 0.4], F)
    _, px, _ = ev.render_replay(recs, [c.reshape(1, 1, 3)] * FRAMES, W, H)
    assert np.array_equal(run_cli(tmp_path, sc, "--background", "0.2,0.3,0.4"), px)
    # a small lat-long PFM (rows bottom to top, little-endian) through hipptEnvFromEquirect
    img = (10.0 ** np.random.default_rng(7).uniform(-2, 1, size=(8, 16, 3))).astype(F)
    pfm = tmp_path / "sky.pfm"
    with open(pfm, "wb") as f:
        f.write(b"PF\n16 8\n-1.0\n")
        f.write(np.ascontiguousarray(img[::-1]).astype("<f4").tobytes())
    E = hippt.env_from_equirect(img, 8)
    _, px, _ = ev.render_replay(recs, [E] * FRAMES, W, H)
    assert np.array_equal(run_cli(tmp_path, sc, "--env", str(pfm), "--env-size", "8"), px)
    assert not np.array_equal(px, want_image((None,) * FRAMES)[2])
    # a malformed file: a message, no frame
    bad = tmp_path / "bad.pfm"
    bad.write_bytes(b"PF\n16 8\n-1.0\n" + b"\0" * 100)
    r = subprocess.run([EXE, "--mesh", str(tmp_path / "scene.obj"), "--env", str(bad), "--width", "8", "--height", "8"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "shorter than its header says" in r.stderr
