"""The environment map on the CPU (no GPU): the library's host side against tests/env_ref.py, and conditions on
the reference alone that the GPU tests of tests/test_gpu_environment.py rely on.

hipptEnvLookup runs the text the path kernel compiles (qt-raytracer_amd/csrc/hippt_env.h), so its words against
env_ref.lookup's, bit for bit, pin the kernel's arithmetic before any GPU test does."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import env_ref as ev
import hippt
import path_ref as pr
from hippt import scenes

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")
SIZES = (1, 2, 5, 64)


@pytest.fixture()
def lib():
    L = hippt.load_library()
    L.cudaPathTracerShutdown()
    yield L
    assert L.hipptSetEnvironment(None, 0, 0, None)


def set_env(L, E, flags=0):
    E = np.ascontiguousarray(E, F)
    e = ctypes.c_char_p()
    ok = L.hipptSetEnvironment(E.ctypes.data, int(E.shape[0]), flags, ctypes.byref(e))
    return ok, (e.value or b"").decode()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _directions():
    """The directions of the sets below: 4,097 seeded ones of every length of the near-scene query domain's
    middle, the six axes, zero and -0 components, and both at lengths 2^-100 and 2^80."""
    rng = np.random.default_rng(19)
    d = rng.normal(size=(4097, 3)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(4097, 1))
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    zeros = np.array([[0.0, 0.3, -0.7], [-0.0, 0.3, -0.7], [0.4, 0.0, 0.6], [0.4, -0.0, 0.6], [0.4, -0.5, 0.0],
                      [0.4, -0.5, -0.0], [-0.0, -1.0, -0.0], [0.0, -1.0, 0.0], [-0.0, 1.0, 0.0], [-0.5, -0.0, -0.5],
                      [0.5, -0.0, 0.5], [-0.0, -0.0, 1.0], [1.0, -0.0, -0.0]], np.float64)
    return np.ascontiguousarray(np.concatenate([d, axes, zeros]), F)


DIRS = _directions()


# ---- 1. arguments --------------------------------------------------------------------------------------
def test_argument_errors_and_a_rejected_call_keeps_the_old_environment(lib):
    old = ev.random_env(5, 1)
    assert set_env(lib, old)[0]
    want = hippt.env_lookup(DIRS)
    good = np.ones((2, 2, 3), F)
    e = ctypes.c_char_p()
    for bad, word in ((np.array([[[1, 1, -1e-30]]], F), "negative"), (np.array([[[np.nan, 1, 1]]], F), "not finite"),
                      (np.array([[[1, np.inf, 1]]], F), "not finite"), (np.array([[[1, -np.inf, 1]]], F), "negative")):
        ok, msg = set_env(lib, bad)
        assert not ok and word in msg, msg
        assert hippt.env_lookup(DIRS).tobytes() == want.tobytes()
    for size in (0, -1, 4097, 1 << 20):
        assert not lib.hipptSetEnvironment(good.ctypes.data, size, 0, ctypes.byref(e)) and b"size must be in 1..4096" in e.value
    assert not lib.hipptSetEnvironment(None, 2, 0, ctypes.byref(e)) and b"null texels" in e.value
    for flags in (2, 4, -1, 3):
        assert not lib.hipptSetEnvironment(good.ctypes.data, 2, flags, ctypes.byref(e)) and b"unknown flags" in e.value
    assert not lib.hipptSetEnvironment(None, 0, 2, ctypes.byref(e)) and b"unknown flags" in e.value
    # device memory before an Init: refused without a device call
    assert not lib.hipptSetEnvironment(good.ctypes.data, 2, hippt.ENV_DEVICE, ctypes.byref(e))
    assert b"needs an initialized path tracer" in e.value
    assert not lib.hipptSetEnvironment(good.ctypes.data, 0, 0, None)  # (a null message pointer is allowed)
    assert set_env(lib, old)[0]
    assert hippt.env_lookup(DIRS).tobytes() == want.tobytes()
    # -0 is not negative, and 0 and values above 1 are texels like any other
    assert set_env(lib, np.array([[[-0.0, 0.0, 1e30]]], F))[0]
    # the lookup's own arguments
    out = np.zeros(3, F)
    assert not lib.hipptEnvLookup(None, 1, out.ctypes.data, ctypes.byref(e)) and b"null pointer" in e.value
    assert not lib.hipptEnvLookup(DIRS.ctypes.data, 1, None, ctypes.byref(e)) and b"null pointer" in e.value
    assert not lib.hipptEnvLookup(DIRS.ctypes.data, -1, out.ctypes.data, ctypes.byref(e)) and b"negative count" in e.value
    assert lib.hipptEnvLookup(None, 0, None, ctypes.byref(e))
    # the Python layer's
    pt = hippt.PathTracer()
    for bad in (np.ones((2, 3, 3), F), np.ones((2, 2, 4), F), np.ones((2, 2), F), np.ones((2, 2, 3), np.float64),
                np.ones((2, 4, 3), F)[:, ::2], [[[1.0, 1.0, 1.0]]]):
        with pytest.raises(hippt.HipptError):
            pt.setEnvironment(bad)
    with pytest.raises(hippt.HipptError, match="negative"):
        pt.setEnvironment(-good)
    for bad in (0, 4097):
        with pytest.raises(hippt.HipptError):
            hippt.env_directions(bad)
        with pytest.raises(hippt.HipptError):
            hippt.env_from_equirect(np.ones((2, 4, 3), F), bad)


def test_remove_brings_the_gradient_back(lib):
    e = ctypes.c_char_p()
    assert set_env(lib, ev.random_env(5, 0))[0]
    assert lib.hipptSceneDownload(hippt.SCENE_ENVIRONMENT, None, 0, ctypes.byref(e)) == 5 * 5 * 16
    assert lib.hipptSetEnvironment(None, 0, 0, ctypes.byref(e))
    assert lib.hipptSceneDownload(hippt.SCENE_ENVIRONMENT, None, 0, ctypes.byref(e)) == 0
    assert not lib.hipptEnvLookup(DIRS.ctypes.data, 1, np.zeros(3, F).ctypes.data, ctypes.byref(e))
    assert b"no environment set" in e.value
    assert lib.hipptGetOption(hippt.INFO_ENVIRONMENT) == 0
    assert lib.hipptSetEnvironment(None, 0, 0, ctypes.byref(e))  # removing nothing is no error
    # the reference's side of it: the swap ends, and path_ref.sky is the gradient's again
    gradient = pr.sky
    d, thr = (F(0.3), F(0.5), F(-0.2)), (0.5, 0.25, 1.0)
    before = gradient(d, thr)
    with ev.swap(np.full((1, 1, 3), 2.0, F)):
        assert pr.sky is not gradient and pr.sky(d, thr) == (F(1.0), F(0.5), F(2.0))
    assert pr.sky is gradient and pr.sky(d, thr) == before


# ---- 2. the lookup, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_lookup_matches_the_reference_bit_for_bit(lib, size):
    E = ev.random_env(size, 0)
    assert np.log10(E[E > 0].max() / E[E > 0].min()) > (3 if size > 1 else 0)  # several decades
    assert set_env(lib, E)[0]
    want = ev.lookups(E, DIRS)
    got = hippt.env_lookup(DIRS)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert bad.size == 0, f"S={size}: {bad.size} differ, first {DIRS[bad[:3]]}: {got[bad[:3]]} vs {want[bad[:3]]}"
    # the rule has no square: every length of the near-scene query domain gives the unit direction's words
    for scale in (F(2.0) ** F(-100), F(2.0) ** F(80)):
        scaled = DIRS * scale
        assert np.isfinite(scaled).all() and (np.abs(scaled[np.abs(DIRS) > 1e-3]) > 0).all()
        assert hippt.env_lookup(scaled).tobytes() == got.tobytes(), f"S={size} scale {scale}"
        assert ev.lookups(E, scaled[:257]).tobytes() == want[:257].tobytes()
    # a zero direction (no path holds one): NaN coordinates clamp to texel (0, 0), by minNum/maxNum
    assert hippt.env_lookup(np.zeros((1, 3), F)).tobytes() == E[0, 0].tobytes() == ev.lookups(E, np.zeros((1, 3))).tobytes()


def test_a_size_of_one_is_a_constant_colour_and_equal_neighbours_are_exact(lib):
    c = np.array([0.2, 0.3, 0.4], F)
    assert set_env(lib, c.reshape(1, 1, 3))[0]
    got = hippt.env_lookup(DIRS)
    assert (bits(got) == bits(c)).all()
    for size in (2, 5, 64):  # every texel equal: that value exactly, whatever the weights
        for value in (c, np.array([1e-3, 7.0, 123.456], F)):
            assert set_env(lib, np.broadcast_to(value, (size, size, 3)))[0]
            assert (bits(hippt.env_lookup(DIRS)) == bits(value)).all()


def test_texel_centres_map_back_to_their_own_texel(lib):
    for size in (1, 2, 5, 64, 257):
        D = hippt.env_directions(size)
        assert D.dtype == F and D.shape == (size, size, 3)
        want = ev.texel_directions(size)
        assert np.abs(D - want).max() < 1e-7 and np.abs(np.linalg.norm(D.astype(np.float64), axis=2) - 1).max() < 1e-6
        assert np.abs(scenes.env_texel_directions(size) - want).max() < 1e-15
        h = F(0.5) * F(size)
        for (y, x) in {(0, 0), (size - 1, 0), (size // 2, size // 3), (size - 1, size - 1), (size // 3, size - 1)}:
            u, w = ev.coords(D[y, x])
            assert abs(float(u) - ((2 * x + 1) / size - 1)) < 2e-5 and abs(float(w) - ((2 * y + 1) / size - 1)) < 2e-5
            # (so the filter's weights there are within 2e-5 * S / 2 of (1, 0): the texel's own value, nearly)
            assert abs((float(u) * float(h) + float(h) - 0.5) - x) < 2e-5 * size
    # a map with one bright texel returns it at that texel's direction
    size = 5
    E = np.zeros((size, size, 3), F)
    E[3, 1] = (4.0, 5.0, 6.0)
    assert set_env(lib, E)[0]
    got = hippt.env_lookup(hippt.env_directions(size))
    assert np.allclose(got[3, 1], (4.0, 5.0, 6.0), rtol=1e-4) and np.abs(got[0, 4]).max() < 1e-3


# ---- 3. orientation ------------------------------------------------------------------------------------
QUAD = {(1, 1): (1.0, 0.0, 0.25), (1, -1): (0.0, 2.0, 0.5), (-1, 1): (4.0, 0.5, 0.0), (-1, -1): (0.125, 8.0, 3.0)}
UPPER, LOWER = (0.5, 0.75, 16.0), (0.25, 0.125, 0.0625)


def sign_map(size):
    d = ev.texel_directions(size)
    E = np.zeros((size, size, 3), F)
    for (sx, sz), c in QUAD.items():
        E[((d[..., 0] >= 0) == (sx > 0)) & ((d[..., 2] >= 0) == (sz > 0))] = c
    return E


def hemisphere_map(size):
    d = ev.texel_directions(size)
    return np.where(d[..., 1:2] >= 0, np.asarray(UPPER, F), np.asarray(LOWER, F)).astype(F)


@pytest.mark.parametrize("size", [16, 64])
def test_orientation_by_sign_and_by_hemisphere(lib, size):
    d64 = DIRS[:4097].astype(np.float64)
    s = np.abs(d64).sum(axis=1, keepdims=True)
    texel = 2.0 / size
    # by the signs of dx and dz: the image's quadrants, in both hemispheres; away from the axes by two texels
    assert set_env(lib, sign_map(size))[0]
    got = hippt.env_lookup(DIRS[:4097])
    far = (np.abs(d64[:, 0:1] / s) > 2 * texel).ravel() & (np.abs(d64[:, 2:3] / s) > 2 * texel).ravel()
    assert far.sum() > (1000 if size == 64 else 400)
    for i in np.flatnonzero(far):
        want = QUAD[(1 if d64[i, 0] >= 0 else -1, 1 if d64[i, 2] >= 0 else -1)]
        assert tuple(got[i]) == tuple(F(v) for v in want), (i, d64[i])
    # by hemisphere: the inner diamond is +y; away from the diamond's edge by two texels on each axis
    assert set_env(lib, hemisphere_map(size))[0]
    got = hippt.env_lookup(DIRS[:4097])
    far = (np.abs(d64[:, 1:2] / s) > 4 * texel).ravel()
    assert far.sum() > (1000 if size == 64 else 400)
    up = d64[:, 1] >= 0
    assert (got[far & up] == np.asarray(UPPER, F)).all() and (got[far & ~up] == np.asarray(LOWER, F)).all()
    assert (far & up).sum() > 100 and (far & ~up).sum() > 100
    # within half a texel of the lower hemisphere's fold lines (the square's border) the filter is not continuous
    # (clamp to edge, documented): under a map that is smooth on the sphere, 1 + dx, two directions 2e-4 apart
    # across the plane x = 0 below the horizon read the border texels of either side, 2 dx of a border texel apart
    smooth = np.repeat((1.0 + ev.texel_directions(size)[..., 0:1]).astype(F), 3, axis=2)
    assert set_env(lib, smooth)[0]
    a, b = hippt.env_lookup(np.array([[1e-4, -1.0, 0.5], [-1e-4, -1.0, 0.5]], F))
    assert a[0] - b[0] > (0.05 if size == 16 else 0.0125)
    a, b = hippt.env_lookup(np.array([[1e-4, 1.0, 0.5], [-1e-4, 1.0, 0.5]], F))  # (above it: continuous)
    assert abs(a[0] - b[0]) < 1e-3


def test_equirect_of_the_same_patterns_gives_those_maps():
    W, H, size = 64, 32, 16
    theta = np.pi * (np.arange(H) + 0.5) / H
    phi = 2 * np.pi * (np.arange(W) + 0.5) / W - np.pi
    dx = np.sin(theta)[:, None] * np.cos(phi)[None, :]
    dy = np.cos(theta)[:, None] * np.ones(W)[None, :]
    dz = np.sin(theta)[:, None] * np.sin(phi)[None, :]
    by_sign = np.zeros((H, W, 3), F)
    for (sx, sz), c in QUAD.items():
        by_sign[((dx >= 0) == (sx > 0)) & ((dz >= 0) == (sz > 0))] = c
    by_hemi = np.where(dy[..., None] >= 0, np.asarray(UPPER, F), np.asarray(LOWER, F)).astype(F)
    d = ev.texel_directions(size)
    # away from the patterns' edges by more than two lat-long pixels (2 * 2 pi / 64 < 0.2 rad < asin(0.25))
    far_sign = (np.abs(d[..., 0]) > 0.25) & (np.abs(d[..., 2]) > 0.25)
    far_hemi = np.abs(d[..., 1]) > 0.25
    assert far_sign.sum() > size * size // 4 and far_hemi.sum() > size * size // 2
    got = hippt.env_from_equirect(by_sign, size)
    assert got.dtype == F and got.shape == (size, size, 3)
    assert (got[far_sign] == sign_map(size)[far_sign]).all()
    got = hippt.env_from_equirect(by_hemi, size)
    assert (got[far_hemi] == hemisphere_map(size)[far_hemi]).all()
    # between the patterns' colours elsewhere (bilinear), and a constant image is that constant everywhere
    assert (got >= np.minimum(UPPER, LOWER).astype(F)).all() and (got <= np.maximum(UPPER, LOWER).astype(F)).all()
    flat = hippt.env_from_equirect(np.full((3, 7, 3), 0.3, F), 5)
    assert (flat == F(0.3)).all()
    # row 0 is +y: a image that is bright in its top row only lights the texels around +y
    top = np.zeros((8, 16, 3), F)
    top[0] = 1.0
    got = hippt.env_from_equirect(top, 9)
    assert got[4, 4, 0] > 0.5 and got[0, 0, 0] == 0 and got[4, 0, 0] == 0  # centre: +y; corner: -y; edge: horizon


# ---- 4. closed forms on the reference alone --------------------------------------------------------------
def one_triangle(up=True, albedo=(0.5, 0.25, 0.75)):
    v = np.array([[-50.0, 0.0, -50.0, 0.0, 0.0, 60.0, 50.0, 0.0, -50.0]], F)  # counter-clockwise from above: +y
    if not up:
        v = np.ascontiguousarray(v.reshape(3, 3)[::-1].reshape(1, 9))
    return scenes.Scene("one_triangle", v, np.zeros(1, np.int32), np.asarray([albedo], F), lookfrom=(0.0, 30.0, -60.0),
                        lookat=(0.0, 0.0, 0.0), vfov=60.0)


def rays_towards_plane(n, side, seed=5):
    """Rays from y = side * 20 towards points of the plane y = 0 within and around the triangle."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-30, 30, n), np.full(n, side * 20.0), rng.uniform(-30, 30, n)], axis=1)
    aim = np.stack([rng.uniform(-70, 70, n), np.zeros(n), rng.uniform(-70, 70, n)], axis=1)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0.001, aim - o, np.inf
    return rays


def test_closed_form_under_a_constant_environment():
    from test_gpu_ray_query import Ref
    rho, c = np.array([0.5, 0.25, 0.75], F), np.array([0.2, 3.0, 0.7], F)
    sc = one_triangle(True, rho)
    ref = pr.PathRef(sc, Ref(sc))
    rays, seeds = rays_towards_plane(512, 1), hippt.path_seeds(512)
    for E in (c.reshape(1, 1, 3), np.broadcast_to(c, (5, 5, 3))):
        rad, segs = ev.paths_under(ref, E, rays, seeds)
        hit = rad[:, 3] == 1.0
        assert 100 < hit.sum() < 412
        # a hit: one Lambertian scatter, throughput rho, then the environment: rho * c, one multiply per channel
        assert (segs[hit] == 2).all() and (bits(rad[hit, :3]) == bits(rho * c)).all()
        assert (segs[~hit] == 1).all() and (bits(rad[~hit, :3]) == bits(c)).all()
    # the replayed record is the direct run
    rec = ev.record(ref, rays, seeds)
    assert ev.replay(rec, c.reshape(1, 1, 3))[0].tobytes() == rad.tobytes()


def test_the_floor_sees_the_upper_colour_and_a_ceiling_the_lower():
    from test_gpu_ray_query import Ref
    rho = np.array([0.5, 0.25, 0.75], F)
    E = hemisphere_map(64)
    for up, colour, other in ((True, UPPER, LOWER), (False, LOWER, UPPER)):
        sc = one_triangle(up, rho)
        ref = pr.PathRef(sc, Ref(sc))
        rays, seeds = rays_towards_plane(512, 1 if up else -1), hippt.path_seeds(512)
        log = []
        with ev.swap(E, log):
            rad, segs, _, _ = ref.paths(rays, seeds)
        hit = rad[:, 3] == 1.0
        assert 100 < hit.sum() < 412 and (segs[hit] == 2).all() and len(log) == 512
        # the scattered direction leaves on the triangle's own side; away from the horizon's texels the map is
        # the side's colour exactly, and nowhere does a path see more of the other side's than of its own
        clear = np.array([abs(float(l["d"][1])) / sum(abs(float(x)) for x in l["d"]) > 4 * 2.0 / 64 for l in log])
        assert (hit & clear).sum() > 0.8 * hit.sum()
        assert (bits(rad[hit & clear, :3]) == bits(rho * np.asarray(colour, F))).all()
        mid = 0.5 * (np.asarray(colour, np.float64) + np.asarray(other, np.float64)) * rho
        nearer = np.abs(rad[hit, :3] - rho * np.asarray(colour, F)) <= np.abs(rad[hit, :3] - mid) + 1e-6
        assert nearer.all()


# ---- 5. conditions on the ray sets the GPU tests use -------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed", "blob64x34", "random_scene"])
def test_the_gpu_tests_ray_sets_look_the_map_up_in_every_way(name):
    sc, rays, seeds, rec = ev.path_case(name)
    missed, segs = rec["missed"], rec["segs"]
    primary, later = missed & (segs == 1), missed & (segs > 1)
    assert primary.sum() >= 30 and later.sum() >= 100, (primary.sum(), later.sum())
    d = rec["d"][missed]
    low = clamp5 = clamp64 = 0
    texels2 = set()
    for k in range(len(d)):
        det5, det64, det2 = {}, {}, {}
        ev.lookup(ev.env_of(5), d[k], det5)
        ev.lookup(ev.env_of(64), d[k], det64)
        ev.lookup(ev.env_of(2), d[k], det2)
        low += det5["low"]
        clamp5 += det5["clamped"]
        clamp64 += det64["clamped"]
        texels2 |= det2["texels"]
    n = len(d)
    print(f"{name}: primary misses {primary.sum()}, after a scatter {later.sum()}, dy < 0 {100 * low / n:.0f} %, "
          f"clamped S=5 {100 * clamp5 / n:.0f} %, clamped S=64 {clamp64} of {n}, texels S=2 {len(texels2)}")
    assert low >= 0.15 * n and clamp5 >= 0.10 * n and clamp64 >= 1 and texels2 == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_replay_is_the_reference_under_the_swap():
    """env_ref.replay (a ray set traced once, its sky calls made again per map) against a direct run of PathRef
    and emit_ref.render_with under env_ref.swap, and against the gradient's own references."""
    import emit_ref as er
    sc, rays, seeds, rec = ev.path_case("cornell34")
    ref = ev._path_ref_of("cornell34")[1]
    n = 1025
    E = ev.env_of(5)
    rad, segs = ev.paths_under(ref, E, rays[:n], seeds[:n])
    got, gs = ev.replay(rec, E)
    assert got[:n].tobytes() == rad.tobytes() and gs[:n].tobytes() == segs.tobytes()
    assert (got[rec["missed"]][:, :3] != pr.path_case("cornell34")[3][rec["missed"]][:, :3]).any(axis=1).mean() > 0.9
    g0, s0 = ev.replay(rec, None)
    assert g0.tobytes() == pr.path_case("cornell34")[3].tobytes() and s0.tobytes() == pr.path_case("cornell34")[4].tobytes()
    w, h = 8, 6
    scc, recs = ev.camera_case("cornell34", w, h, 2)
    acc, px, total = ev.render_replay(recs, [E, E], w, h)
    wacc, wpx, wtotal = ev.render_under(ref, E, scc, w, h, 2)
    assert acc.tobytes() == wacc.tobytes() and np.array_equal(px, wpx) and total == wtotal
    acc, px, total = ev.render_replay(recs, [None, None], w, h)
    wacc, wpx, wtotal, _, _ = er.render_with(ref, scc, w, h, 2)
    assert acc.tobytes() == wacc.tobytes() and np.array_equal(px, wpx) and total == wtotal


def test_sun_sky_is_a_valid_environment(lib):
    E = scenes.sun_sky(64)
    assert E.dtype == F and E.shape == (64, 64, 3) and np.isfinite(E).all() and (E >= 0).all()
    assert E.max() > 50 and 0 < np.count_nonzero(E[..., 0] > 50) < 64  # the disc: a few texels
    assert set_env(lib, E)[0]
    assert hippt.env_lookup(np.array([[0.35, 0.8, 0.45]], F))[0].max() > 30 > hippt.env_lookup(np.array([[0, 1, 0]], F))[0].max()


# ---- 6. the file reader and the resampler, stand-alone ---------------------------------------------------
def test_env_io_stand_alone_program(tmp_path):
    exe = tmp_path / "env_io_check"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(REPO, "tests", "native", "env_io_check.cpp"), os.path.join(CSRC, "env_io.cpp")], check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and "env_io_check ok" in r.stdout, r.stdout + r.stderr
