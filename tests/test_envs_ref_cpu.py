"""Environment sampling without a GPU: the option through the ABI, the constants, the properties of the selection
table of tests/envs_ref.py, the header's arithmetic (qt-raytracer_amd/csrc/hippt_env.h, the kernels' own text) against
the restatement through a stand-alone program, that the GPU tests' ray sets meet every case of the rule, and on the
references alone that the option leaves the expectation where it was and lowers the variance."""
import ctypes
import fractions
import os
import re
import subprocess

import numpy as np
import pytest

import env_ref as ev
import envs_ref as es
import hippt
import mis_ref as mr
import nee_ref as nr
import pyoracle as po

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "hippt.h")
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")
EPS = 2.0 ** -24


# ---- the public surface ------------------------------------------------------------------------------
def test_the_option_takes_0_and_1_only_and_reads_back():
    lib = hippt.load_library()
    assert lib.hipptGetOption(hippt.OPT_ENV_SAMPLING) == 0
    try:
        for bad in (-1, 2):
            assert not lib.hipptSetOption(hippt.OPT_ENV_SAMPLING, bad)
            assert lib.hipptGetOption(hippt.OPT_ENV_SAMPLING) == 0
        assert lib.hipptSetOption(hippt.OPT_ENV_SAMPLING, 1)
        assert lib.hipptGetOption(hippt.OPT_ENV_SAMPLING) == 1
        assert lib.hipptGetOption(hippt.INFO_ENV_SAMPLING) == 0  # (nothing rendered)
    finally:
        assert lib.hipptSetOption(hippt.OPT_ENV_SAMPLING, 0)
    assert lib.hipptGetOption(hippt.OPT_ENV_SAMPLING) == 0


def test_python_constants_equal_the_headers():
    header = open(HEADER).read()
    for c_name, value in (("HIPPT_OPT_ENV_SAMPLING", hippt.OPT_ENV_SAMPLING), ("HIPPT_INFO_ENV_SAMPLING", hippt.INFO_ENV_SAMPLING),
                          ("HIPPT_SCENE_ENV_TABLE", hippt.SCENE_ENV_TABLE)):
        m = re.search(rf"\b{c_name} = (\d+)\b", header)
        assert m and int(m.group(1)) == value, c_name
    assert (hippt.OPT_ENV_SAMPLING, hippt.INFO_ENV_SAMPLING, hippt.SCENE_ENV_TABLE) == (40, 111, 6)
    assert hippt.ENV_ROW_DTYPE.itemsize == 8 and hippt.ENV_ROW_DTYPE.names == ("m", "C")
    assert hippt.ENV_TEXEL_DTYPE.itemsize == 12 and hippt.ENV_TEXEL_DTYPE.names == ("q", "c", "k")


def test_the_table_download_is_empty_without_an_environment():
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    assert lib.hipptSetEnvironment(None, 0, 0, ctypes.byref(e))
    assert lib.hipptSceneDownload(hippt.SCENE_ENV_TABLE, None, 0, ctypes.byref(e)) == 0
    E = np.ones((5, 5, 3), F)
    assert lib.hipptSetEnvironment(E.ctypes.data, 5, 0, ctypes.byref(e))
    try:
        assert lib.hipptSceneDownload(hippt.SCENE_ENV_TABLE, None, 0, ctypes.byref(e)) == 4 * (2 * 5 + 3 * 25)
    finally:
        assert lib.hipptSetEnvironment(None, 0, 0, ctypes.byref(e))


# ---- the table ---------------------------------------------------------------------------------------
def test_vectorised_fmaf_is_the_c_librarys():
    from hit_ref import fmaf
    rng = np.random.default_rng(5)
    a = (rng.normal(size=4000) * 10.0 ** rng.uniform(-3, 3, 4000)).astype(F)
    b = (rng.normal(size=4000) * 10.0 ** rng.uniform(-3, 3, 4000)).astype(F)
    c = (-(a.astype(np.float64) * b).astype(F) * (1 + rng.integers(-3, 4, 4000) * F(EPS))).astype(F)  # heavy cancellation
    c[::2] = (rng.normal(size=2000) * 10.0 ** rng.uniform(-3, 3, 2000)).astype(F)
    got = es.vfmaf(a, b, c)
    want = np.array([fmaf(a[i], b[i], c[i]) for i in range(len(a))], F)
    assert got.tobytes() == want.tobytes()


def test_size_1():
    tab = es.table(np.full((1, 1, 3), 0.3, F))
    assert tab["texels"]["q"].tolist() == [[4096]] and tab["rows"]["m"].tolist() == [65536]
    assert tab["rows"]["C"].tolist() == [65536] and tab["texels"]["k"].tolist() == [[0.25]]


@pytest.mark.parametrize("size", [2, 5, 64, 255])
def test_every_texel_and_row_can_be_selected(size):
    tab = es.table(ev.random_env(size, 1))
    assert tab["texels"]["q"].min() >= 1 and tab["rows"]["m"].min() >= 1
    assert tab["texels"]["q"].max() == es.Q_ONE and tab["rows"]["m"].max() == es.M_ONE
    assert (np.diff(tab["rows"]["C"].astype(np.int64)) >= 1).all()
    assert (np.diff(tab["texels"]["c"].astype(np.int64), axis=1) >= 1).all()
    assert (tab["texels"]["k"] > 0).all()


def test_the_totals_fit_at_4096():
    tab = es.table(np.full((4096, 4096, 3), 0.5, F))
    T, R = int(tab["rows"]["C"][-1]), tab["texels"]["c"][:, -1].astype(np.int64)
    assert 4096 <= T <= 1 << 28 and R.min() >= 4096 and R.max() <= 1 << 24
    # (an all-equal map is not all-equal in weight: the solid angle per texel falls towards the corners)
    assert tab["texels"]["q"].max() == es.Q_ONE and tab["texels"]["q"].min() >= 1
    print(f"all-equal 4096^2: T = {T}, R in {R.min()}..{R.max()}")


def test_black_and_invalid_maps_give_the_flat_table():
    size = 7
    black = es.table(np.zeros((size, size, 3), F))
    bad = np.zeros((size, size, 3), F)
    bad[0], bad[1], bad[2:4], bad[4:] = np.nan, -1.0, np.inf, [np.inf, -np.inf, 0.0]
    for tab in (black, es.table(bad)):
        assert (tab["texels"]["q"] == 1).all() and (tab["rows"]["m"] == 1).all()
        assert tab["rows"]["C"].tolist() == list(range(1, size + 1))
        assert (tab["texels"]["c"] == np.arange(1, size + 1, dtype=np.uint32)[None, :]).all()
        k = (F(1.0) / F(size)) * (F(1.0) / F(size)) * (F(0.25) * (F(size) * F(size)))
        assert (tab["texels"]["k"] == k).all()
    # one valid texel among invalid ones takes its row, and its row nearly everything
    bad[3, 2] = (1.0, 2.0, 3.0)
    tab = es.table(bad)
    assert tab["texels"]["q"][3].tolist() == [1, 1, 4096, 1, 1, 1, 1] and tab["rows"]["m"].tolist() == [1, 1, 1, 65536, 1, 1, 1]


def test_one_bright_texel_takes_about_its_share():
    """One texel 10^5 times the others (S = 64): its selection probability m_y q / (T R_y), an exact rational,
    against the share of its W in the sum of W formed in float64.  The ratio is printed; asserted within a factor 2."""
    size, y, x = 64, 40, 21
    E = np.full((size, size, 3), 0.01, F)
    E[y, x] = 1000.0
    tab = es.table(E)
    num, den = es.selection_probability(tab, x, y)
    p = fractions.Fraction(num, den)
    W = es.weights(E).astype(np.float64)
    share = W[y, x] / W.sum()
    ratio = float(p) / share
    print(f"one bright texel: selection probability {float(p):.6f}, share of W {share:.6f}, ratio {ratio:.4f}")
    assert 0.5 < ratio < 2.0


def test_a_sun_on_a_1024_sky_takes_about_its_share():
    """DESIGN.md §20's claim: on a 1024^2 sky a sun of 21 texels at 10^5 times the sky's radiance is selected with
    about the share its power has (one level of 12 bits would give it 21 * 4096 / 2^20 = 8 %)."""
    size = 1024
    E = np.full((size, size, 3), 0.3, F)
    yy, xx = np.mgrid[0:size, 0:size]
    sun = (yy - 600) ** 2 + (xx - 430) ** 2 <= 6
    assert sun.sum() == 21
    E[sun] = 0.3e5
    tab = es.table(E)
    rows, tex = tab["rows"], tab["texels"]
    p = sum(fractions.Fraction(*es.selection_probability(tab, int(x), int(y))) for y, x in np.argwhere(sun))
    W = es.weights(E).astype(np.float64)
    share = W[sun].sum() / W.sum()
    print(f"sun on a 1024^2 sky: selected with probability {float(p):.4f}, its share of the power {share:.4f}")
    assert 0.5 < float(p) / share < 2.0 and share > 0.5
    assert int(rows["C"][-1]) <= 1 << 28 and int(tex["c"][:, -1].max()) <= 1 << 24


@pytest.mark.parametrize("size", [1, 2, 5, 64, 257, 1000])
def test_the_density_integrates_to_one(size):
    """sum k * 4 / S^2 = sum_y (m_y / T) sum_x (q / R_y) = 1 in exact arithmetic.  Each k carries the roundings of
    float(T), two quotients, two products and, for an S that is no power of two, of 0.25 * S^2 folded into one: six
    factors (1 + e), |e| <= 2^-24; summed in float64 the total is within 7 * 2^-24 of 1, whatever S."""
    tab = es.table(ev.random_env(size, 2))
    total = float(tab["texels"]["k"].astype(np.float64).sum() * 4.0 / (size * size))
    print(f"S = {size}: the density integrates to 1 {total - 1.0:+.3e}")
    assert abs(total - 1.0) <= 7 * EPS


# ---- the header's arithmetic, by a stand-alone program ---------------------------------------------------
def check_file(path, E, n_draw, n_miss, seed):
    """Writes the cases of tests/native/env_sample_check.cpp for the map E: the table, draws with their connection
    factors, and miss weights, all by the restatement."""
    size = E.shape[0]
    tab = es.table(E)
    rng = np.random.default_rng(seed)
    words = [np.array([size, n_draw, n_miss, 0], np.uint32), np.ascontiguousarray(E, F).view(np.uint32).reshape(-1),
             tab["rows"].view(np.uint32).reshape(-1), tab["texels"].view(np.uint32).reshape(-1)]
    din, dout = np.zeros((n_draw, 6), np.uint32), np.zeros((n_draw, 10), np.uint32)
    lower = shadow = 0
    for i in range(n_draw):
        state = int(rng.integers(0, 1 << 32))
        n = rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(F)
        sel, mis = F(0.5 if i % 3 == 0 else 1.0), i % 2
        st = ctypes.c_uint32(state)
        dr = es.draw(tab, st)
        g, _ = es.connect_factor(dr["k"], dr["n3"], es.fdot(tuple(n), dr["om"]), sel, mis)
        din[i] = [state, *n.view(np.uint32), sel.view(np.uint32), mis]
        dout[i, :3] = [st.value, dr["x"], dr["y"]]
        dout[i, 3:8] = np.array([*dr["om"], dr["n3"], dr["k"]], F).view(np.uint32)
        dout[i, 8] = g is not None
        dout[i, 9] = F(g if g is not None else 0).view(np.uint32)
        lower += dr["om"][1] < 0
        shadow += g is not None
    min_, mout = np.zeros((n_miss, 5), F), np.zeros(n_miss, F)
    for i in range(n_miss):
        d = (rng.normal(size=3) * 10.0 ** rng.uniform(-1, 1)).astype(F)
        if i % 7 == 0:
            d[rng.integers(0, 3)] = 0.0
        cb = F(rng.uniform(-0.1, 1.0)) if i % 5 else F([0.0, -0.0, np.nan, 1.0][i // 5 % 4])
        sel = F(0.5 if i % 3 == 0 else 1.0)
        min_[i] = [*d, cb, sel]
        mout[i] = es.miss_weight(tab, d, cb, sel)[0]
    words += [din.reshape(-1), dout.reshape(-1), min_.view(np.uint32).reshape(-1), mout.view(np.uint32)]
    with open(path, "wb") as f:
        for w in words:
            f.write(np.ascontiguousarray(w).astype("<u4").tobytes())
    return lower, shadow


def test_the_headers_arithmetic_stand_alone(tmp_path):
    exe = tmp_path / "env_sample_check"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                    "-o", str(exe), os.path.join(REPO, "tests", "native", "env_sample_check.cpp")], check=True)
    bad = np.array(ev.random_env(9, 4))
    bad[0, :3], bad[8, 8] = [[np.nan] * 3, [-1.0] * 3, [np.inf] * 3], 3.0e38
    for name, E in (("s1", np.full((1, 1, 3), 0.7, F)), ("s2", ev.random_env(2, 0)), ("s5", es.test_env(5)),
                    ("s64", es.test_env(64)), ("block", es.test_env(64, "block")), ("s257", ev.random_env(257, 0)),
                    ("black", np.zeros((6, 6, 3), F)), ("bad", bad)):
        path = tmp_path / f"{name}.bin"
        n = 400 if E.shape[0] <= 64 else 100
        lower, shadow = check_file(str(path), E, n, n, 17)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and "env_sample_check ok" in r.stdout, name + ": " + r.stdout + r.stderr
        if name in ("s2", "s5", "s64", "s257"):
            assert 0 < lower < n and 0 < shadow < n, name  # (both hemispheres drawn; faced and backfacing normals)


# ---- the GPU tests' ray sets -------------------------------------------------------------------------------
def counts_of(events):
    return {what: int(np.count_nonzero(events & bit)) for what, bit in es.EVENTS.items()}


ENV_EVENTS = ("env visible", "env occluded", "env backfacing", "lower drawn")


@pytest.mark.parametrize("case", es.PATH_CASES, ids=es.case_id)
def test_the_ray_sets_meet_every_case_of_the_rule(case):
    name, size, kind, select = case
    for mode in (1, 2):
        out = es.case(name, mode, size, kind, select)
        c = counts_of(out[8])
        print(es.case_id(case), "mode", mode, {k: v for k, v in c.items() if v})
        for what in ENV_EVENTS:
            assert c[what] > 0, (mode, what)
        assert c["env infinite g"] == 0  # (cannot happen: envs_ref's last paragraph)
        assert c["unweighted miss after diffuse" if mode == 1 else "weighted miss"] > 0
        if kind == "block":  # (a random map's floor texels weigh about 10^-3 of their rows: not met by 1,025 paths)
            assert c["floor texel"] > 0
        lit = bool(es.scene_of(name)[0].materials()["kind"].tolist().count(hippt.scenes.MAT_EMISSIVE))
        if lit:
            assert c["coin lights"] > 0 and c["coin map"] > 0 and c["visible"] > 0
            if mode == 2:
                assert c["weighted hit"] > 0
        else:
            assert c["coin lights"] == 0 and c["coin map"] == 0
        assert out[9].sum() > 0 and (out[5] > 1).any()


def test_depth_one_makes_no_connection():
    out = es.case("cornell34", 2, 5, "random", False, 1)
    assert not out[9].any() and (out[5] <= 1).all() and not (out[8] & (es.ENV_VISIBLE | es.ENV_OCCLUDED)).any()


def test_without_a_lambertian_vertex_the_paths_are_the_plain_ones():
    """A path that never scatters at a Lambertian surface is env_ref's under the swap, words and segments."""
    from hippt import scenes
    import path_ref as pr
    sc, E, rays, seeds, rad, segs, ends, kinds = es.case("cornell_mixed", 2, 5)[:8]
    plain = pr.PathRef(sc, es.scene_of("cornell_mixed")[1])
    same = (kinds & (1 << scenes.MAT_LAMBERTIAN)) == 0
    assert 50 < same.sum() < len(rays)
    want, wsegs = ev.paths_under(plain, E, rays[same], seeds[same])
    assert rad[same].tobytes() == want.tobytes() and segs[same].tobytes() == wsegs.tobytes()


# ---- same expectation, less noise ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 1])
def test_same_expectation_and_less_variance_on_the_open_box(mode):
    """A condition on the references: the open box under a map with a 2 x 2 block 10^4 times the rest (S = 64), 96
    rays, 12 seeds each.  The means with and without the option agree within 5 standard errors of their difference,
    and the mean per-ray sample variance is lower with it.  Both are printed, not fixed."""
    sc, ref = es.scene_of("open_box")
    E = es.test_env(64, "block")
    rays = es.rays_of("open_box")[0][:96]
    on = es.ref_class(mode)(sc, ref, E)
    off = (mr.MisRef if mode == 2 else nr.NeeRef)(sc, ref)  # (no light: PathRef's paths, under the swap)
    samples = {}
    for what, r in (("on", on), ("off", off)):
        s = np.zeros((12, len(rays), 3))
        for k in range(12):
            seeds = hippt.path_seeds(len(rays), 100 + k)
            if what == "on":
                s[k] = r.paths_events(rays, seeds, 8)[0][:, :3]
            else:
                with ev.swap(E):
                    s[k] = r.paths_events(rays, seeds, 8)[0][:, :3]
        samples[what] = s.mean(axis=2)  # (seed, ray): the channels' mean
    var = {k: float(v.var(axis=0, ddof=1).mean()) for k, v in samples.items()}
    diff = float(samples["on"].mean() - samples["off"].mean())
    se = float(np.sqrt((samples["on"].var(axis=0, ddof=1) + samples["off"].var(axis=0, ddof=1)).sum() / 12) / len(rays))
    print(f"mode {mode}: means {samples['on'].mean():.5f} (on) {samples['off'].mean():.5f} (off), difference {diff:+.5f}, "
          f"standard error {se:.5f}; mean per-ray variance {var['off']:.5f} (off) {var['on']:.5f} (on)")
    assert abs(diff) <= 5 * se
    assert var["on"] < var["off"]
