"""Light selection by power without a GPU: the option through the ABI, the constants, the properties of the
selection table and of the references of tests/select_ref.py (conditions on the references alone), and that the
GPU tests' ray sets meet every case of the rule."""
import os
import re

import numpy as np
import pytest

import hippt
import lit_scenes as ls
import mis_ref as mr
import nee_ref as nr
import select_ref as sr
import select_scenes as ss

F = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hippt.h")


# ---- the public surface ------------------------------------------------------------------------------
def test_the_option_takes_0_and_1_only_and_reads_back():
    lib = hippt.load_library()
    assert lib.hipptGetOption(hippt.OPT_LIGHT_SELECT) == 0
    try:
        for bad in (-1, 2):
            assert not lib.hipptSetOption(hippt.OPT_LIGHT_SELECT, bad)
            assert lib.hipptGetOption(hippt.OPT_LIGHT_SELECT) == 0
        assert lib.hipptSetOption(hippt.OPT_LIGHT_SELECT, hippt.LIGHT_SELECT_POWER)
        assert lib.hipptGetOption(hippt.OPT_LIGHT_SELECT) == 1
        assert lib.hipptGetOption(hippt.INFO_LIGHT_SELECT) == 0  # (nothing rendered)
    finally:
        assert lib.hipptSetOption(hippt.OPT_LIGHT_SELECT, 0)
    assert lib.hipptGetOption(hippt.OPT_LIGHT_SELECT) == 0


def test_python_constants_equal_the_headers():
    header = open(HEADER).read()
    for c_name, value in (("HIPPT_OPT_LIGHT_SELECT", hippt.OPT_LIGHT_SELECT), ("HIPPT_LIGHT_SELECT_POWER", hippt.LIGHT_SELECT_POWER),
                          ("HIPPT_INFO_LIGHT_SELECT", hippt.INFO_LIGHT_SELECT), ("HIPPT_SCENE_LIGHTS", hippt.SCENE_LIGHTS)):
        m = re.search(rf"\b{c_name} = (\d+)\b", header)
        assert m and int(m.group(1)) == value, c_name
    assert (hippt.OPT_LIGHT_SELECT, hippt.LIGHT_SELECT_POWER, hippt.INFO_LIGHT_SELECT, hippt.SCENE_LIGHTS) == (39, 1, 109, 4)
    assert hippt.LIGHT_TABLE_DTYPE.itemsize == 16 and hippt.LIGHT_TABLE_DTYPE.names == ("prim", "q", "c", "ip")


# ---- the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1000, 65537, sr.LIGHT_MAX])
def test_equal_weights_give_ip_n_exactly(n):
    tab = sr.from_weights(np.arange(n), np.full(n, 0.37, F), np.full(n, 4.5, F))
    assert (tab["q"] == sr.Q_ONE).all() and int(tab["c"][-1]) == n * sr.Q_ONE
    assert (tab["ip"] == F(n)).all()
    assert np.array_equal(tab["c"], (np.arange(1, n + 1, dtype=np.uint64) * sr.Q_ONE).astype(np.uint32))


def test_the_floor_of_1_and_q_0_exactly_for_unlit_lights():
    area = np.array([1.0, 1e-9, 0.0, 1.0, np.nan, 0.25, 1e-3], F)
    y = np.array([8.0, 8.0, 8.0, 0.0, 8.0, 8.0, np.nan], F)
    tab = sr.from_weights(np.arange(7), area, y)
    assert tab["q"].tolist() == [4096, 1, 0, 0, 0, 1024, 0]
    assert tab["c"].tolist() == [4096, 4097, 4097, 4097, 4097, 5121, 5121]
    assert tab["ip"].tolist() == [F(5121) / F(4096), F(5121), 0.0, 0.0, 0.0, F(5121) / F(1024), 0.0]
    # every x below T selects a lit light
    for x in (0, 4095, 4096, 4097, 5120):
        j = int(np.searchsorted(tab["c"], x, side="right"))
        assert tab["q"][j] > 0
    assert sr.select(tab, 0) == 0 and sr.select(tab, 0xFFFFFFFF) == 5


def test_an_infinite_weight_makes_the_table_flat():
    tab = sr.from_weights(np.arange(4), np.array([np.inf, 1.0, 0.0, 1e-20], F), np.array([1.0, 2.0, 3.0, 1e-20], F))
    assert tab["q"].tolist() == [1, 1, 0, 1] and tab["ip"].tolist() == [3.0, 3.0, 0.0, 3.0]
    # (the last light's weight underflows to 0: lit all the same, and alone it makes a flat table too)
    alone = sr.from_weights(np.arange(1), np.array([1e-30], F), np.array([1e-30], F))
    assert alone["q"].tolist() == [1] and alone["ip"].tolist() == [1.0]
    # a finite product that overflows
    over = sr.from_weights(np.arange(2), np.array([1e30, 1.0], F), np.array([1e30, 1.0], F))
    assert over["q"].tolist() == [1, 1]


def test_no_lit_light_gives_t_0():
    sc = sr.scene_refs("all_unlit")[0]
    tab = sr.table(sc)
    assert len(tab) == 3 and not tab["q"].any() and not tab["c"].any() and not tab["ip"].any()
    _, rays, seeds, rad, segs, ends, kinds, events, shadow = sr.case("all_unlit", 2)
    assert (events & sr.NO_LIGHT).any() and not shadow.any()
    assert len(sr.table(ls.scene_refs("light_edges")[0])) == 5


def test_uneven_lamps_is_the_scene_the_issue_asks_for():
    sc = sr.scene_refs("uneven_lamps")[0]
    tab = sr.table(sc)
    n = len(tab)
    assert n > 256 and n % 64 != 0 and n == 304
    assert int((tab["q"] == 0).sum()) == 101  # a third of the small lights emit nothing; one has no area
    assert int((tab["q"] == 1).sum()) > 50 and int(tab["q"].max()) == sr.Q_ONE
    areas = np.array([sr.light_area(sc, int(k)) for k in tab["prim"]])
    small = areas[2:302]
    assert small.min() > 0 and small.max() / small.min() >= 0.99e6
    assert sc.num_spheres == 1 and int(tab["prim"][-1]) == sc.num_tris


# ---- the references ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_one_light_gives_the_uniform_rules_bytes(mode):
    name = "light_edges_one"
    got = sr.case(name, mode)
    want = (ls.nee_case if mode == 1 else mr.mis_case)(name)
    assert got[1].tobytes() == want[1][:ss.RAYS].tobytes()
    tab = sr.scene_refs(name)[1].tab
    assert tab["q"].tolist() == [sr.Q_ONE] and tab["ip"].tolist() == [1.0]
    for k in (3, 4, 5, 6, 8):  # radiance, segments, ends, kinds, shadow rays
        assert got[k].tobytes() == want[k][:ss.RAYS].tobytes(), k


def test_the_ray_sets_meet_every_case_of_the_rule():
    counts = {}
    for name in ("uneven_lamps", "light_edges"):
        ref = sr.scene_refs(name)[2]
        before = ref.zero_q_hits
        events = sr.case(name, 2)[7]
        counts[name] = {
            "floor selected": int(np.count_nonzero(events & sr.FLOOR_SELECTED)),
            "skipped": int(np.count_nonzero(events & (nr.BACKFACING | nr.FAR_SIDE))),
            "weighted hit": int(np.count_nonzero(events & mr.WEIGHTED_HIT)),
            "weighted connection": int(np.count_nonzero(events & mr.WEIGHTED_CONNECTION)),
            "hit on a light with q = 0": ref.zero_q_hits - before,
        }
        print(name, counts[name])
    for what in counts["uneven_lamps"]:
        assert sum(c[what] for c in counts.values()) > 0, what
    assert counts["uneven_lamps"]["floor selected"] > 0 and counts["uneven_lamps"]["weighted hit"] > 0


def test_selection_changes_paths_with_a_lambertian_vertex_only():
    from hippt import scenes
    for mode in (1, 2):
        on, off = sr.case("uneven_lamps", mode, 1), sr.case("uneven_lamps", mode, 0)
        differ = (on[3] != off[3]).any(axis=1)
        same = (off[6] & (1 << scenes.MAT_LAMBERTIAN)) == 0  # no Lambertian vertex: no connection either way
        assert differ.any() and same.any() and not differ[same].any()
        assert np.array_equal(on[4][same], off[4][same])


def test_less_variance_with_selection_on_uneven_lamps():
    """A condition on the reference: over 96 of the set's rays, 12 seeds each, the mean per-ray sample variance
    (over the channels too) of SelectMisRef is below MisRef's.  The ratio is printed, not fixed."""
    sc, _, sel, _, uni = sr.scene_refs("uneven_lamps")
    rays = ss.rays_seeds("uneven_lamps")[0][:96]
    out = {}
    for what, ref in (("selection", sel), ("uniform", uni)):
        samples = np.zeros((12, len(rays), 3))
        for s in range(12):
            seeds = hippt.path_seeds(len(rays), 100 + s)
            samples[s] = ref.paths_events(rays, seeds, 8)[0][:, :3]
        out[what] = float(samples.var(axis=0, ddof=1).mean())
    print(f"mean per-ray variance: uniform {out['uniform']:.5f}, selection {out['selection']:.5f}")
    assert out["selection"] < out["uniform"]
