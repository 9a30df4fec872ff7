"""Light sampling with MIS without a GPU: the reference of tests/mis_ref.py is nee_ref.NeeRef (and so
path_ref.PathRef) over a scene without a light and emit_ref.EmitRef wherever NeeRef is, the GPU tests' ray sets
meet every case of the rule often enough (conditions on the reference alone), the near-field scene shows the
bound that the rule guarantees and that plain light sampling lacks, and the option takes its new value before any
device call.

Counts measured on the reference (paths of each set with the event; 4,097 rays unless said):
  cornell34_lit       weighted connection 3195 (visible 2554, occluded 1308), weighted hit 221, light with cb < 0 60,
                      backfacing 1734, far side 1705
  cornell_mixed_lit   2843 (2374, 1163), 187, 91, 571, 1403
  cornell34_lit_tris  3386 (2761, 1331), 103, 26, 1837, 0 (no sphere light)
  blob64x34_lit       3394 (2203, 2878), 516, 171, 2081, 38
  random_scene_lit    (257 rays) 74 (17, 57), 21, 62, 76, 72
  light_edges         (1,025) 878 (795, 259), 184, 46, 118, 425
  light_edges_one     (1,025) 793 (703, 164), 105, 15, 157, 858
An unweighted hit after a diffuse vertex (wb = 1) needs cb <= 0, a grazing or degenerate light, or an overflowing
gh^2: none of those seven sets has one.  mis_scenes.huge_case, which tests/test_gpu_mis.py also runs bit for bit,
is made for it: 61 of its 128 paths end so (67 on a weighted hit).  g = +inf is met by no set and is built by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import emit_ref as er
import hippt
import lit_scenes as ls
import mis_ref as mr
import mis_scenes as ms
import nee_ref as nr
import path_ref as pr
from hippt import scenes
from test_gpu_ray_query import Ref

F = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hippt.h")
SETS = list(er.LIT) + list(ls.SETS)


# ---- the reference is pinned -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_without_a_light_it_is_nee_ref_and_path_ref(name):
    sc, rays, seeds, rad, segs, ends, kinds = pr.path_case(name)
    ref = mr.MisRef(sc, Ref(sc))
    assert ref.lights == []
    got = ref.paths_events(rays, seeds, pr.MAX_DEPTH)
    want = nr.NeeRef(sc, Ref(sc)).paths_events(rays, seeds, pr.MAX_DEPTH)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert got[0].tobytes() == rad.tobytes() and got[1].tobytes() == segs.tobytes()
    assert np.array_equal(got[2], ends) and np.array_equal(got[3], kinds)
    assert not got[4].any() and not got[5].any()


@pytest.mark.parametrize("name", list(er.LIT))
def test_with_sampling_disabled_it_is_emit_ref(name):
    sc, rays, seeds, rad, segs, ends, kinds = er.emit_case(name)[:7]
    ref = mr.MisRef(sc, Ref(sc), sample=False)
    got, gsegs, gends, gkinds, events, shadow = ref.paths_events(rays, seeds, pr.MAX_DEPTH)
    assert got.tobytes() == rad.tobytes() and gsegs.tobytes() == segs.tobytes()
    assert np.array_equal(gends, ends) and np.array_equal(gkinds, kinds)
    assert not shadow.any() and not (events & ~(nr.LIGHT_SPECULAR)).any()


@pytest.mark.parametrize("name", list(er.LIT))
def test_the_rule_changes_paths_only_after_a_lambertian_vertex(name):
    """A path whose vertices are all Metal or Dielectric, or that has none, is EmitRef's, as NeeRef's is; and a
    path differs from NeeRef's only by its weights: the same segments, ends, shadow rays and draws."""
    sc, rays, seeds, rad, segs, ends, kinds = er.emit_case(name)[:7]
    _, mrays, mseeds, mrad, msegs, mends, mkinds, events, shadow = mr.mis_case(name)
    _, _, _, nrad, nsegs, nends, nkinds, nevents, nshadow = nr.nee_case(name)
    assert mrays.tobytes() == rays.tobytes() and mseeds.tobytes() == seeds.tobytes()
    same = (kinds & (1 << scenes.MAT_LAMBERTIAN)) == 0
    assert same.any() and (~same).any()
    assert mrad[same].tobytes() == rad[same].tobytes() and np.array_equal(msegs[same], segs[same])
    assert mrad[same].tobytes() == nrad[same].tobytes() and not shadow[same].any()
    assert msegs.tobytes() == nsegs.tobytes() and np.array_equal(mends, nends) and np.array_equal(mkinds, nkinds)
    assert shadow.tobytes() == nshadow.tobytes()
    assert np.array_equal(events & (nr.OCCLUDED | nr.BACKFACING | nr.FAR_SIDE | nr.LIGHT_AFTER_DIFFUSE | nr.LIGHT_SPECULAR),
                          nevents & (nr.OCCLUDED | nr.BACKFACING | nr.FAR_SIDE | nr.LIGHT_AFTER_DIFFUSE | nr.LIGHT_SPECULAR))
    assert np.all(np.isfinite(mrad)) and np.all(mrad >= 0)
    assert np.count_nonzero((mrad != nrad).any(axis=1)) > 1000


# ---- the ray sets of the GPU tests are not vacuous ---------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_fixed_ray_sets_meet_the_cases_of_the_rule(name):
    sc, rays, seeds, rad, segs, ends, kinds, events, shadow = mr.mis_case(name)
    counts = {what: int(np.count_nonzero(events & bit)) for what, bit in mr.EVENTS.items()}
    print(f"{name}: paths with {counts}; shadow rays {int(shadow.sum())} of {int(segs.sum())} segments")
    sphere_light = name != "cornell34_lit_tris"
    for what in ("weighted connection", "visible", "occluded", "weighted hit", "light specular", "backfacing", "far side"):
        if what == "far side" and not sphere_light:
            assert counts[what] == 0 and sc.num_spheres == 0
            continue
        assert counts[what] >= 10, (what, counts[what])
    # every shadow ray traced carries the weight; a weighted hit is a light hit after a diffuse vertex
    assert counts["weighted connection"] == int(np.count_nonzero(shadow))
    assert counts["light after diffuse"] == counts["weighted hit"] + counts["unweighted hit after diffuse"]
    # a light met at segment 0 shows its emission itself
    first = (ends == mr.EMITTED) & (segs == 1)
    assert first.any() and np.all(events[first] & mr.LIGHT_SPECULAR)


def test_unweighted_hits_after_a_diffuse_vertex_are_met():
    """wb = 1 after a Lambertian vertex: no set above has one (the module's docstring); the huge lamp's has."""
    total = sum(int(np.count_nonzero(mr.mis_case(name)[7] & mr.UNWEIGHTED_HIT_AFTER_DIFFUSE)) for name in SETS)
    sc, rays, seeds, rad, segs, ends, kinds, events, shadow = ms.huge_case()
    n = int(np.count_nonzero(events & mr.UNWEIGHTED_HIT_AFTER_DIFFUSE))
    print(f"unweighted hits after a diffuse vertex: {total} in the seven sets, {n} of {len(rays)} under the huge lamp")
    assert total + n >= 10 and int(np.count_nonzero(events & mr.WEIGHTED_HIT)) >= 10
    assert np.all(ends == mr.EMITTED) and np.all(np.isfinite(rad))
    # such a path returns its connection (if visible) plus the whole emission: albedo * Le at least
    whole = (events & mr.UNWEIGHTED_HIT_AFTER_DIFFUSE) != 0
    le = np.asarray(sc.albedo[1], F)
    assert np.all(rad[whole, :3] >= F(ms.ALBEDO) * le) and np.all(rad[~whole, :3] < F(ms.ALBEDO) * le * F(1.5) + 1e-3)


def test_an_infinite_g_makes_no_shadow_ray():
    """Built by hand: a lamp of area 2e16 in the plane y = 0 and a vertex 1e-13 under the very point the connection
    draws.  cosS = cosL = 1, d2 = 1e-26, g = A / (pi d2) overflows: option 1 would add +inf, the MIS rule traces no
    shadow ray; from 1 below the same point g is finite and the connection is traced with at most Le / 2."""
    import pyoracle as po
    tris = [(-30.0, -5.0, -30.0) + (30.0, -5.0, -30.0) + (-30.0, -5.0, 30.0),
            (-20.0, 0.0, -20.0) + (2e8, 0.0, -20.0) + (-20.0, 0.0, 2e8)]
    mats = [(scenes.MAT_LAMBERTIAN, (0.5,) * 3, 0.0, 1.0), (scenes.MAT_EMISSIVE, (3.0, 2.0, 1.0), 0.0, 1.0)]
    sc = scenes._sphere_scene("lamp_in_y0", [], mats, verts=np.asarray(tris, np.float64).astype(F), tri_mat=[0, 1])
    sc.sph_mat = np.zeros(0, np.int32)
    ref, nee = mr.MisRef(sc, Ref(sc)), nr.NeeRef(sc, Ref(sc))
    assert ref.lights == [1]
    n, thr = (F(0.0), F(1.0), F(0.0)), (F(1.0), F(1.0), F(1.0))
    skipped = traced = 0
    with np.errstate(all="ignore"):
        for seed in range(16):
            first = ctypes.c_uint32(1000 + 77 * seed)
            drawn = ctypes.c_uint32(first.value)
            po.lib().po_rand01(ctypes.byref(drawn))  # the light choice; then the point
            q = ref.light_point(1, drawn)[0]
            for depth_under, finite in ((F(1e-13), False), (F(1.0), True)):
                p = (q[0], -depth_under, q[2])
                st, st1 = ctypes.c_uint32(first.value), ctypes.c_uint32(first.value)
                ld, om, k, why = ref.connect(p, n, thr, st)
                nld = nee.connect(p, n, thr, st1)[0]
                assert st.value == st1.value == drawn.value and k == 1  # the draws are consumed all the same
                if finite:
                    assert why == 0 and np.all(np.asarray(ld) <= np.asarray(sc.albedo[1], F) * F(0.5))
                    traced += 1
                else:
                    assert why == mr.INFINITE_G and ld is None and np.all(np.isinf(np.asarray(nld)))
                    skipped += 1
    assert skipped == 16 and traced == 16


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depth_limits_on_the_reference(depth):
    sc, rays, seeds, rad, segs, ends, kinds, events, shadow = mr.mis_case("cornell_mixed_lit", depth)
    erad, esegs = er.emit_case("cornell_mixed_lit", depth)[3:5]
    assert int(shadow.max()) == max(0, depth - 1)
    if depth == 1:  # no vertex scatters: EmitRef's words
        assert rad.tobytes() == erad.tobytes() and segs.tobytes() == esegs.tobytes()
    else:
        assert int(np.count_nonzero(events & mr.VISIBLE)) >= 10 and int(segs.max()) == depth + (depth - 1)
    if depth == 2:  # a light hit after the one diffuse vertex now counts, with a weight below 1
        hit = (events & mr.WEIGHTED_HIT) != 0
        assert np.count_nonzero(hit) >= 10 and np.all(rad[hit, :3].max(axis=1) > 0)


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_camera_samples_make_weighted_connections(name):
    sc, acc, px, total, shadow = mr.render_case(name)
    _, nacc, npx, ntotal, nshadow = nr.render_case(name)
    print(f"{name}: 32x24, frames 0..2: {shadow} shadow rays among {total} segments")
    assert (total, shadow) == (ntotal, nshadow) and shadow >= 1000  # the same segments as option 1's render
    assert np.all(acc[..., 3] == 1.0) and np.all(np.isfinite(acc))
    assert np.count_nonzero((acc != nacc).any(axis=-1)) > 24 * 32 // 2


# ---- the near field -------------------------------------------------------------------------------------
def test_near_field_plain_light_sampling_has_no_bound_and_mis_has():
    rays, seeds = ms.rays_seeds()
    assert rays.shape == (ms.N_RAYS, 8) and ms.scene_refs()[2].lights == [12, 13]
    assert abs(ms.BOUND - 67.5 * (1 + 2.0 ** -10)) < 1e-12
    nrad, mrad = ms.case(False)[0], ms.case(True)[0]
    above_n = int(np.count_nonzero(nrad[:, :3].max(axis=1) > ms.BOUND))
    above_m = int(np.count_nonzero(mrad[:, :3].max(axis=1) > ms.BOUND))
    vn, vm = nrad[:, :3].astype(np.float64).var(axis=0, ddof=1), mrad[:, :3].astype(np.float64).var(axis=0, ddof=1)
    print(f"near field: option 1: {above_n} of {ms.N_RAYS} paths above B = {ms.BOUND:.4f}, largest "
          f"{float(nrad[:, :3].max()):.2f}, variance {vn}; option 2: {above_m} above, largest {float(mrad[:, :3].max()):.4f}, "
          f"variance {vm}")
    assert above_n >= ms.N_RAYS // 100 + 1          # 1. at least 1 % of option 1's paths exceed the bound
    assert above_m == 0                             # 2. none of option 2's does: the rule's own guarantee
    assert np.all(vm < vn)                          # 3. and the sample variance is lower, per channel
    ev = ms.case(True)[4]
    assert np.count_nonzero(ev & mr.WEIGHTED_HIT) > ms.N_RAYS // 2 and np.all(ev & mr.WEIGHTED_CONNECTION)


def test_the_weights_of_a_point_add_up_to_one():
    """For one point seen by both techniques the two weights are 1 / (1 + g^2) and g^2 / (1 + g^2) of the same g, in
    float32 to a few ulps: the hit's gh at the point the connection drew is the connection's g."""
    sc, nee, ref = ms.scene_refs()
    n = (F(0.0), F(-1.0), F(0.0))
    p = (F(5.2), F(10.0), F(4.9))
    checked = 0
    with np.errstate(all="ignore"):
        for seed in range(200, 232):
            st, st1 = ctypes.c_uint32(seed * 7919), ctypes.c_uint32(seed * 7919)
            ld, om, k, why = ref.connect(p, n, (F(1), F(1), F(1)), st)
            nld = nee.connect(p, n, (F(1), F(1), F(1)), st1)[0]
            if ld is None:
                continue
            g = float(nld[0]) / ms.LE
            wl = float(ld[0]) / float(nld[0])
            # the same point as a hit of the scattered direction om from p: cb = cosS, t = the distance
            t = F((9.9 - 10.0) / float(om[1]))
            wb, formula = ref.hit_weight(k, t, p, om, F(-float(om[1])))
            assert formula and abs(wl - 1.0 / (1.0 + g * g)) < 1e-5 and abs(float(wb) + wl - 1.0) < 1e-3, (g, wl, wb)
            checked += 1
    assert checked >= 16


# ---- the option ----------------------------------------------------------------------------------------
def test_mode_option_accepts_the_mis_value():
    header = open(HEADER).read()
    assert re.search(r"HIPPT_LIGHT_SAMPLING_MIS\s*=\s*2\b", header) and hippt.LIGHT_SAMPLING_MIS == 2
    assert re.search(r"HIPPT_OPT_LIGHT_SAMPLING_MODE\s*=\s*38\b", header) and hippt.OPT_LIGHT_SAMPLING_MODE == 38
    lib = hippt.load_library()
    lib.cudaPathTracerShutdown()
    mode, onoff = hippt.OPT_LIGHT_SAMPLING_MODE, hippt.OPT_LIGHT_SAMPLING
    assert lib.hipptGetOption(mode) == 0  # the default
    for v in (2, 1, 2, 0):
        assert lib.hipptSetOption(mode, v) and lib.hipptGetOption(mode) == v
        assert lib.hipptGetOption(onoff) == v  # one word behind both keys
    assert lib.hipptSetOption(mode, 2)
    for bad in (-1, 3, 1 << 40):
        assert not lib.hipptSetOption(mode, bad)
        assert lib.hipptGetOption(mode) == 2
    # the on/off key keeps its range (0 and 1) and writes the same word
    assert not lib.hipptSetOption(onoff, 2) and lib.hipptGetOption(mode) == 2
    assert lib.hipptSetOption(onoff, 1) and lib.hipptGetOption(mode) == 1
    assert lib.hipptSetOption(mode, 2) and lib.hipptSetOption(onoff, 0) and lib.hipptGetOption(mode) == 0
    assert lib.hipptGetOption(hippt.INFO_LIGHT_SAMPLING) == 0


def test_cpp_host_knows_the_mis_flag():
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    r = subprocess.run([exe, "--no-such-option", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mis" in r.stderr
    r = subprocess.run([exe, "--mis", "--backend", "none"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2  # "--backend none" was parsed (and rejected), not taken as the flag's value
