"""The lit scenes of tests/lit_scenes.py without a GPU: conditions on the references alone, so that the GPU tests
that compare against them (tests/test_gpu_lit_scenes.py) are not vacuous.  Every class of event of the light
sampling rule occurs in every scene's fixed ray set, a connection picks a zero-area light and traces no shadow
ray, the blob's light list is long and scattered, and with sampling disabled the reference is EmitRef's bytes."""
import numpy as np
import pytest

import lit_scenes as ls
import nee_ref as nr
from hippt import scenes

F = np.float32


def recorded_connections(ref, rays, seeds, depth=8):
    """[(light id, Ld or None, vertex p)] of every connection NeeRef makes over the rays."""
    seen = []
    inner = type(ref).connect

    def connect(p, n, thr, st):
        out = inner(ref, p, n, thr, st)
        seen.append((out[2], out[0], p))
        return out
    ref.connect = connect
    try:
        ref.paths_events(rays, seeds, depth)
    finally:
        del ref.connect
    return seen


def areas(sc):
    v = np.asarray(sc.verts, np.float64).reshape(-1, 3, 3)
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


@pytest.mark.parametrize("name", list(ls.SETS))
def test_fixed_ray_sets_meet_every_case_of_the_rule(name):
    sc, rays, seeds, rad, segs, ends, kinds, events, shadow = ls.nee_case(name)
    assert len(rays) == ls.SETS[name][0]
    counts = {what: int(np.count_nonzero(events & bit)) for what, bit in nr.EVENTS.items()}
    print(f"{name}: {len(ls.scene_refs(name)[1].lights)} lights; paths with {counts}; shadow rays "
          f"{int(shadow.sum())} of {int(segs.sum())} segments")
    for what, n in counts.items():
        assert n >= (3 if name.startswith("light_edges") else 10), (name, what, n)
    assert not np.isnan(rad).any() and np.all(rad[:, :3] >= 0)


@pytest.mark.parametrize("name", list(ls.SETS))
def test_with_sampling_disabled_it_is_emit_ref(name):
    sc, rays, seeds, rad, segs, ends, kinds = ls.emit_case(name)
    n = min(len(rays), 1025)  # (the blob: a quarter of its rays, the reference is per ray in Python)
    ref = nr.NeeRef(sc, ls.scene_refs(name)[1].ref, sample=False)
    got, gsegs, gends, gkinds, events, shadow = ref.paths_events(rays[:n], seeds[:n], 8)
    assert got.tobytes() == rad[:n].tobytes() and gsegs.tobytes() == segs[:n].tobytes()
    assert np.array_equal(gends, ends[:n]) and np.array_equal(gkinds, kinds[:n])
    assert not shadow.any() and not (events & ~nr.LIGHT_SPECULAR).any()
    # and light sampling gives other paths
    nrad = ls.nee_case(name)[3]
    assert np.count_nonzero((nrad != rad).any(axis=1)) > len(rays) // 8


def test_the_blobs_light_list_is_long_and_scattered():
    sc, ref, _ = ls.scene_refs("blob64x34_lit")
    assert len(ref.lights) == 273 > 64 and ref.lights[-1] == sc.num_tris  # (the sphere follows the triangles)
    tri_lights = np.asarray(ref.lights[:-1])
    assert np.array_equal(tri_lights, np.arange(10, sc.num_tris, 16))
    assert np.count_nonzero(areas(sc)[tri_lights] == 0) == 8
    # the tree lives in global memory: far more primitives than the LDS scene copy holds (cloud_scene: <= 200)
    assert sc.num_tris == 4362


@pytest.mark.parametrize("name", ["blob64x34_lit", "light_edges"])
def test_a_zero_area_light_is_picked_and_no_shadow_ray_traced(name):
    sc, rays, seeds = ls.nee_case(name)[:3]
    ref = ls.scene_refs(name)[1]
    n = 1025
    seen = recorded_connections(ref, rays[:n], seeds[:n])
    flat = set(np.flatnonzero(areas(sc) == 0).tolist())
    picked = [ld for k, ld, _ in seen if k in flat]
    print(f"{name}: {len(seen)} connections, {len(picked)} of them to a zero-area light")
    assert len(picked) >= 3 and all(ld is None for ld in picked)
    # the draws are consumed all the same: the paths go on, and the recorder changes nothing
    rad = ref.paths_events(rays[:n], seeds[:n], 8)[0]
    assert rad.tobytes() == ls.nee_case(name)[3][:n].tobytes()


def test_light_edges_meets_its_edges():
    """The black light is connected to and adds exactly 0, the 1e30 light gives radiance beyond 1e29 and nothing
    is NaN, vertices under the small triangle 1e-3 above the floor connect to it with a d2 below 1e-4."""
    name = "light_edges"
    sc, rays, seeds, rad = ls.nee_case(name)[:4]
    ref = ls.scene_refs(name)[1]
    assert ref.lights == [24, 25, 26, 27, sc.num_tris + 1]
    em = ref.prim_emission
    assert not em[24].any() and em[26].tolist() == [5.0, 5.0, 5.0] and em[sc.num_tris + 1].tolist() == [F(1e30)] * 3
    seen = recorded_connections(ref, rays, seeds)
    black = [ld for k, ld, _ in seen if k == 24 and ld is not None]
    assert len(black) >= 10 and all(max(ld) == 0.0 for ld in black)
    v0 = np.asarray(sc.verts, np.float64).reshape(-1, 3, 3)[26, 0]
    near = [max(ld) for k, ld, p in seen if k == 26 and ld is not None and np.linalg.norm(np.asarray(p) - v0) < 0.006]
    assert len(near) >= 10 and min(near) > 0.0  # (d2 < 0.006^2 + 0.004^2 + ...: below 1e-4)
    huge = [max(ld) for k, ld, _ in seen if k == sc.num_tris + 1 and ld is not None]
    assert len(huge) >= 10 and max(huge) > 1e29
    assert not np.isnan(rad).any() and float(rad.max()) > 1e29
    print(f"{name}: max radiance {rad.max():.6g}, {np.count_nonzero(np.isinf(rad))} infinite words")


def test_light_edges_one_has_one_light():
    sc, ref, _ = ls.scene_refs("light_edges_one")
    assert ref.lights == [sc.num_tris + 1]


@pytest.mark.parametrize("name", list(ls.SETS))
def test_render_references_make_connections(name):
    sc, acc, px, total, shadow = ls.nee_render(name)
    w, h, frames = ls.SETS[name][1]
    print(f"{name}: {w}x{h}, {frames} frames: {shadow} shadow rays among {total} segments")
    assert acc.shape == (h, w, 4) and px.shape == (h, w) and 50 <= shadow < total
    assert not np.isnan(acc).any()
    eacc = ls.emit_render(name)[1]
    assert np.count_nonzero((acc != eacc).any(axis=-1)) > w * h // 8


def test_random_scene_lit_keeps_its_lens_and_neighbours():
    sc = ls.scene_refs("random_scene_lit")[0]
    base = scenes.random_scene()
    assert sc.aperture == base.aperture == 0.1
    kind = sc.materials()["kind"]
    lit = kind == scenes.MAT_EMISSIVE
    assert np.count_nonzero(lit) == 69 and np.array_equal(kind[~lit], base.materials()["kind"][~lit])
    assert len({tuple(a) for a in sc.materials()["albedo"][lit].tolist()}) == 3
    for k in (scenes.MAT_LAMBERTIAN, scenes.MAT_METAL, scenes.MAT_DIELECTRIC):
        assert np.count_nonzero(kind == k) >= 10
    # the lens: the camera rays of one frame start at many points
    import path_ref as pr
    rays, _ = pr.camera_rays_seeds(sc, 16, 12, 0)
    assert len(np.unique(rays[:, 0:3], axis=0)) > 100
