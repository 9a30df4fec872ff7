"""Emissive materials without a GPU: the reference of tests/emit_ref.py is path_ref.PathRef wherever no
light is met and throughput x emission where one is, hipptUploadScene accepts HIPPT_MAT_EMISSIVE and rejects a
negative emission before any device call, and the GPU tests' ray sets and camera samples end on lights often
enough (conditions on the reference alone)."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emit_ref as er
import hippt
import path_ref as pr
from hippt import scenes
from test_gpu_ray_query import Ref

F = np.float32


# ---- the scenes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["cornell34", "cornell_mixed"])
@pytest.mark.parametrize("sphere", [True, False])
def test_cornell_lit_is_the_base_scene_plus_the_lamp(base, sphere):
    b = scenes.get_scene(base)
    sc = scenes.cornell_lit(base, sphere)
    assert sc.name == f"{base}_lit" and sc.name not in scenes.SCENES
    bm, m = b.materials(), sc.materials()
    k = len(bm)
    assert sc.num_tris == b.num_tris + 2 and sc.num_spheres == b.num_spheres + int(sphere)
    assert sc.verts[:b.num_tris].tobytes() == np.ascontiguousarray(b.verts, F).tobytes()
    assert sc.verts.dtype == np.float32 and sc.tri_mat.dtype == np.int32 and sc.sph_mat.dtype == np.int32
    quad = np.asarray(scenes._quad((213, 554, 227), (343, 554, 227), (343, 554, 332), (213, 554, 332)), F)
    assert np.array_equal(sc.verts[b.num_tris:], quad) and list(sc.tri_mat[b.num_tris:]) == [k, k]
    assert m[:k].tobytes() == bm.tobytes() and len(m) == k + 1 + int(sphere)
    assert m["kind"][k] == scenes.MAT_EMISSIVE == hippt.MAT_EMISSIVE == 3 and tuple(m["albedo"][k]) == (15.0, 15.0, 15.0)
    if sphere:
        assert tuple(sc.spheres[-1]) == (90.0, 400.0, 400.0, 40.0) and sc.sph_mat[-1] == k + 1
        assert m["kind"][k + 1] == scenes.MAT_EMISSIVE and tuple(m["albedo"][k + 1]) == (4.0, 2.0, 1.0)
    assert (sc.lookfrom, sc.lookat, sc.vfov, sc.aperture) == (b.lookfrom, b.lookat, b.vfov, b.aperture)
    assert not sc.lambertian_triangles


def test_scene_file_round_trips_the_emissive_kind(tmp_path):
    sc = scenes.cornell_lit("cornell_mixed")
    path = str(tmp_path / "lit.scene")
    scenes.write_scene_file(sc, path)
    back = scenes.load_scene_file(path)
    assert back.materials().tobytes() == sc.materials().tobytes()
    assert back.verts.tobytes() == sc.verts.tobytes() and back.spheres.tobytes() == sc.spheres.tobytes()
    assert np.array_equal(back.tri_mat, sc.tri_mat) and np.array_equal(back.sph_mat, sc.sph_mat)


# ---- the reference is pinned -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_without_a_light_it_is_path_ref(name):
    _, rays, seeds, rad, segs, ends, kinds = pr.path_case(name)
    _, erays, eseeds, erad, esegs, eends, ekinds, _, _ = er.emit_case(name)
    assert erays.tobytes() == rays.tobytes() and eseeds.tobytes() == seeds.tobytes()
    assert erad.tobytes() == rad.tobytes() and esegs.tobytes() == segs.tobytes()
    assert np.array_equal(eends, ends) and np.array_equal(ekinds, kinds)
    assert not np.any(eends == er.EMITTED)


@pytest.mark.parametrize("name", list(er.LIT))
def test_lit_scenes_differ_from_path_ref_only_at_lights(name):
    sc, rays, seeds, rad, segs, ends, kinds, thr, prim = er.emit_case(name)
    sub = er.lambertian_substitute(sc)
    assert not np.any(sub.materials()["kind"] == scenes.MAT_EMISSIVE)
    want, wsegs, wends, wkinds = pr.PathRef(sub, Ref(sc)).paths(rays, seeds, pr.MAX_DEPTH)
    m = sc.materials()
    emissive = np.flatnonzero(m["kind"] == scenes.MAT_EMISSIVE)
    kind_of = np.concatenate([m["kind"][sc.tri_mat], m["kind"][sc.sph_mat]])
    emission_of = np.concatenate([m["albedo"][sc.tri_mat], m["albedo"][sc.sph_mat]]).astype(F)
    lit = ends == er.EMITTED
    # a path that never meets a light: the oracle's path over the substituted scene, bit for bit
    assert rad[~lit].tobytes() == want[~lit].tobytes() and np.array_equal(segs[~lit], wsegs[~lit])
    assert np.array_equal(ends[~lit], wends[~lit]) and np.array_equal(kinds[~lit], wkinds[~lit])
    # (the substituted scene scatters at the light: that path is at least as long, with the same prefix)
    assert np.all(wsegs[lit] >= segs[lit])
    assert not np.any(kinds & (1 << scenes.MAT_EMISSIVE))  # no path scatters at a light
    # a path ended by a light: its last hit is a light, rgb = throughput of the prefix x emission in float32
    assert lit.any() and np.all(np.isin(kind_of[prim[lit]], [scenes.MAT_EMISSIVE]))
    assert len(emissive) == (2 if er.LIT[name][1] else 1)
    with np.errstate(all="ignore"):
        product = thr[lit] * emission_of[prim[lit]]
    assert product.dtype == np.float32 and np.ascontiguousarray(rad[lit, :3]).tobytes() == product.tobytes()
    first = lit & (segs == 1)
    assert np.all(thr[first] == 1.0) and np.all(rad[first, 3] == 1.0)
    assert np.ascontiguousarray(rad[first, :3]).tobytes() == emission_of[prim[first]].tobytes()
    # a = 1 exactly when segment 0 hit: where a path's first segment missed it has one segment and ended in the sky
    assert np.array_equal(rad[:, 3] == 0.0, (ends == er.INVALID) | ((ends == er.MISS) & (segs == 1)))
    # every other path that does not end on a light never hit one
    hit_light = np.isin(kind_of[np.maximum(prim, 0)], [scenes.MAT_EMISSIVE]) & (prim >= 0)
    assert np.array_equal(hit_light, lit)


# ---- the ray sets of the GPU tests are not vacuous ---------------------------------------------------
MIN_ENDS = {"cornell34_lit": (40, 150, 10, 100), "cornell_mixed_lit": (40, 150, 10, 100), "cornell34_lit_tris": (15, 60, 3, None)}


@pytest.mark.parametrize("name", list(er.LIT))
def test_fixed_ray_sets_end_on_lights(name):
    sc, rays, seeds, rad, segs, ends, kinds, thr, prim = er.emit_case(name)
    lit = ends == er.EMITTED
    at0 = int(np.count_nonzero(lit & (segs == 1)))
    later = int(np.count_nonzero(lit & (segs > 1)))
    last = int(np.count_nonzero(lit & (segs == pr.MAX_DEPTH)))
    on_sphere = int(np.count_nonzero(lit & (prim >= sc.num_tris)))
    print(f"{name}: ended on a light at segment 0: {at0}, later: {later}, on segment {pr.MAX_DEPTH}: {last}, "
          f"on the sphere: {on_sphere}")
    m0, m1, m2, m3 = MIN_ENDS[name]
    assert at0 >= m0 and later >= m1 and last >= m2
    if m3 is None:
        assert on_sphere == 0 and sc.num_spheres == 0  # triangles only: what a FULL = false dispatch would trace
    else:
        assert on_sphere >= m3
    # a later ending carries a throughput other than (1, 1, 1): the product is not the emission itself.  The
    # one exception is a path that reached the light through Dielectric hits alone (attenuation 1: 2 of
    # cornell_mixed_lit's 228 later endings): its throughput is exactly (1, 1, 1).
    glass_only = lit & (segs > 1) & (kinds == 1 << scenes.MAT_DIELECTRIC)
    attenuated = lit & (segs > 1) & ~glass_only
    assert np.all((thr[attenuated] != 1.0).any(axis=1)) and np.all(thr[glass_only] == 1.0)
    assert int(np.count_nonzero(attenuated)) >= m1
    assert not glass_only.any() or name == "cornell_mixed_lit"
    # the eighth segment's light is lit although the depth limit would have ended the path black there
    assert rad[lit & (segs == pr.MAX_DEPTH), :3].any(axis=1).all()


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_camera_samples_end_on_lights(name):
    sc, acc, px, total, ends, nseg = er.render_case(name)
    lit = ends == er.EMITTED
    at0, later = int(np.count_nonzero(lit & (nseg == 1))), int(np.count_nonzero(lit & (nseg > 1)))
    print(f"{name}: 32x24, frames 0..2: ended on a light at segment 0: {at0}, later: {later}")
    assert at0 >= 15 and later >= 50
    assert total == int(nseg.sum()) and acc.shape == (24, 32, 4) and px.shape == (24, 32)
    assert np.all(acc[..., 3] == 1.0) and float(acc[..., :3].max()) > 1.0  # a lamp pixel's average exceeds 1


def test_cpp_host_emit_option_names_a_group_of_the_mesh(tmp_path):
    """hippt_render --emit: a name that is no `usemtl` group of the OBJ, or a malformed radiance, is an error
    before any device call."""
    sc = scenes.cornell_lit("cornell34", sphere=False)
    obj = tmp_path / "lit.obj"
    scenes.write_obj(sc, str(obj), style="plain")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    for emit in ("lamp=15,15,15", "m3=15,15", "m3", "m3=15,15,15;m9=1,1,1"):
        r = subprocess.run([exe, "--mesh", str(obj), "--emit", emit, "--width", "8", "--height", "8", "--spp", "1"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "emit needs NAME=r,g,b" in r.stderr, (emit, r.stderr)
    r = subprocess.run([exe, "--mesh", str(obj), "--emit", "m3=-1,15,15", "--width", "8", "--height", "8", "--spp", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "negative emission component" in r.stderr, r.stderr


# ---- upload through the C ABI: no Init, no device ----------------------------------------------------
def test_upload_accepts_emissive_and_rejects_a_negative_emission():
    lib = hippt.load_library()
    lib.cudaPathTracerShutdown()
    pt = hippt.PathTracer()
    pt.resetStats()
    sc = scenes.cornell_lit("cornell_mixed")
    k = len(sc.materials()) - 2
    pt.uploadMesh(scenes.cornell_lit("cornell34", sphere=False))  # (uploadMesh passes it on to hipptUploadScene)
    pt.uploadScene(sc)  # kind 3 is accepted
    before = pt.stats()
    assert before["numTris"] == sc.num_tris + sc.num_spheres

    def variant(**fields):
        v = copy.copy(sc)
        for name, (index, value) in fields.items():
            a = np.array(getattr(sc, name))
            a[index] = value
            setattr(v, name, a)
        return v

    for c in range(3):
        with pytest.raises(hippt.HipptError, match="negative emission component"):
            pt.uploadScene(variant(albedo=((k + c % 2, c), -0.25)))
    with pytest.raises(hippt.HipptError, match="non-finite material parameter"):
        pt.uploadScene(variant(albedo=((k, 1), np.nan)))
    with pytest.raises(hippt.HipptError, match="non-finite material parameter"):
        pt.uploadScene(variant(albedo=((k, 0), np.inf)))
    with pytest.raises(hippt.HipptError, match="non-finite material parameter"):
        pt.uploadScene(variant(fuzz=(k, np.nan)))  # ignored by the material, finite all the same
    with pytest.raises(hippt.HipptError, match="unknown material kind"):
        pt.uploadScene(variant(mat_kind=(k, 4)))
    with pytest.raises(hippt.HipptError, match="unknown material kind"):
        pt.uploadScene(variant(mat_kind=(0, -1)))
    # a rejected upload leaves the statistics (the scene's among them) and a later upload alone
    assert pt.stats() == before
    # a negative albedo of another kind is none of this check's business (as before)
    pt.uploadScene(variant(albedo=((0, 0), -0.25)))
    # an absorber (0, 0, 0), -0 and a radiance far above 1 are emissions
    pt.uploadScene(variant(albedo=((k, slice(None)), 0.0)))
    pt.uploadScene(variant(albedo=((k, 2), -0.0)))
    pt.uploadScene(variant(albedo=((k, 0), 3.0e38)))
    pt.uploadScene(sc)
    assert pt.stats() == before
    # hipptMaterial keeps its 24 bytes
    assert scenes.MATERIAL_DTYPE.itemsize == 24
    # no device was touched: the state is still "not initialized"
    e = ctypes.c_char_p()
    rays, out = np.zeros((1, 8), np.float32), np.zeros((1, 4), np.float32)
    seeds = np.zeros(1, np.uint32)
    assert not lib.hipptTraceRadiance(rays.ctypes.data, seeds.ctypes.data, 1, 8, 0, out.ctypes.data, None, ctypes.byref(e))
    assert b"not initialized" in e.value
    lib.cudaPathTracerShutdown()
