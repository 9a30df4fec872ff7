"""Ray and path queries (GPU) on the far-ray families of tests/far_rays.py: origins up to 2^20 M from
the scene, directions of length 2^-100..2^80, directions with zero and near-zero components, far rays
that pass the scene by, and tmin / tmax set on and one float past a far ray's hit.  Every comparison is
bit for bit against the oracle's closest hit (test_gpu_ray_query.Ref.closest), the hit records
(hit_ref.HitRef) and the paths (path_ref.PathRef, emit_ref.EmitRef); tests/test_far_rays_cpu.py asserts
on the references alone that these cells hold hits, walls and answers that change.

The box test only culls: what these tests catch is a box that culls a ray whose oracle hit lies under
it, which the builder's pad alone allows from a few hundred M on and for directions shorter than the
1e-20 clamp (DESIGN.md §5 "query slack")."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import emit_ref
import far_rays as fr
import hippt
import path_ref as pr
from hit_ref import HitRef, assert_records
from refit_util import verts_of, with_verts, wobble
from test_gpu_ray_query import Ref, pt, upload  # noqa: F401 (pt: the fixture)

pytestmark = pytest.mark.gpu


def assert_cells(case, t, prim, what, rt=None, rp=None, cells=None):
    """t's bytes and prim equal to the reference's, reported per cell (the case's own reference: but for
    its rays whose reference hit is a triangle without area, Case.noise)."""
    own = rt is None
    rt, rp = (case.t, case.prim) if own else (rt, rp)
    t, prim = np.asarray(t), np.asarray(prim)
    assert t.dtype == np.float32 and prim.dtype == np.int32 and t.shape == rt.shape and prim.shape == rp.shape
    bad = (t.view(np.uint32) != rt.view(np.uint32)) | (prim != rp)
    if own:
        bad &= ~case.noise
    if bad.any():
        lines = []
        for c in cells or case.cells:
            k = np.flatnonzero(bad[c.sl])
            if k.size:
                i = c.start + k[0]
                lines.append(f"{c.label}: {k.size} of {c.stop - c.start} differ (oracle hits: "
                             f"{np.count_nonzero(rp[c.sl] >= 0)}); ray {i}: t {t[i]!r} prim {prim[i]} "
                             f"vs {rt[i]!r} {rp[i]}")
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} of {bad.size} rays differ\n" + "\n".join(lines))


def keep(case, a):
    """a without the rays that are not compared (Case.noise)."""
    return np.asarray(a)[~case.noise]


# ---- 1. closest hit, occlusion, hit records: every family -------------------------------------------
@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", list(fr.SCENES))
def test_every_family_matches_the_oracle(pt, name, lds, width):
    c = fr.far_case(name)
    upload(pt, c.sc, lds, width)
    t, prim = pt.traceRays(c.rays)
    assert_cells(c, t, prim, f"{name} lds={lds} width={width}")
    assert np.array_equal(keep(c, pt.occluded(c.rays)), keep(c, c.prim >= 0).astype(np.uint8))
    hits = pt.traceHits(c.rays)
    assert_records(keep(c, hits), keep(c, fr.hit_records(name)), f"{name} lds={lds} width={width}")
    # the miss encoding, for the rays that pass the scene by too
    miss = np.flatnonzero(c.prim < 0)
    assert np.all(np.isinf(t[miss])) and np.all(prim[miss] == -1) and np.all(hits["matFlags"][miss] == -1)
    assert not hits["normal"][miss].any() and not hits["u"][miss].any() and not hits["v"][miss].any()


def test_odd_slices_give_the_same_bytes(pt):
    c = fr.far_case("cornell_mixed")
    upload(pt, c.sc)
    pt.setOption(hippt.OPT_QUERY_SLICE, 777)
    t, prim = pt.traceRays(c.rays)
    assert_cells(c, t, prim, "slice 777")
    assert np.array_equal(pt.occluded(c.rays), (c.prim >= 0).astype(np.uint8))
    assert_records(pt.traceHits(c.rays), fr.hit_records("cornell_mixed"), "slice 777")


def test_device_tensors(pt):
    assert torch.cuda.is_available()
    c = fr.far_case("blob64x34")
    pt.setDevices([0])
    upload(pt, c.sc, 0)
    dr = torch.from_numpy(np.array(c.rays)).to(torch.device("cuda", 0))
    t, prim = pt.traceRays(dr)
    assert_cells(c, t.cpu().numpy(), prim.cpu().numpy(), "device rays")
    assert np.array_equal(keep(c, pt.occluded(dr).cpu().numpy()), keep(c, c.prim >= 0).astype(np.uint8))
    rec = pt.traceHits(dr).cpu().numpy().view(hippt.HIT_DTYPE).reshape(-1)
    assert_records(keep(c, rec), keep(c, fr.hit_records("blob64x34")), "device rays")
    del dr, t, prim


# ---- 2. path queries: only segment 0 is far ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_case(name, depth):
    """(scene, rays, seeds, radiance, segments, cells) of the path cells of cornell_mixed's families over
    cornell_mixed or its lit variant; computed once, never modified."""
    c = fr.far_case("cornell_mixed")
    cells = fr.path_cells(c)
    rays = np.ascontiguousarray(np.concatenate([c.rays[x.sl] for x in cells]))
    at, moved = 0, []
    for x in cells:
        moved.append(dataclasses.replace(x, start=at, stop=at + x.stop - x.start))
        at = moved[-1].stop
    if name == "cornell_mixed":
        sc, ref = c.sc, pr.PathRef(c.sc, c.ref)
    else:
        sc = emit_ref.lit_scene(name)
        ref = emit_ref.EmitRef(sc, Ref(sc))
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    rad, segs = ref.paths(rays, seeds, depth)[:2]
    for a in (rays, seeds, rad, segs):
        a.setflags(write=False)
    return sc, rays, seeds, rad, segs, tuple(moved)


@pytest.mark.parametrize("depth", [8, 1])
@pytest.mark.parametrize("name", ["cornell_mixed", "cornell_mixed_lit"])
def test_radiance_from_far_and_scaled_rays(pt, name, depth):
    sc, rays, seeds, want_rad, want_segs, cells = path_case(name, depth)
    # a condition on the reference alone: in every cell most paths hit with segment 0, and at depth 8
    # most go on from there (so the segments after the far one are traced too)
    for x in cells:
        n = x.stop - x.start
        assert 2 * np.count_nonzero(want_rad[x.sl, 3] == 1.0) >= n, x.label
        if depth == 8:
            assert 2 * np.count_nonzero(want_segs[x.sl] >= 2) >= n, x.label
    for lds, width in ((1, 4), (0, 2)):
        upload(pt, sc, lds, width)
        rad, segs = pt.traceRadiance(rays, seeds, depth)
        rad, segs = np.asarray(rad), np.asarray(segs)
        bad = (rad.view(np.uint32) != want_rad.view(np.uint32)).any(axis=1) | (segs != want_segs)
        lines = [f"{x.label}: {np.count_nonzero(bad[x.sl])} of {x.stop - x.start} paths differ"
                 for x in cells if bad[x.sl].any()]
        assert not lines, f"{name} depth {depth} lds={lds} width={width}\n" + "\n".join(lines)
        pr.assert_paths(rad, segs, want_rad, want_segs, f"{name} depth {depth}")


# ---- 3. the far camera -------------------------------------------------------------------------------
def test_far_camera_queries(pt):
    """hipptSetCamera to 4096 M with a long lens on the room: the camera's first hits, hit records and
    paths are the oracle's of the camera's own rays."""
    w, h = 40, 30
    c = fr.far_case("cornell34")
    far = dataclasses.replace(c.sc, lookfrom=(278.0, 278.0, -4096.0 * c.M), vfov=0.008)
    upload(pt, c.sc, w=w, h=h)
    cam = hippt.build_camera(lookfrom=far.lookfrom, lookat=far.lookat, vup=far.vup, vfov=far.vfov, aspect=w / h,
                             aperture=far.aperture, focus=far.focus)
    err = ctypes.c_char_p()
    assert hippt.load_library().hipptSetCamera(ctypes.byref(cam), ctypes.byref(err)), err.value
    rays, seeds = pr.camera_rays_seeds(far, w, h, 0)
    rt, rp = c.ref.closest(rays)
    assert 2 * np.count_nonzero(rp >= 0) >= rp.size  # the lens is on the room
    got_rays, got_seeds = pt.cameraRays(0)
    assert got_rays.tobytes() == rays.tobytes() and np.array_equal(got_seeds, seeds)
    t, prim = pt.traceCamera(0)
    whole = fr.Cell("camera", 4096.0, 1.0, "", 0, rp.size)
    assert_cells(c, t.reshape(-1), prim.reshape(-1), "far camera", rt, rp, [whole])
    assert_records(pt.traceCameraHits(0), HitRef(c.sc, c.ref).records(rays, rt, rp), "far camera")
    want_rad, want_segs = pr.PathRef(c.sc, c.ref).paths(rays, seeds, 8)[:2]
    rad, segs = pt.traceRadiance(rays, seeds, 8)
    pr.assert_paths(rad, segs, want_rad, want_segs, "far camera paths")


# ---- 4. after a refit --------------------------------------------------------------------------------
def test_far_rays_after_a_vertex_update(pt):
    """The refit rewrites the boxes and the pad word the queries read M from: the wobbled mesh, then the
    first vertices again, whose flat walls then sit in boxes the refit made."""
    c = fr.far_case("cornell34")
    cells = c.of("far", K=4096.0)
    rays = np.ascontiguousarray(np.concatenate([c.rays[x.sl] for x in cells]))
    v1 = wobble(verts_of(c.sc))
    sc1 = with_verts(c.sc, v1)
    ref = Ref(sc1)
    rt, rp = ref.closest(rays)
    before = np.concatenate([c.t[x.sl] for x in cells])
    assert 2 * np.count_nonzero(rp >= 0) >= rp.size and 2 * np.count_nonzero(rt != before) >= rp.size
    for lds in (1, 0):
        upload(pt, c.sc, lds)
        pt.updateVertices(v1)
        t, prim = pt.traceRays(rays)
        whole = fr.Cell("far", 4096.0, 0.0, "refit", 0, rp.size)
        assert_cells(c, t, prim, f"after updateVertices lds={lds}", rt, rp, [whole])
        assert np.array_equal(pt.occluded(rays), (rp >= 0).astype(np.uint8))
        assert_records(pt.traceHits(rays), HitRef(sc1, ref).records(rays, rt, rp), "after updateVertices")
        pt.updateVertices(verts_of(c.sc))
        t, prim = pt.traceRays(rays)
        back = np.concatenate([c.prim[x.sl] for x in cells])
        assert_cells(c, t, prim, f"first vertices again lds={lds}", before, back, [whole])
