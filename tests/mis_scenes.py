"""The near-field scene of the MIS tests: where uniform area sampling of a light has no bound and
the power heuristic has one.

  near_field   a closed Lambertian box (0, 0, 0)..(10, 10, 10), albedo 0.73, with one quad lamp
               (4..6, 9.9, 4..6) of emission 15, 0.1 under the ceiling: two triangles, so nLights = 2.  The
               1,024 rays start in the gap above the lamp (y = 9.95, tmin 0) and go up, as lit_scenes.edge_rays
               starts its rays in a gap: their first vertex lies on the ceiling 0.1 above the lamp, where a
               connection's g = A nLights cosS cosL / (pi d2) reaches hundreds.

  huge_lamp    a floor and a lamp of area 2e16 0.01 above it (below): the light hits whose gh^2 overflows, which
               count whole (wb = 1), the one case of the rule that the other ray sets never meet.

The bound B: under the MIS rule every connection adds at most thr' * Le / 2 with thr' <= 1 (the weight
g / (1 + g^2) is at most 1/2 in float32 as in the reals), at most maxDepth - 1 connections are made, and the
final term is at most max(Le, sky) = Le; so no channel of a path exceeds Le * (1 + (maxDepth - 1) / 2), and the
factor 1 + 2^-10 covers the roundings of the float32 sums (at most maxDepth additions, each within 2^-24).
Rays, seeds and references are computed once, shared by the tests and never modified."""
import functools

import numpy as np

import hippt
import mis_ref as mr
import nee_ref as nr
import path_ref as pr
from hippt import scenes

F = np.float32
N_RAYS, MAX_DEPTH, LE, ALBEDO = 1024, 8, 15.0, 0.73
BOUND = LE * (1.0 + (MAX_DEPTH - 1) / 2.0) * (1.0 + 2.0 ** -10)   # 67.5 * (1 + 2^-10)


def near_field():
    tris = scenes._box((0, 0, 0), (10, 10, 10)) + scenes._quad((4.0, 9.9, 4.0), (6.0, 9.9, 4.0), (6.0, 9.9, 6.0),
                                                               (4.0, 9.9, 6.0))
    mats = [(scenes.MAT_LAMBERTIAN, (ALBEDO,) * 3, 0.0, 1.0), (scenes.MAT_EMISSIVE, (LE,) * 3, 0.0, 1.0)]
    sc = scenes._sphere_scene("near_field", [], mats, verts=np.asarray(tris, np.float64).astype(F),
                              tri_mat=[0] * 12 + [1, 1], lookfrom=(5.0, 5.0, 0.5), lookat=(5.0, 9.0, 5.0), vfov=70.0,
                              aperture=0.0, focus=10.0)
    sc.sph_mat = np.zeros(0, np.int32)
    return sc


@functools.lru_cache(maxsize=None)
def scene_refs():
    """(scene, NeeRef, MisRef) of near_field."""
    from test_gpu_ray_query import Ref
    sc = near_field()
    ref = Ref(sc)
    return sc, nr.NeeRef(sc, ref), mr.MisRef(sc, ref)


@functools.lru_cache(maxsize=None)
def rays_seeds():
    rng = np.random.default_rng(37)
    rays = np.zeros((N_RAYS, 8), np.float64)
    rays[:, 0] = rng.uniform(4.0, 6.0, N_RAYS)
    rays[:, 1] = 9.95
    rays[:, 2] = rng.uniform(4.0, 6.0, N_RAYS)
    rays[:, 3], rays[:, 7] = 0.0, np.inf
    rays[:, 4:7] = np.stack([rng.normal(size=N_RAYS), rng.uniform(0.2, 2.0, N_RAYS), rng.normal(size=N_RAYS)], axis=1)
    rays = np.ascontiguousarray(rays, F)
    seeds = hippt.path_seeds(N_RAYS, pr.SEED_FRAME)
    rays.setflags(write=False)
    seeds.setflags(write=False)
    return rays, seeds


@functools.lru_cache(maxsize=None)
def case(mis):
    """(radiance, segments, ends, kinds, events, shadow rays) of the rays under MisRef (mis) or NeeRef."""
    _, nee, ref = scene_refs()
    out = (ref if mis else nee).paths_events(*rays_seeds(), MAX_DEPTH)
    for a in out:
        a.setflags(write=False)
    return out


# ---- a lamp so large and so near that light sampling could not have produced the point hit ----------------
HUGE_RAYS = 128


def huge_lamp():
    """A Lambertian floor triangle in y = 0 and, 0.01 above it, a triangle lamp with legs of 2e8 (area 2e16), each
    with its first corner near the origin, where the rays are (so the triangle test's differences stay small).
    A ray scattered at the floor meets the lamp at d2 = 1e-4 / cos^2, and gh = cos^4 * 6.4e19 there: its square
    overflows for about half the paths, and the hit counts whole (wb = 1)."""
    tris = [(-30.0, 0.0, -30.0) + (4e8, 0.0, -30.0) + (-30.0, 0.0, 4e8),
            (-20.0, 0.01, -20.0) + (2e8, 0.01, -20.0) + (-20.0, 0.01, 2e8)]
    mats = [(scenes.MAT_LAMBERTIAN, (ALBEDO,) * 3, 0.0, 1.0), (scenes.MAT_EMISSIVE, (3.0, 2.0, 1.0), 0.0, 1.0)]
    sc = scenes._sphere_scene("huge_lamp", [], mats, verts=np.asarray(tris, np.float64).astype(F), tri_mat=[0, 1],
                              lookfrom=(0.0, 0.005, -5.0), lookat=(0.0, 0.0, 0.0), vfov=70.0, aperture=0.0, focus=10.0)
    sc.sph_mat = np.zeros(0, np.int32)
    return sc


@functools.lru_cache(maxsize=None)
def huge_case():
    """(scene, rays, seeds, radiance, segments, ends, kinds, events, shadow rays) under MisRef: the rays start
    between the floor and the lamp and go down, with tmin 0."""
    from test_gpu_ray_query import Ref
    sc = huge_lamp()
    rng = np.random.default_rng(41)
    n = HUGE_RAYS
    rays = np.zeros((n, 8), np.float64)
    rays[:, 0], rays[:, 1], rays[:, 2] = rng.uniform(-10.0, 10.0, n), 0.005, rng.uniform(-10.0, 10.0, n)
    rays[:, 3], rays[:, 7] = 0.0, np.inf
    rays[:, 4:7] = np.stack([rng.normal(size=n), -rng.uniform(0.2, 2.0, n), rng.normal(size=n)], axis=1)
    rays = np.ascontiguousarray(rays, F)
    seeds = hippt.path_seeds(n, pr.SEED_FRAME)
    out = mr.MisRef(sc, Ref(sc)).paths_events(rays, seeds, MAX_DEPTH)
    for a in (rays, seeds, *out):
        a.setflags(write=False)
    return (sc, rays, seeds) + out
