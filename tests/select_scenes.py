"""Scenes for light selection by power (tests/select_ref.py): lights of very different area and emission.

  uneven_lamps  a closed Lambertian box (0, 0, 0)..(10, 10, 10) holding one large bright quad lamp under the
                ceiling (two triangles of area 8, emission 30), 300 small triangle lights on the floor and the
                walls whose areas span six decades (5e-7 .. 0.5) with three emissions in turn, one of them
                (0, 0, 0), one triangle light of zero area and one small sphere light: 304 lights, more than one
                block of 256 and no multiple of 64.
  all_unlit     the box with three lights none of which can add anything: a triangle of emission (0, 0, 0), a
                triangle of zero area and a sphere of emission (0, 0, 0).  T == 0.
  many_lights   (n, seed): n small emissive triangles over a Lambertian floor quad, from a seeded generator:
                areas over eight decades, three emissions in turn, one of them (0, 0, 0), and for n >= 3 one
                degenerate triangle (index n // 2).  The table test's scenes.

A scene's rays and seeds are computed once and never modified."""
import functools

import numpy as np

import hippt
import lit_scenes as ls
import path_ref as pr
from hippt import scenes

F = np.float32
RAYS = 1025
LAMP_EMISSION = (30.0, 30.0, 30.0)
SMALL_EMISSIONS = ((2.0, 1.5, 1.0), (0.0, 0.0, 0.0), (0.5, 1.0, 3.0))
SMALL = 300


def _box_scene(name, tris, tmat, mats, spheres, smat):
    sc = scenes._sphere_scene(name, spheres, mats, verts=np.asarray(tris, np.float64).astype(F), tri_mat=tmat,
                              lookfrom=(5.0, 5.0, 0.5), lookat=(5.0, 4.0, 9.0), vfov=80.0, aperture=0.0, focus=10.0)
    sc.sph_mat = np.asarray(smat, np.int32)
    return sc


def uneven_lamps():
    rng = np.random.default_rng(41)
    tris = scenes._box((0, 0, 0), (10, 10, 10))
    tmat = [0] * len(tris)
    mats = [(scenes.MAT_LAMBERTIAN, (0.7, 0.65, 0.6), 0.0, 1.0), (scenes.MAT_EMISSIVE, LAMP_EMISSION, 0.0, 1.0)]
    mats += [(scenes.MAT_EMISSIVE, le, 0.0, 1.0) for le in SMALL_EMISSIONS]
    lamp = scenes._quad((3.0, 9.9, 3.0), (7.0, 9.9, 3.0), (7.0, 9.9, 7.0), (3.0, 9.9, 7.0))
    tris += lamp
    tmat += [1] * len(lamp)
    # (wall: the fixed axis, its coordinate 0.02 inside the box; the triangle's legs run along the other two)
    walls = ((1, 0.02), (0, 0.02), (0, 9.98), (2, 0.02), (2, 9.98))
    for i in range(SMALL):
        side = 10.0 ** (-3.0 + 3.0 * i / (SMALL - 1))
        axis, at = walls[i % len(walls)]
        u, v = [a for a in range(3) if a != axis]
        p = np.zeros(3)
        p[axis] = at
        p[u], p[v] = rng.uniform(0.5, 8.5, 2)
        a, b = p.copy(), p.copy()
        a[u] += side
        b[v] += side
        tris.append(tuple(p) + tuple(a) + tuple(b))
        tmat.append(2 + i % 3)
    tris.append((4.0, 5.0, 9.0) + (5.0, 5.5, 9.0) + (6.0, 6.0, 9.0))  # zero area
    tmat.append(2)
    mats.append((scenes.MAT_EMISSIVE, (3.0, 3.0, 3.0), 0.0, 1.0))
    return _box_scene("uneven_lamps", tris, tmat, mats, [(2.0, 2.0, 7.5, 0.4)], [len(mats) - 1])


def all_unlit():
    tris = scenes._box((0, 0, 0), (10, 10, 10))
    tmat = [0] * len(tris)
    mats = [(scenes.MAT_LAMBERTIAN, (0.7, 0.65, 0.6), 0.0, 1.0), (scenes.MAT_EMISSIVE, (0.0, 0.0, 0.0), 0.0, 1.0),
            (scenes.MAT_EMISSIVE, (3.0, 3.0, 3.0), 0.0, 1.0)]
    tris.append((3.0, 9.5, 3.0) + (7.0, 9.5, 3.0) + (7.0, 9.5, 7.0))  # emits nothing
    tmat.append(1)
    tris.append((4.0, 5.0, 9.0) + (5.0, 5.5, 9.0) + (6.0, 6.0, 9.0))  # zero area
    tmat.append(2)
    return _box_scene("all_unlit", tris, tmat, mats, [(2.0, 2.0, 7.5, 0.8)], [1])


def many_lights(n, seed=5):
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(5.0, 95.0, size=(n, 1, 3))
    side = 10.0 ** rng.uniform(-4.0, 0.0, size=(n, 1, 1))
    legs = rng.normal(size=(n, 2, 3))
    legs /= np.linalg.norm(legs, axis=2, keepdims=True)
    v = np.concatenate([c, c + side * legs], axis=1)
    if n >= 3:
        v[n // 2, 1] = v[n // 2, 0]  # two corners in one point: both cross products' terms are exact zeros
    floor = np.asarray(scenes._quad((0.0, 0.0, 0.0), (100.0, 0.0, 0.0), (100.0, 0.0, 100.0), (0.0, 0.0, 100.0)))
    verts = np.concatenate([v.reshape(n, 9), floor.reshape(2, 9)]).astype(F)
    tmat = np.concatenate([1 + np.arange(n) % 3, [0, 0]]).astype(np.int32)
    mats = [(scenes.MAT_LAMBERTIAN, (0.6, 0.6, 0.6), 0.0, 1.0), (scenes.MAT_EMISSIVE, (5.0, 4.0, 3.0), 0.0, 1.0),
            (scenes.MAT_EMISSIVE, (0.0, 0.0, 0.0), 0.0, 1.0), (scenes.MAT_EMISSIVE, (0.25, 0.5, 2.0), 0.0, 1.0)]
    sc = scenes._sphere_scene(f"many_lights{n}", [], mats, verts=verts, tri_mat=tmat, lookfrom=(50.0, 60.0, -120.0),
                              lookat=(50.0, 40.0, 50.0), vfov=50.0, aperture=0.0, focus=10.0)
    sc.sph_mat = np.zeros(0, np.int32)
    return sc


SCENES = {"uneven_lamps": uneven_lamps, "all_unlit": all_unlit}


@functools.lru_cache(maxsize=None)
def rays_seeds(name):
    """At most RAYS rays of a scene of SCENES (make_rays' mix) or of lit_scenes.SETS (the first of its own), and
    their seeds."""
    import select_ref as sr
    from test_gpu_ray_query import make_rays
    if name in SCENES:
        rays = make_rays(sr.scene_refs(name)[0], RAYS)
        seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    else:
        rays, seeds = (np.array(a[:RAYS]) for a in ls.rays_seeds(name))
    rays.setflags(write=False)
    seeds.setflags(write=False)
    return rays, seeds
