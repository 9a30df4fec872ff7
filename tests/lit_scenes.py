"""Lit scenes beyond the Cornell box for the emissive and light-sampling tests: a deep tree with hundreds of lights
scattered through leaf order, many sphere lights among Metal and Dielectric spheres under a lens camera, and a
hand-made box of edge cases.  Each scene's rays, seeds and references (tests/nee_ref.py, tests/emit_ref.py) are
computed once, shared by the tests and never modified.

  blob64x34_lit     scenes.blob_scene(64, 34) with triangles 10, 26, 42, ... (every 16th of the blob) emissive
                    (6, 4, 2): 272 lights, 8 of them of zero area (the blob's poles), and one emissive sphere
                    (4, 2, 1), so that a connection also meets the far side of a sphere light.
  random_scene_lit  scenes.random_scene() with every 7th small sphere emissive, three emissions in turn; the
                    lens camera (aperture 0.1) and the Metal, Dielectric and Lambertian neighbours stay.
  light_edges       a Lambertian box (0, 0, 0)..(10, 10, 10) around a small one and a Metal sphere, with five lights: a triangle of
                    emission (0, 0, 0), a sphere of emission 1e30, a triangle of zero area, a small triangle coplanar
                    with the floor and 1e-3 above it (connections with a tiny d2), and a plain triangle lamp.
  light_edges_one   the same box with exactly one light, a sphere (the light-count factor is 1)."""
import functools

import numpy as np

import emit_ref as er
import hippt
import nee_ref as nr
import path_ref as pr
import pyoracle as po
from hippt import scenes

F = np.float32
# name: (rays of the path queries, (width, height, frames) of the renders)
SETS = {"blob64x34_lit": (4097, (32, 24, 3)), "random_scene_lit": (257, (16, 12, 2)),
        "light_edges": (1025, (16, 12, 2)), "light_edges_one": (1025, (16, 12, 2))}
BLOB_EMISSION, BLOB_SPHERE, BLOB_SPHERE_EMISSION = (6.0, 4.0, 2.0), (90.0, 400.0, 400.0, 40.0), (4.0, 2.0, 1.0)
RANDOM_EMISSIONS = ((6.0, 4.0, 2.0), (1.0, 3.0, 8.0), (12.0, 12.0, 12.0))


def blob64x34_lit():
    sc = scenes.blob_scene(64, 34)
    k = len(sc.albedo)
    tm = np.array(sc.tri_mat, np.int32)
    tm[np.arange(10, sc.num_tris, 16)] = k
    sc.name = "blob64x34_lit"
    sc.tri_mat = tm
    sc.albedo = np.concatenate([sc.albedo, [BLOB_EMISSION, BLOB_SPHERE_EMISSION]]).astype(F)
    sc.mat_kind = np.array([0] * k + [scenes.MAT_EMISSIVE] * 2, np.int32)
    sc.fuzz, sc.ir = np.zeros(k + 2, F), np.ones(k + 2, F)
    sc.spheres = np.asarray([BLOB_SPHERE], F)
    sc.sph_mat = np.asarray([k + 1], np.int32)
    return sc


def random_scene_lit():
    sc = scenes.random_scene()
    small = np.arange(1, sc.num_spheres - 3)  # (0 is the ground, the last three are the large spheres)
    lit = small[::7]
    kind, albedo = np.array(sc.mat_kind, np.int32), np.array(sc.albedo, F)
    mat = np.asarray(sc.sph_mat, np.int64)[lit]  # (every sphere has a material of its own)
    kind[mat] = scenes.MAT_EMISSIVE
    albedo[mat] = np.asarray(RANDOM_EMISSIONS, F)[np.arange(len(lit)) % len(RANDOM_EMISSIONS)]
    sc.name, sc.mat_kind, sc.albedo = "random_scene_lit", kind, albedo
    return sc


def light_edges(one=False):
    # (the inner box gives Lambertian vertices that face away from a light)
    tris = scenes._box((0, 0, 0), (10, 10, 10)) + scenes._box((1, 0, 1), (3, 2.5, 3))
    tmat = [0] * len(tris)
    mats = [(scenes.MAT_LAMBERTIAN, (0.7, 0.6, 0.5), 0.0, 1.0), (scenes.MAT_METAL, (0.8, 0.8, 0.9), 0.1, 1.0)]
    spheres, smat = [(3.0, 2.0, 6.0, 1.5)], [1]
    if one:
        mats.append((scenes.MAT_EMISSIVE, (9.0, 7.0, 5.0), 0.0, 1.0))
        spheres.append((7.0, 6.0, 4.0, 1.0))
        smat.append(2)
    else:
        lights = [((2.0, 9.0, 2.0) + (4.0, 9.0, 2.0) + (2.0, 9.0, 4.0), (0.0, 0.0, 0.0)),     # emits nothing
                  ((5.0, 5.0, 5.0) + (6.0, 6.0, 6.0) + (7.0, 7.0, 7.0), (3.0, 3.0, 3.0)),     # zero area
                  ((6.0, 0.001, 1.0) + (6.004, 0.001, 1.0) + (6.0, 0.001, 1.004), (5.0, 5.0, 5.0)),  # 1e-3 over the floor
                  ((6.0, 9.5, 6.0) + (9.0, 9.5, 6.0) + (9.0, 9.5, 9.0), (15.0, 12.0, 9.0))]   # a plain lamp
        for verts, le in lights:
            tris.append(verts)
            tmat.append(len(mats))
            mats.append((scenes.MAT_EMISSIVE, le, 0.0, 1.0))
        spheres.append((7.0, 5.0, 7.0, 1.0))
        smat.append(len(mats))
        mats.append((scenes.MAT_EMISSIVE, (1e30, 1e30, 1e30), 0.0, 1.0))
    sc = scenes._sphere_scene("light_edges_one" if one else "light_edges", spheres, mats,
                              verts=np.asarray(tris, np.float64).astype(F), tri_mat=tmat, lookfrom=(1.0, 5.0, 0.5),
                              lookat=(6.0, 4.0, 6.0), vfov=70.0, aperture=0.0, focus=10.0)
    sc.sph_mat = np.asarray(smat, np.int32)
    return sc


BUILDERS = {"blob64x34_lit": blob64x34_lit, "random_scene_lit": random_scene_lit, "light_edges": light_edges,
            "light_edges_one": lambda: light_edges(one=True)}


@functools.lru_cache(maxsize=None)
def scene_refs(name):
    """(scene, NeeRef with sampling, EmitRef) of a scene of SETS."""
    from test_gpu_ray_query import Ref
    sc = BUILDERS[name]()
    ref = Ref(sc)
    return sc, nr.NeeRef(sc, ref), er.EmitRef(sc, ref)


def random_lit_rays(sc, n):
    """make_rays' mix for a quarter of the rays (its degenerate rays among them).  A light is one of 69 small
    spheres on the ground among 400 others, so few of those rays' connections reach their light; the other
    quarters are aimed where more happens: at the flank of the large Lambertian sphere, which looks over the small
    ones; from above at the ground right beside a light, from where a scattered ray also meets that light; and at
    the lights themselves."""
    from test_gpu_ray_query import make_rays
    rng = np.random.default_rng(23)
    sp = np.asarray(sc.spheres, np.float64).reshape(-1, 4)
    kind = sc.materials()["kind"][np.asarray(sc.sph_mat, np.int64)]
    quarter = n // 4
    rays = np.zeros((n, 8), np.float64)
    rays[:, 3], rays[:, 7] = 0.001, np.inf
    a = n - 3 * quarter
    rays[:a] = make_rays(sc, a)
    big = sp[-2]  # (-4, 1, 0), radius 1, Lambertian
    assert kind[-2] == scenes.MAT_LAMBERTIAN and big[3] == 1.0
    phi, y = rng.uniform(0.0, 2.0 * np.pi, quarter), rng.uniform(0.0, 0.8, quarter)
    out = np.stack([np.sqrt(1.0 - y * y) * np.cos(phi), y, np.sqrt(1.0 - y * y) * np.sin(phi)], axis=1)
    rays[a:a + quarter, 0:3] = big[:3] + 3.0 * out
    rays[a:a + quarter, 4:7] = -out
    a += quarter
    lights = sp[kind == scenes.MAT_EMISSIVE][rng.integers(0, np.count_nonzero(kind == scenes.MAT_EMISSIVE), quarter)]
    phi = rng.uniform(0.0, 2.0 * np.pi, quarter)
    beside = lights[:, :3] + 0.3 * np.stack([np.cos(phi), np.zeros(quarter), np.sin(phi)], axis=1)
    beside[:, 1] = 0.0
    rays[a:a + quarter, 0:3] = beside + [0.2, 3.0, -0.1]
    rays[a:a + quarter, 4:7] = [-0.2, -3.0, 0.1]
    a += quarter
    org = lights[:, :3] + rng.normal(size=(quarter, 3)) * [2.0, 0.0, 2.0] + [0.0, rng.uniform(1.0, 4.0), 0.0]
    rays[a:, 0:3] = org
    rays[a:, 4:7] = lights[:, :3] + rng.uniform(-0.1, 0.1, size=(quarter, 3)) - org
    return np.ascontiguousarray(rays, F)


def edge_rays(sc, n):
    """make_rays' mix, and in place of 128 of its rays (before the degenerate ones) rays that start in the gap
    between the floor and the triangle 1e-3 above it and go down, with tmin 0: their first vertex lies under the
    light, no other ray reaches it there, and its connection to that light has a d2 of 1e-6 to 4e-5."""
    from test_gpu_ray_query import degenerate_rays, make_rays
    rng = np.random.default_rng(29)
    rays = np.array(make_rays(sc, n))
    m, end = 128, n - len(degenerate_rays())
    a, b = rng.random(m), rng.random(m)
    a, b = np.where(a + b > 1, 1 - a, a), np.where(a + b > 1, 1 - b, b)
    rays[end - m:end, 0] = 6.0 + 0.004 * a
    rays[end - m:end, 1] = 0.0005
    rays[end - m:end, 2] = 1.0 + 0.004 * b
    rays[end - m:end, 3] = 0.0
    rays[end - m:end, 4:7] = np.stack([rng.normal(size=m), -rng.uniform(0.2, 2.0, m), rng.normal(size=m)], axis=1)
    return np.ascontiguousarray(rays, F)


@functools.lru_cache(maxsize=None)
def rays_seeds(name):
    from test_gpu_ray_query import make_rays
    sc = scene_refs(name)[0]
    make = {"random_scene_lit": random_lit_rays, "light_edges": edge_rays}.get(name, make_rays)
    rays = make(sc, SETS[name][0])
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    rays.setflags(write=False)
    seeds.setflags(write=False)
    return rays, seeds


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nee_case(name, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds, events, shadow rays) with light sampling."""
    sc, ref, _ = scene_refs(name)
    rays, seeds = rays_seeds(name)
    return (sc, rays, seeds) + _frozen(ref.paths_events(rays, seeds, max_depth))


@functools.lru_cache(maxsize=None)
def emit_case(name, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds) without light sampling: EmitRef's paths."""
    sc, _, ref = scene_refs(name)
    rays, seeds = rays_seeds(name)
    return (sc, rays, seeds) + _frozen(ref.paths(rays, seeds, max_depth))


def render_nee(ref, sc, w, h, frames, max_depth=pr.MAX_DEPTH):
    """nee_ref.render_case's loop over any NeeRef: (accumulation (h, w, 4), pixel words (h, w), segments, shadow
    rays among them)."""
    L = po.lib()
    acc = np.zeros((h * w, 4), F)
    px = np.zeros(h * w, np.uint32)
    total = shadow = 0
    for f in range(frames):
        rays, seeds = pr.camera_rays_seeds(sc, w, h, f)
        rad, nseg, _, _, _, nshadow = ref.paths_events(rays, seeds, max_depth)
        total += int(nseg.sum())
        shadow += int(nshadow.sum())
        rgb = np.ascontiguousarray(rad[:, :3])
        for i in range(h * w):
            px[i] = L.po_accumulate(acc[i].ctypes.data_as(er.PF), rgb[i].ctypes.data_as(er.PF), f)
    return acc.reshape(h, w, 4), px.reshape(h, w), total, shadow


@functools.lru_cache(maxsize=None)
def nee_render(name):
    """(scene, accumulation, pixel words, segments, shadow rays) of SETS[name]'s render with light sampling."""
    sc, ref, _ = scene_refs(name)
    return (sc,) + _frozen(render_nee(ref, sc, *SETS[name][1]))


@functools.lru_cache(maxsize=None)
def emit_render(name):
    """(scene, accumulation, pixel words, segments) of SETS[name]'s render without light sampling."""
    sc, _, ref = scene_refs(name)
    return (sc,) + _frozen(er.render_with(ref, sc, *SETS[name][1])[:3])
