"""Closed forms for emissive paths and light sampling (DESIGN.md §2 "Light sampling", §16): three tiny closed
scenes whose mean radiance along a set of query rays is known analytically, in numpy float64, independent of
the oracle and of tests/nee_ref.py.  The estimator, on or off, must have these means: a mistake shared by the
kernel and its float32 restatement (the sphere's area, the light-count factor, the far-side rule, "a light after
a diffuse vertex adds nothing", the depth rule) moves the mean and passes every bit-exact test.

Every scene is closed, so in exact arithmetic no path reaches the sky and the answers hold for any sky.  In
float32 a vertex lies up to an ulp off its surface, and a scattered ray that leaves it almost tangentially (the
scattered direction n + u is short then, and the 0.001 of tmin counts in its length) can meet the same surface
again from the wrong side: about 8 in 100,000 vertices of the integrating sphere do, and such a path leaves the
shell for the sky.  The sky is at most 1 per channel, and the sphere's emission is chosen large against it:
measured on the reference over 2^17 paths at maxDepth 8, 76 paths (sampling off) and 85 (on) escape, and
without sampling what they return is 1.7e-5, 3.3e-5 and 1.2e-4 of the closed form per channel, against standard
errors of 2.4e-3 (off) and 8.8e-4 (on) of it at 2^20 paths.  tests/test_light_closed_forms_cpu.py asserts on the
reference that the escaped paths' largest possible share stays below the standard error.

  sphere_D<k>  integrating sphere: a Lambertian shell (radius R = 10, albedo rho) seen from inside around an
               emissive sphere (radius r = 2, emission Le) at its centre; rays start at radius 5 and point
               radially outward.  A point of the shell sees the light under the form factor F = (r / R)^2
               (a sphere wholly above the horizon, on the normal) and the shell under 1 - F, and every point
               of the shell is like every other, so at maxDepth D >= 2
                   L = Le * rho * F * sum_{j = 0}^{D - 2} (rho * (1 - F))^j
               with light sampling (term j is the connection at the j-th shell vertex; the light met by a
               scattered ray adds nothing) and without (term j is the path that ends on the light with its
               (j + 2)-th segment).
  inside_D<k>  white furnace seen from inside a light: an emissive sphere (radius 10, Le) around a Lambertian
               sphere (radius 1, albedo rho) at its centre; rays start at radius 5 and point at the small
               sphere.  The small sphere is convex and sees Le over its whole hemisphere: L = rho * Le at every
               maxDepth >= 2.  rho and Le are powers of two, so without light sampling every path returns
               rho * Le exactly and the standard error is 0: the test then asks for the exact value.  That
               holds only where the first vertex lies on the sphere exactly, so the rays come along the six
               half-axes: their hit points (+-1, 0, 0), ... are exact in float32, and a ray scattered from one
               cannot meet the small sphere again.  (With rays aimed at random points of the small sphere a
               vertex lies up to an ulp inside it, and 32 of 2^20 paths of the reference leave it almost
               tangentially and meet it again from inside: the mean without light sampling is then
               rho * Le * (1 - 3.0e-5) with a standard error of 5.4e-6 of it.)
  box_<p>      a closed Lambertian box (0, 0, 0)..(10, 10, 10) with three unequal lights: a quad (two
               triangles), one triangle, one sphere.  maxDepth 2 (direct light only): at the point p with
               normal n
                   L = albedo / pi * sum_i Le_i * E_i(p),  E = the integral of cos over the light's solid angle:
               Lambert's formula for a polygon, pi * (r / d)^2 * cos(theta) for a sphere wholly above the horizon.
               The points keep off the diagonals of the box's faces (the oracle's triangle test misses a ray
               aimed exactly at the edge two triangles share), and `unoccluded` asserts that no light hides
               another from a point.

Albedos and emissions enter the closed forms as the float32 values the scene stores."""
import dataclasses
import functools

import numpy as np

from hippt import scenes

F32 = np.float32
OPTIONS = (True, False)  # light sampling on, off
N_CPU = 8192             # paths per case and option on the reference
N_GPU = 1 << 20          # paths per case and option on the device
N_BYTES = 4097           # the first paths of a device run that are compared with the reference's bytes


def f64(x):
    """The float32 value(s) a scene stores for x, as float64."""
    return np.asarray(x, F32).astype(np.float64)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    scene: object
    depth: int
    want: np.ndarray   # (3,) float64: the mean radiance per channel
    origins: object    # rng, n -> (origins (n, 3), directions (n, 3)) float64
    seed: int          # of numpy.random.default_rng: the rays and the paths' RNG states

    def rays_seeds(self, n):
        """(rays (n, 8) float32, seeds (n,) uint32) from default_rng(self.seed); a prefix of a longer draw is not
        the shorter draw, so a test compares runs of the same n only."""
        rng = np.random.default_rng(self.seed)
        o, d = self.origins(rng, n)
        rays = np.zeros((n, 8), F32)
        rays[:, 0:3], rays[:, 4:7] = o, d
        rays[:, 3], rays[:, 7] = 0.001, np.inf
        seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        return np.ascontiguousarray(rays), np.ascontiguousarray(seeds)


def unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


# ---- 1. integrating sphere ------------------------------------------------------------------------------
SPHERE_R, SPHERE_r, SPHERE_RHO, SPHERE_LE = 10.0, 2.0, 0.6, (50.0, 30.0, 10.0)
SPHERE_DEPTHS = (2, 3, 5, 8)


def sphere_scene():
    mats = [(scenes.MAT_LAMBERTIAN, (SPHERE_RHO,) * 3, 0.0, 1.0), (scenes.MAT_EMISSIVE, SPHERE_LE, 0.0, 1.0)]
    return scenes._sphere_scene("integrating_sphere", [(0, 0, 0, SPHERE_R), (0, 0, 0, SPHERE_r)], mats, aperture=0.0)


def sphere_mean(depth):
    rho, le = float(f64(SPHERE_RHO)), f64(SPHERE_LE)
    ff = (SPHERE_r / SPHERE_R) ** 2
    return le * rho * ff * sum((rho * (1.0 - ff)) ** j for j in range(depth - 1))


def sphere_rays(rng, n):
    u = unit(rng, n)
    return 5.0 * u, u


# ---- 2. white furnace from inside a light --------------------------------------------------------------
INSIDE_RHO, INSIDE_LE = 0.5, (8.0, 2.0, 0.5)
INSIDE_DEPTHS = (2, 5)


def inside_scene():
    mats = [(scenes.MAT_EMISSIVE, INSIDE_LE, 0.0, 1.0), (scenes.MAT_LAMBERTIAN, (INSIDE_RHO,) * 3, 0.0, 1.0)]
    return scenes._sphere_scene("inside_a_light", [(0, 0, 0, 10.0), (0, 0, 0, 1.0)], mats, aperture=0.0)


def inside_rays(rng, n):
    """From the six points of the axes at radius 5 towards the centre: see the module's docstring."""
    axes = np.concatenate([np.eye(3), -np.eye(3)])[rng.integers(0, 6, n)]
    return 5.0 * axes, -axes


# ---- 3. closed box, three unequal lights ---------------------------------------------------------------
BOX_ALBEDO = (0.7, 0.5, 0.3)
BOX_QUAD = ((3.0, 8.0, 4.0), (6.0, 8.0, 4.0), (6.0, 8.0, 7.0), (3.0, 8.0, 7.0))
BOX_TRI = ((1.0, 6.0, 1.0), (2.0, 6.5, 1.0), (1.0, 6.0, 2.5))
BOX_SPHERE = (7.5, 5.0, 2.0, 0.8)
BOX_LE = {"quad": (15.0, 15.0, 15.0), "tri": (40.0, 5.0, 1.0), "sphere": (2.0, 6.0, 9.0)}
# name: (p, normal, offset of the rays' origin from p); off the faces' diagonals (floor x = z, wall x = 0: y = z)
BOX_POINTS = {"floor_a": ((4.5, 0.0, 5.5), (0.0, 1.0, 0.0), (0.3, 2.0, -0.2)),
              "floor_b": ((2.0, 0.0, 3.0), (0.0, 1.0, 0.0), (0.3, 2.0, -0.2)),
              "wall": ((0.0, 4.0, 6.0), (1.0, 0.0, 0.0), (2.0, 0.3, -0.2))}


def box_scene():
    tris = scenes._box((0, 0, 0), (10, 10, 10)) + scenes._quad(*BOX_QUAD) + [BOX_TRI[0] + BOX_TRI[1] + BOX_TRI[2]]
    mats = [(scenes.MAT_LAMBERTIAN, BOX_ALBEDO, 0.0, 1.0), (scenes.MAT_EMISSIVE, BOX_LE["quad"], 0.0, 1.0),
            (scenes.MAT_EMISSIVE, BOX_LE["tri"], 0.0, 1.0), (scenes.MAT_EMISSIVE, BOX_LE["sphere"], 0.0, 1.0)]
    sc = scenes._sphere_scene("three_light_box", [BOX_SPHERE], mats, verts=np.asarray(tris, np.float64).astype(F32),
                              tri_mat=[0] * 12 + [1, 1, 2], aperture=0.0)
    sc.sph_mat = np.asarray([3], np.int32)
    return sc


def polygon_e(p, n, poly):
    """Lambert's formula: the integral of cos over the solid angle of a polygon wholly above p's horizon,
    1/2 |sum over its edges of (the angle the edge subtends) * (the unit normal of the edge's plane through p) . n|."""
    v = [np.asarray(q, np.float64) - p for q in poly]
    v = [q / np.linalg.norm(q) for q in v]
    assert all(q @ n > 0 for q in v), "the polygon is not wholly above the horizon"
    total = 0.0
    for i in range(len(v)):
        a, b = v[i], v[(i + 1) % len(v)]
        c = np.cross(a, b)
        total += np.arccos(np.clip(a @ b, -1.0, 1.0)) * (c / np.linalg.norm(c)) @ n
    return abs(total) / 2.0


def sphere_e(p, n, sphere):
    c, r = np.asarray(sphere[:3], np.float64), float(sphere[3])
    w = c - p
    d = np.linalg.norm(w)
    cos = (w / d) @ n
    assert cos * d > r, "the sphere is not wholly above the horizon"  # (its lowest point over the tangent plane)
    return np.pi * (r / d) ** 2 * cos


def box_mean(point):
    p, n, _ = (np.asarray(x, np.float64) for x in BOX_POINTS[point])
    e = f64(BOX_LE["quad"]) * polygon_e(p, n, BOX_QUAD) + f64(BOX_LE["tri"]) * polygon_e(p, n, BOX_TRI) + \
        f64(BOX_LE["sphere"]) * sphere_e(p, n, BOX_SPHERE)
    return f64(BOX_ALBEDO) * e / np.pi


def box_rays(point):
    p, _, off = (np.asarray(x, np.float64) for x in BOX_POINTS[point])

    def make(rng, n):
        return np.tile(p + off, (n, 1)), np.tile(-off, (n, 1))
    return make


def box_light_targets():
    """{light: (primitive ids, points of it to aim at)}: of each triangle its corners, edge midpoints and centroid,
    every one pulled 2 % towards the centroid (off the edges: the oracle's contract at a shared edge); of the
    sphere its centre, `unoccluded` adds its limb as seen from the point."""
    def tri(a, b, c):
        v = np.asarray([a, b, c], np.float64)
        g = v.mean(axis=0, keepdims=True)
        pts = np.concatenate([v, 0.5 * (v + np.roll(v, -1, axis=0)), g])
        return pts + 0.02 * (g - pts)
    q = BOX_QUAD
    return {"quad": ((12, 13), np.concatenate([tri(q[0], q[1], q[2]), tri(q[0], q[2], q[3])])),
            "tri": ((14,), tri(*BOX_TRI)), "sphere": ((15,), np.asarray([BOX_SPHERE[:3]], np.float64))}


def unoccluded(ref, point):
    """Asserts with ref.closest (test_gpu_ray_query.Ref of box_scene()) that the segments from the point towards
    every light's corners, edge midpoints, centre and limb (at 98 % of the radius, so that the ray meets the
    light) end on that light: no light hides another, and no wall hides a light.  Returns the segments checked."""
    p, n, _ = (np.asarray(x, np.float64) for x in BOX_POINTS[point])
    start = p + 1e-3 * n
    checked = 0
    for light, (ids, pts) in box_light_targets().items():
        if light == "sphere":
            c, r = np.asarray(BOX_SPHERE[:3], np.float64), BOX_SPHERE[3]
            w = c - start
            a = np.cross(w, [0.3, 0.5, 0.8])
            a /= np.linalg.norm(a)
            b = np.cross(w, a)
            b /= np.linalg.norm(b)
            ang = np.arange(8) * (np.pi / 4.0)
            pts = np.concatenate([pts, c + 0.98 * r * (np.cos(ang)[:, None] * a + np.sin(ang)[:, None] * b)])
        rays = np.zeros((len(pts), 8), F32)
        rays[:, 0:3], rays[:, 4:7] = start, pts - start
        rays[:, 3], rays[:, 7] = 0.0, np.inf
        _, prim = ref.closest(rays)
        assert np.isin(prim, ids).all(), (point, light, prim.tolist())
        checked += len(pts)
    return checked


# ---- the cases -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}; built once, never modified."""
    out = {}
    sc = sphere_scene()
    for k, depth in enumerate(SPHERE_DEPTHS):
        out[f"sphere_D{depth}"] = Case(f"sphere_D{depth}", sc, depth, sphere_mean(depth), sphere_rays, 100 + k)
    sc = inside_scene()
    for k, depth in enumerate(INSIDE_DEPTHS):
        out[f"inside_D{depth}"] = Case(f"inside_D{depth}", sc, depth, float(f64(INSIDE_RHO)) * f64(INSIDE_LE),
                                       inside_rays, 200 + k)
    sc = box_scene()
    for k, point in enumerate(BOX_POINTS):
        out[f"box_{point}"] = Case(f"box_{point}", sc, 2, box_mean(point), box_rays(point), 300 + k)
    for c in out.values():
        c.want.setflags(write=False)
    return out


CASES = ("sphere_D2", "sphere_D3", "sphere_D5", "sphere_D8", "inside_D2", "inside_D5", "box_floor_a", "box_floor_b",
         "box_wall")


def statistics(rad):
    """(mean (3,), standard error (3,)) of the rgb of radiance (n, 4) float32, accumulated in float64."""
    x = np.asarray(rad)[:, :3].astype(np.float64)
    return x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(len(x))


def report(name, option, mean, se, want):
    """One line per case and option: what the INDEX of profiles/lit_scenes records."""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(se > 0, (mean - want) / se, np.where(mean == want, 0.0, np.inf))
    fmt = lambda a: "(" + ", ".join(f"{v:.6g}" for v in a) + ")"  # noqa: E731
    return f"{name} {'on ' if option else 'off'}: mean {fmt(mean)} closed form {fmt(want)} SE {fmt(se)} " \
           f"SE/closed form {fmt(se / want)} z {fmt(z)}"
