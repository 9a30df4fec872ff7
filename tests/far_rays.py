"""Ray families the queries' validity promise (include/hippt.h) covers and test_gpu_ray_query.make_rays
does not: origins far outside the scene, directions of extreme length, directions with zero and
near-zero components, and far rays that pass the scene by.  Shared by tests/test_far_rays_cpu.py (the
conditions on the reference alone, and the host model of the box test) and tests/test_gpu_far_rays.py.

Every family has a fixed seed; the reference is test_gpu_ray_query.Ref.closest (the oracle's
po_closest_hit / po_sphere_t), computed once per scene and never modified.  M is the largest
|coordinate| of the scene and its camera, the quantity the builder's pad M * 2^-16 is made from; a far
origin lies K * M from the point it aims at.

Families (256 rays per cell; a cell's first three quarters aim at interior points of random primitives,
its last quarter at mesh vertices, where leaves share edges):
  far     o = p - u K M, d = u s; K in FAR_K, s in FAR_S; tmin 0.001, tmax inf
  scale   the same with K in SCALE_K, s in SCALE_S; tmin 0 (with a long d every t is below 0.001)
  axis    in-box and K = 512 origins; one or two components of d exactly +0.0 / -0.0, or one component
          at 1e-20, 1e-25, 9.9e-21 beside components of order 1; lengths 1e-3, 1, 1e3
  miss    64 rays per far cell whose line stays three scene radii from the scene's centre
  bounds  the oracle hits of the far cells of K = 4096 with tmax = t (a miss: tmax is exclusive),
          tmax = nextafter(t) (that hit), tmin = t (that hit), tmin = nextafter(t) (the next surface)
"""
import dataclasses
import functools

import numpy as np

from hippt import scenes
from refit_util import pad_of, sphere_boxes, tri_boxes

F = np.float32
INF = F(np.inf)
CELL = 256
FAR_K = (8, 64, 512, 4096, 2 ** 16, 2 ** 20)
FAR_S = (2.0 ** -20, 1.0, 2.0 ** 20)
SCALE_K = (1, 8)
SCALE_S = (2.0 ** -100, 2.0 ** -70, 2.0 ** -64, 2.0 ** -60, 2.0 ** 60, 2.0 ** 64, 2.0 ** 80)
AXIS_K = (0, 512)  # 0: an origin inside the scene's box
AXIS_KINDS = ("zero1", "zero2", "tiny")
AXIS_LEN = (1e-3, 1.0, 1e3)
TINY = (1e-20, 1e-25, 9.9e-21)
BOUNDS_K = 4096
BOUNDS = ("tmax=t", "tmax=next", "tmin=t", "tmin=next")
SCENES = {
    "cornell34": scenes.cornell34,
    "cornell_mixed": scenes.cornell_mixed,
    "blob64x34": lambda: scenes.blob_scene(64, 34),
}
SEEDS = {"far": 101, "scale": 202, "axis": 303, "miss": 404}


@dataclasses.dataclass(frozen=True)
class Cell:
    family: str
    K: float       # the origin's distance in units of M (0: inside the box)
    s: float       # the direction's length (axis: 0, lengths are mixed; bounds: the far cell's)
    kind: str      # axis: AXIS_KINDS; bounds: BOUNDS; else ""
    start: int
    stop: int

    @property
    def sl(self):
        return slice(self.start, self.stop)

    @property
    def label(self):
        return f"{self.family}{'/' + self.kind if self.kind else ''} K={self.K:g} s=2^{np.log2(self.s):g}" if self.s \
            else f"{self.family}/{self.kind} K={self.K:g}"


def scene_M(sc):
    """The largest |coordinate| of the primitives' boxes and the camera: pad * 2^16 (bvh_builder.cpp)."""
    boxes = np.concatenate([tri_boxes(np.ascontiguousarray(sc.verts, F).reshape(-1, 9)), sphere_boxes(sc.spheres)])
    return float(pad_of(boxes, max(abs(float(v)) for v in sc.lookfrom)) * F(65536.0))


def _box(sc):
    pts = [np.asarray(sc.verts, np.float64).reshape(-1, 3)]
    sp = np.asarray(sc.spheres, np.float64).reshape(-1, 4)
    if sp.shape[0]:
        pts += [sp[:, :3] - sp[:, 3:4], sp[:, :3] + sp[:, 3:4]]
    p = np.concatenate(pts)
    return p.min(axis=0), p.max(axis=0)


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _targets(sc, rng, n):
    """n points to aim at: the first n - n // 4 interior points of random primitives (surface points of
    spheres), the rest mesh vertices."""
    verts = np.asarray(sc.verts, np.float64).reshape(-1, 3)
    tris = verts.reshape(-1, 3, 3)
    sp = np.asarray(sc.spheres, np.float64).reshape(-1, 4)
    nt, ns = tris.shape[0], sp.shape[0]
    out = np.zeros((n, 3))
    prim = rng.integers(0, nt + ns, size=n)
    bary = rng.dirichlet((1.0, 1.0, 1.0), size=n)
    on = _unit(rng, n)
    corner = rng.integers(0, max(verts.shape[0], 1), size=n)
    for i in range(n):
        if i >= n - n // 4 and nt:
            out[i] = verts[corner[i]]
        elif prim[i] < nt:
            out[i] = (tris[prim[i]] * bary[i][:, None]).sum(axis=0)
        else:
            c = sp[prim[i] - nt]
            out[i] = c[:3] + abs(c[3]) * on[i]
    return out


def _rays(o, d, tmin, tmax=np.inf):
    r = np.zeros((len(o), 8), np.float64)
    r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7] = o, d, tmin, tmax
    with np.errstate(over="raise"):
        return r.astype(F)


def _aimed(sc, rng, M, K, s, tmin):
    p = _targets(sc, rng, CELL)
    u = _unit(rng, CELL)
    return _rays(p - u * (K * M), u * s, tmin)


def _axis(sc, rng, M, K, kind):
    lo, hi = _box(sc)
    p = _targets(sc, rng, CELL)
    d = rng.normal(size=(CELL, 3))
    ax = rng.integers(0, 3, size=CELL)
    zero = np.where(rng.integers(0, 2, size=(CELL, 3)) == 0, 0.0, -0.0)
    tiny = rng.choice(TINY, size=CELL) * rng.choice((-1.0, 1.0), size=CELL)
    length = rng.choice(AXIS_LEN, size=CELL)
    for i in range(CELL):
        a = ax[i]
        if kind == "zero1":
            d[i, a] = zero[i, a]
        elif kind == "zero2":
            d[i, (a + 1) % 3], d[i, (a + 2) % 3] = zero[i, (a + 1) % 3], zero[i, (a + 2) % 3]
        else:
            d[i, a] = tiny[i]
    live = np.abs(d) > 1e-3 * np.abs(d).max(axis=1, keepdims=True)
    u = np.where(live, d, 0.0)
    u /= np.linalg.norm(u, axis=1, keepdims=True)  # the line through p the ray follows (up to the tiny term)
    if K:
        back = np.full(CELL, K * M)
    else:  # back along -u from p, staying inside the box
        with np.errstate(divide="ignore", invalid="ignore"):
            room = np.where(u > 0, (p - lo) / u, np.where(u < 0, (p - hi) / u, np.inf))
        back = np.clip(room.min(axis=1), 0.0, None) * rng.uniform(0.1, 0.9, size=CELL)
    scale = length / np.linalg.norm(d, axis=1)
    dd = d * scale[:, None]
    if kind == "tiny":  # the tiny component keeps its value whatever the length
        dd[np.arange(CELL), ax] = tiny
    return _rays(p - u * back[:, None], dd, 0.001)


def _miss(sc, rng, M, K, s):
    lo, hi = _box(sc)
    centre, radius = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    n = CELL // 4
    u = _unit(rng, n)
    w = np.cross(u, _unit(rng, n))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    # at K M the origin's float32 rounding moves the line by at most 2^-24 K M sqrt(3) < 0.11 M for K = 2^20
    p = centre + w * (3.0 * radius + 0.25 * M)
    return _rays(p - u * (K * M), u * s, 0.001)


@dataclasses.dataclass(frozen=True)
class Case:
    sc: object
    M: float
    rays: np.ndarray   # (n, 8) float32
    t: np.ndarray      # reference t (n,)
    prim: np.ndarray   # reference primitive (n,)
    cells: tuple
    ref: object        # the scene's test_gpu_ray_query.Ref
    noise: np.ndarray  # (n,) bool: the reference hit is a triangle without area (see zero_area_triangles)

    def of(self, family, **kw):
        return [c for c in self.cells if c.family == family and all(getattr(c, k) == v for k, v in kw.items())]


@functools.lru_cache(maxsize=None)
def far_case(name):
    """The families over a named scene with their reference; computed once, never modified."""
    from test_gpu_ray_query import Ref
    sc = SCENES[name]()
    M = scene_M(sc)
    ref = Ref(sc)
    parts, cells = [], []

    def add(family, K, s, kind, rays):
        at = sum(len(p) for p in parts)
        parts.append(rays)
        cells.append(Cell(family, float(K), float(s), kind, at, at + len(rays)))

    rng = np.random.default_rng(SEEDS["far"])
    for K in FAR_K:
        for s in FAR_S:
            add("far", K, s, "", _aimed(sc, rng, M, K, s, 0.001))
    rng = np.random.default_rng(SEEDS["scale"])
    for K in SCALE_K:
        for s in SCALE_S:
            add("scale", K, s, "", _aimed(sc, rng, M, K, s, 0.0))
    rng = np.random.default_rng(SEEDS["axis"])
    for K in AXIS_K:
        for kind in AXIS_KINDS:
            add("axis", K, 0.0, kind, _axis(sc, rng, M, K, kind))
    rng = np.random.default_rng(SEEDS["miss"])
    for K in FAR_K:
        for s in FAR_S:
            add("miss", K, s, "", _miss(sc, rng, M, K, s))
    base = np.concatenate(parts)
    bt, bp = ref.closest(base)
    # far with bounds: the oracle hits of the K = 4096 far cells
    for c in [c for c in cells if c.family == "far" and c.K == BOUNDS_K]:
        hit = c.start + np.flatnonzero(bp[c.sl] >= 0)
        for kind in BOUNDS:
            r = base[hit].copy()
            col = 7 if kind.startswith("tmax") else 3
            r[:, col] = bt[hit] if kind.endswith("=t") else np.nextafter(bt[hit], INF)
            add("bounds", c.K, c.s, kind, r)
    rays = np.ascontiguousarray(np.concatenate(parts))
    nb = len(base)
    t, prim = np.concatenate([bt, np.zeros(len(rays) - nb, F)]), np.concatenate([bp, np.zeros(len(rays) - nb, np.int32)])
    t[nb:], prim[nb:] = ref.closest(rays[nb:])
    noise = np.isin(prim, zero_area_triangles(sc))
    for a in (rays, t, prim, noise):
        a.setflags(write=False)
    return Case(sc, M, rays, t, prim, tuple(cells), ref, noise)


def bounds_base(case, cell):
    """(t, prim) the unbounded far rays of a bounds cell have: its rays are the far cell's oracle hits."""
    far = case.of("far", K=cell.K, s=cell.s)[0]
    hit = far.start + np.flatnonzero(case.prim[far.sl] >= 0)
    return case.t[hit], case.prim[hit]


def zero_area_triangles(sc):
    """Ids of the triangles whose corners lie on one line (exactly: float64 products of float32
    differences): the blob's pole triangles repeat a corner.  The contract lets them never hit
    (DESIGN.md §2), but po_tri_setup's float32 cross product can leave a rounding residue for a normal,
    and po_tri_hit then divides noise by noise: the t it accepts (ray 9448 of blob64x34: 122.39 where the
    ray reaches the scene at 409.3) is no point of the ray, and no box around the triangle can hold it.
    Such reference hits are not compared (Case.noise); tests/test_far_rays_cpu.py bounds their number."""
    v = np.asarray(sc.verts, np.float32).reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return np.flatnonzero((n == 0).all(axis=1))


def wall_triangles(sc):
    """Ids of the flat walls: triangles with no extent on one axis (their leaf box is the pad alone there)
    that span at least half the scene on the other two."""
    b = tri_boxes(np.ascontiguousarray(sc.verts, F).reshape(-1, 9))
    size = b[:, 3:] - b[:, :3]
    half = 0.5 * (b[:, 3:].max(axis=0) - b[:, :3].min(axis=0))
    return np.flatnonzero(((size == 0).sum(axis=1) == 1) & ((size >= half).sum(axis=1) == 2))


@functools.lru_cache(maxsize=None)
def hit_records(name):
    """The reference hit records (hit_ref.HitRef) of far_case(name)."""
    from hit_ref import HitRef
    c = far_case(name)
    rec = HitRef(c.sc, c.ref).records(c.rays, c.t, c.prim)
    rec.setflags(write=False)
    return rec


def path_cells(case):
    """The cells traceRadiance is checked on: far K in {512, 2^16} at s = 1, and the scale cells."""
    return [c for c in case.cells if (c.family == "far" and c.K in (512, 2 ** 16) and c.s == 1.0) or c.family == "scale"]


CAMERA_K = (8, 16, 20, 32, 48, 64, 96, 128, 256, 512)


@functools.lru_cache(maxsize=None)
def camera_distance_case(name="cornell34", n=2048, seed=505):
    """Rays as a camera moved straight back to K M from the scene sends them (hipptSetCamera with a long
    lens): from (lookfrom.x, lookfrom.y, -K M) at random points of the scene's box, unit length, the
    renderer's tmin; one cell per K of CAMERA_K.  For the host model only: the distance up to which the
    builder's pad covers the render kernels' camera rays."""
    from test_gpu_ray_query import Ref
    sc = SCENES[name]()
    M = scene_M(sc)
    lo, hi = _box(sc)
    rng = np.random.default_rng(seed)
    parts, cells = [], []
    for K in CAMERA_K:
        o = np.array([sc.lookfrom[0], sc.lookfrom[1], -K * M])
        d = rng.uniform(lo, hi, size=(n, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        cells.append(Cell("camera", float(K), 1.0, "", len(parts) * n, (len(parts) + 1) * n))
        parts.append(_rays(np.broadcast_to(o, (n, 3)), d, 0.001))
    rays = np.ascontiguousarray(np.concatenate(parts))
    ref = Ref(sc)
    t, prim = ref.closest(rays)
    return Case(sc, M, rays, t, prim, tuple(cells), ref, np.zeros(len(rays), bool))


def write_model_file(case, path):
    """The families for tests/native/far_model.cpp: int32 ray count, cell count; per cell
    int32 start, stop, float64 K, s, 32 bytes of label; the rays."""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", len(case.rays), len(case.cells)))
        for c in case.cells:
            f.write(struct.pack("<2i2d32s", c.start, c.stop, c.K, c.s,
                                f"{c.family}{'/' + c.kind if c.kind else ''}".encode()))
        f.write(case.rays.tobytes())
