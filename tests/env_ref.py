"""The reference of the environment map (include/hippt.h hipptSetEnvironment): the statement of
record of env(d), and the other references under it.

The environment is a square octahedral image E[y][x] of S x S rgb texels, +y up, the upper hemisphere the inner
diamond.  The centre of texel (x, y) is u = (2x + 1)/S - 1, w = (2y + 1)/S - 1; its direction has
dy = 1 - |u| - |w| and (dx, dz) = (u, w) if dy >= 0, else ((1 - |w|) sg(u), (1 - |u|) sg(w)), normalised.

env(d), each line one IEEE float32 operation in the association written (lookup below):
    s  = (|dx| + |dy|) + |dz|
    u  = dx / s;   w = dz / s
    if dy < 0:  (u, w) = ((1 - |w|) * sg(u), (1 - |u|) * sg(w))     sg(x) = x < 0 ? -1 : 1, both from the old u, w
    h  = 0.5f * float(S)
    fx = fminf(fmaxf(fmaf(u, h, h) - 0.5f, 0.0f), float(S - 1))     fy the same from w (minNum/maxNum: NaN gives 0)
    x0 = int(fx); x1 = min(x0 + 1, S - 1); a = fx - float(x0)       y0, y1, b the same from fy
    per channel: top = fmaf(a, E[y0][x1] - E[y0][x0], E[y0][x0]);  bot the same on row y1;  e = fmaf(b, bot - top, top)

Where it applies: wherever a path rule says "miss: thr x sky", thr.c * e.c stands in its place (plain paths:
L.c = thr.c * e.c; light sampling: L.c = Lacc.c + thr.c * e.c), e = env(d) of the direction of the segment that
missed, exactly as the path holds it.  Nothing else changes.  path_ref.PathRef, emit_ref.EmitRef, nee_ref.NeeRef,
mis_ref.MisRef, the select_ref references and emit_ref.render_with all call path_ref.sky by that name, so under
`swap(E)` they are the references of this rule without an edit.  Their lru_cached *_case helpers must not be
called under it (they would cache an environment's results as the gradient's): the cases of this file cache per
(scene, environment).

tests/test_env_ref_cpu.py pins the library's hipptEnvLookup (the kernels' own text) to lookup() before any GPU
test relies on it."""
import contextlib
import functools

import numpy as np

import hippt
import path_ref as pr
from hit_ref import fmaf

F = np.float32


def sg(x):
    return F(-1.0) if x < 0 else F(1.0)


def coords(d):
    """The octahedral coordinates (u, w) of direction d (three float32), in float32."""
    dx, dy, dz = F(d[0]), F(d[1]), F(d[2])
    with np.errstate(all="ignore"):
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        u, w = dx / s, dz / s
        if dy < 0:
            u, w = (F(1.0) - np.abs(w)) * sg(u), (F(1.0) - np.abs(u)) * sg(w)
    return F(u), F(w)


def texel_coord(u, size):
    """(fx, whether the clamp changed it) of octahedral coordinate u."""
    h = F(0.5) * F(size)
    with np.errstate(all="ignore"):
        raw = fmaf(u, h, h) - F(0.5)
    fx = np.fmin(np.fmax(raw, F(0.0)), F(size - 1))  # (fmax/fmin: a NaN gives the other operand)
    return F(fx), not (raw == fx)


def lookup(E, d, detail=None):
    """env(d) of the map E (S, S, 3) float32: three float32.  detail (a dict): "low" whether the dy < 0 branch ran,
    "clamped" whether a coordinate was clamped, "texels" the (y, x) of the four taps."""
    size = E.shape[0]
    u, w = coords(d)
    fx, cx = texel_coord(u, size)
    fy, cy = texel_coord(w, size)
    x0, y0 = int(fx), int(fy)
    x1, y1 = min(x0 + 1, size - 1), min(y0 + 1, size - 1)
    a, b = fx - F(x0), fy - F(y0)
    out = []
    for c in range(3):
        top = fmaf(a, E[y0, x1, c] - E[y0, x0, c], E[y0, x0, c])
        bot = fmaf(a, E[y1, x1, c] - E[y1, x0, c], E[y1, x0, c])
        out.append(fmaf(b, bot - top, top))
    if detail is not None:
        detail["low"] = bool(F(d[1]) < 0)
        detail["clamped"] = cx or cy
        detail["texels"] = {(y0, x0), (y0, x1), (y1, x0), (y1, x1)}
    return tuple(out)


def lookups(E, dirs):
    """lookup over directions (n, 3): (n, 3) float32."""
    E = np.ascontiguousarray(E, F)
    return np.array([lookup(E, d) for d in np.asarray(dirs, F).reshape(-1, 3)], F).reshape(-1, 3)


def texel_directions(size):
    """The texel-centre directions (S, S, 3) float64 of the rule's first paragraph."""
    c = (2.0 * np.arange(size, dtype=np.float64) + 1.0) / size - 1.0
    u, w = np.meshgrid(c, c)
    dy = 1.0 - np.abs(u) - np.abs(w)
    low = dy < 0
    dx = np.where(low, (1.0 - np.abs(w)) * np.where(u < 0, -1.0, 1.0), u)
    dz = np.where(low, (1.0 - np.abs(u)) * np.where(w < 0, -1.0, 1.0), w)
    d = np.stack([dx, dy, dz], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def random_env(size, seed):
    """A seeded map (S, S, 3) float32 over several decades: 10^U(-3, 2) per channel, a few texels exactly 0."""
    rng = np.random.default_rng(1000 * size + seed)
    e = (10.0 ** rng.uniform(-3.0, 2.0, size=(size, size, 3))).astype(F)
    e[rng.uniform(size=(size, size)) < 0.05] = 0.0
    return np.ascontiguousarray(e)


@contextlib.contextmanager
def swap(E, log=None):
    """While open, path_ref.sky is thr x env(d) of the map E: every reference that calls it is the reference
    under that environment.  log (a list): one dict of lookup's details, plus "d", per miss."""
    E = np.ascontiguousarray(E, F)
    assert E.ndim == 3 and E.shape[0] == E.shape[1] and E.shape[2] == 3

    def sky(d, thr):
        det = {} if log is not None else None
        e = lookup(E, d, det)
        if log is not None:
            det["d"] = tuple(d)
            log.append(det)
        return tuple(F(thr[k]) * e[k] for k in range(3))

    old = pr.sky
    pr.sky = sky
    try:
        yield
    finally:
        pr.sky = old


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def env_of(size, seed=0):
    return _frozen([random_env(size, seed)])[0]


@functools.lru_cache(maxsize=None)
def _path_ref_of(name):
    from test_gpu_ray_query import Ref, case
    sc = case(name)[0]
    return sc, pr.PathRef(sc, Ref(sc))


# ---- plain paths: traced once per ray set, replayed per environment -------------------------------------------
# A plain path (PathRef, EmitRef) calls path_ref.sky at most once, at its end, and returns that call's result as
# its rgb.  The environment changes nothing before that call, so a ray set is traced once, under a sky that
# records each call's (d, thr), and the radiance under any map E is those calls made again: thr.c * env(d).c,
# the very expression swap() computes.  tests/test_env_ref_cpu.py pins replay() to a direct run under swap().
def record(ref, rays, seeds, max_depth=pr.MAX_DEPTH):
    """A plain reference's paths with their sky calls kept: dict of "rad" (n, 4) with rgb 0 where the path missed,
    "segs", "ends", "missed" (n,) bool, "d" and "thr" (n, 3) float32 of the miss's call."""
    n = len(rays)
    rec = {"rad": np.zeros((n, 4), F), "segs": np.zeros(n, np.int32), "ends": np.zeros(n, np.int32),
           "missed": np.zeros(n, bool), "d": np.zeros((n, 3), F), "thr": np.zeros((n, 3), F)}
    calls = []

    def sky(d, thr):
        calls.append((tuple(d), tuple(thr)))
        return (F(0.0), F(0.0), F(0.0))

    old = pr.sky
    pr.sky = sky
    try:
        for i in range(n):
            calls.clear()
            rec["rad"][i], rec["segs"][i], rec["ends"][i] = ref.path(rays[i], seeds[i], max_depth)[:3]
            assert len(calls) == (1 if rec["ends"][i] == pr.MISS else 0)
            if calls:
                rec["missed"][i], rec["d"][i], rec["thr"][i] = True, calls[0][0], calls[0][1]
    finally:
        pr.sky = old
    return {k: _frozen([v])[0] for k, v in rec.items()}


def replay(rec, E):
    """(radiance (n, 4), segments) of a record()ed ray set under the map E (None: the sky gradient)."""
    E = None if E is None else np.ascontiguousarray(E, F)
    rad = np.array(rec["rad"])
    for i in np.flatnonzero(rec["missed"]):
        d, thr = tuple(rec["d"][i]), tuple(rec["thr"][i])
        if E is None:
            rad[i, 0:3] = pr.sky(d, thr)
        else:
            e = lookup(E, d)
            rad[i, 0:3] = tuple(F(thr[k]) * e[k] for k in range(3))
    return rad, rec["segs"]


@functools.lru_cache(maxsize=None)
def path_case(name, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, record) of test_gpu_ray_query.case(name)'s rays with path_seeds(n, 0); computed once,
    never modified."""
    from test_gpu_ray_query import case
    sc, ref = _path_ref_of(name)
    rays = case(name)[1]
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    seeds.setflags(write=False)
    return sc, rays, seeds, record(ref, rays, seeds, max_depth)


@functools.lru_cache(maxsize=None)
def camera_case(name, w=32, h=24, frames=3, max_depth=pr.MAX_DEPTH):
    """(scene, [record of frame f's camera samples]) of a scene of test_gpu_ray_query.case; computed once."""
    sc, ref = _path_ref_of(name)
    recs = []
    for f in range(frames):
        rays, seeds = pr.camera_rays_seeds(sc, w, h, f)
        recs.append(record(ref, rays, seeds, max_depth))
    return sc, recs


def render_replay(recs, envs, w, h):
    """The image of frames 0 .. len(recs) - 1, frame f under the map envs[f] (None: the gradient), accumulated
    by the oracle's po_accumulate as emit_ref.render_with does: (accumulation (h, w, 4), pixel words (h, w),
    segments)."""
    import emit_ref as er
    import pyoracle as po
    L = po.lib()
    acc = np.zeros((h * w, 4), F)
    px = np.zeros(h * w, np.uint32)
    total = 0
    for f, rec in enumerate(recs):
        rad, segs = replay(rec, envs[f])
        total += int(segs.sum())
        rgb = np.ascontiguousarray(rad[:, :3])
        for i in range(h * w):
            px[i] = L.po_accumulate(acc[i].ctypes.data_as(er.PF), rgb[i].ctypes.data_as(er.PF), f)
    return acc.reshape(h, w, 4), px.reshape(h, w), total


def paths_under(ref, E, rays, seeds, max_depth=pr.MAX_DEPTH):
    """(radiance, segments) of any reference's paths under the map E."""
    with swap(E):
        out = ref.paths(rays, seeds, max_depth)
    return out[0], out[1]


def render_under(ref, E, sc, w, h, frames, max_depth=pr.MAX_DEPTH):
    """emit_ref.render_with under the map E: (accumulation (h, w, 4), pixel words (h, w), segments)."""
    import emit_ref as er
    with swap(E):
        acc, px, total, _, _ = er.render_with(ref, sc, w, h, frames, max_depth)
    return acc, px, total
