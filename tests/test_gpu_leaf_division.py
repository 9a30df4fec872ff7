"""One division per leaf step (hippt_trace.h leaf_step, DEFER): a lane's triangle candidates of a leaf are
resolved in leaf order, each by the take_hit and the division of the immediate form, so every (t, id),
hit record and image stays bit-identical.

Tiny all-Lambertian scenes of exactly two triangles (one leaf), with rays that pass the edge tests of
BOTH triangles, so that a lane holds a pending candidate when the second one arrives:
  twin             the same triangle twice: equal t, the smaller id wins
  stacked          two parallel overlapping triangles 2^-10 apart, the nearer one second: a later candidate
                   replaces an earlier one
  stacked_swapped  the nearer one first: a later candidate does not replace it
  diagonal         the unit square z = 0 split along (0,0)-(1,1), rays aimed at points (s, s, 0) of the shared
                   edge, s = k/256, from integer origins and straight down
The premise (at least 1,000 of a scene's rays accepted by both triangles with t >= tmin) is asserted on
the oracle alone, before anything runs on the GPU.  References are computed once per scene and shared."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime

import hippt
import pyoracle as po
from hippt import scenes
from hit_ref import HitRef, assert_records
from test_gpu_ray_query import Ref, assert_same, pt, upload  # noqa: F401 (pt: the fixture)

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 36, 4, 4
TRI = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32)
GAP = np.float32(2.0 ** -10)
# integer origins above the unit square (z > 0), off its axes
ORIGINS = [(0, 0, 2), (1, 0, 3), (0, 1, 1), (2, 1, 2), (-1, 2, 3), (3, -1, 1), (-2, -1, 4)]


def _scene(name, verts):
    return scenes.Scene(name, np.asarray(verts, np.float32).reshape(2, 9), np.zeros(2, np.int32),
                        np.array([[0.7, 0.6, 0.5]], np.float32), lookfrom=(0.5, 0.5, 3.0), lookat=(0.5, 0.5, 0.0),
                        vfov=40.0)


def _lifted(z):
    v = TRI.copy()
    v[2::3] = z
    return v


def _rays(origins_targets):
    r = np.zeros((len(origins_targets), 8), np.float32)
    r[:, 3] = 0.001
    r[:, 7] = np.inf
    for i, (o, tgt) in enumerate(origins_targets):
        o = np.asarray(o, np.float32)
        r[i, 0:3] = o
        r[i, 4:7] = np.asarray(tgt, np.float32) - o
    return r


def _interior_rays():
    """Rays at points inside TRI (a 16x16 grid of barycentric points k/64): from each integer origin, and
    straight down from z = 1."""
    pts = [(np.float32(a / 64.0), np.float32(b / 64.0)) for a in range(1, 17) for b in range(1, 17)]
    ot = [(o, (x, y, 0.0)) for o in ORIGINS for x, y in pts]
    ot += [((x, y, 1.0), (x, y, 0.0)) for x, y in pts]
    return _rays(ot)


def _diagonal_rays():
    pts = [np.float32(k / 256.0) for k in range(257)]
    ot = [(o, (s, s, 0.0)) for o in ORIGINS for s in pts]
    ot += [((s, s, 1.0), (s, s, 0.0)) for s in pts]
    return _rays(ot)


SCENES = {
    "twin": (lambda: _scene("twin", [TRI, TRI]), _interior_rays),
    "stacked": (lambda: _scene("stacked", [TRI, _lifted(GAP)]), _interior_rays),
    "stacked_swapped": (lambda: _scene("stacked_swapped", [_lifted(GAP), TRI]), _interior_rays),
    "diagonal": (lambda: _scene("diagonal", [[0, 0, 0, 1, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0, 0, 1, 0]]),
                 _diagonal_rays),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, rays, t, prim, records, rays accepted by both triangles, oracle image and accumulation);
    computed once, never modified."""
    make_scene, make_rays = SCENES[name]
    sc, rays = make_scene(), make_rays()
    ref = Ref(sc)
    t, p = ref.closest(rays)
    rec = HitRef(sc, ref).records(rays, t, p)
    tris = [po.tri_setup(sc.verts[k]) for k in range(2)]
    both = 0
    for r in rays:
        h0 = po.tri_hit(tris[0], r[0:3], r[4:7], 0.001)[0]
        h1 = po.tri_hit(tris[1], r[0:3], r[4:7], 0.001)[0]
        both += h0 and h1
    opx, oacc, segs, _ = po.MeshScene(sc, W, H).frames(0, SPP, DEPTH)
    for a in (rays, t, p, rec, opx, oacc):
        a.setflags(write=False)
    return sc, rays, t, p, rec, both, opx, oacc, segs


@pytest.mark.parametrize("name", list(SCENES))
def test_premise_rays_pass_both_triangles(name):
    """On the oracle alone: at least 1,000 of the ~2,000 rays are accepted by both triangles."""
    _, rays, t, p, _, both, _, _, _ = case(name)
    print(f"{name}: {both} of {len(rays)} rays accepted by both triangles; ids hit {np.unique(p).tolist()}")
    assert 1900 <= len(rays) <= 2100 and both >= 1000
    if name == "twin":
        assert np.all(p[p >= 0] == 0)  # equal t: the smaller id
    if name == "stacked":
        assert np.count_nonzero(p == 1) >= 1000  # the later candidate replaces the earlier one
    if name == "stacked_swapped":
        assert np.count_nonzero(p == 0) >= 1000  # ... and does not


@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_queries_match_oracle(pt, name, width):
    sc, rays, rt, rp, rec, _, _, _, _ = case(name)
    upload(pt, sc, 1, width, W, H)
    t, prim = pt.traceRays(rays)
    assert_same(t, prim, rt, rp, f"{name} width {width}")
    assert_records(pt.traceHits(rays), rec, f"{name} width {width}")


@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("mode", ["megakernel", "wavefront"])
@pytest.mark.parametrize("name", list(SCENES))
def test_render_matches_oracle(pt, name, mode, width):
    sc, _, _, _, _, _, opx, oacc, segs = case(name)
    pt.setOption(hippt.OPT_PATH_MODE, 1 if mode == "wavefront" else 0)
    upload(pt, sc, 1, width, W, H)
    pt.resetStats()
    assert pt.renderFrames(SPP, DEPTH), pt.lastError()
    px, acc = pt.readback()
    assert acc.tobytes() == oacc.tobytes(), f"{np.count_nonzero((acc != oacc).any(axis=2))} pixels' sums differ"
    assert np.array_equal(px, opx)
    assert pt.stats()["segments"] == segs
