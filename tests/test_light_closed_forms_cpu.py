"""Light sampling and emissive paths against closed forms, without a GPU: the statement of record of
tests/nee_ref.py (sampling on and off) has the analytic means of tests/light_closed_forms.py, before any GPU
test relies on it.

Per case and option N_CPU = 8,192 paths with rays and RNG states from numpy.random.default_rng (not the
library's path_seeds), and per channel |mean - closed form| <= 5 SE, SE the sample standard deviation over
sqrt(n).  The closed forms' own pieces (Lambert's polygon formula, the sphere's form factor) are checked against
a midpoint-rule integral over the light's area in float64."""
import functools

import numpy as np
import pytest

import light_closed_forms as cf
import nee_ref as nr
from test_gpu_ray_query import Ref


@functools.lru_cache(maxsize=None)
def reference(scene_name, sample):
    sc = {c.scene.name: c.scene for c in cf.cases().values()}[scene_name]
    return nr.NeeRef(sc, Ref(sc), sample=sample)


@pytest.mark.parametrize("option", cf.OPTIONS, ids=["on", "off"])
@pytest.mark.parametrize("name", cf.CASES)
def test_reference_has_the_closed_form_mean(name, option):
    case = cf.cases()[name]
    rays, seeds = case.rays_seeds(cf.N_CPU)
    rad, segs, ends, kinds, events, shadow = reference(case.scene.name, option).paths_events(rays, seeds, case.depth)
    mean, se = cf.statistics(rad)
    print(cf.report(name, option, mean, se, case.want))
    # the scene is closed and every ray meets it; what float32 lets escape to the sky (light_closed_forms'
    # docstring) adds at most 1 per path and channel: less than the standard error
    escaped = int(np.count_nonzero(ends == nr.MISS))
    print(f"{name} {'on ' if option else 'off'}: {escaped} of {len(rad)} paths reach the sky")
    assert np.all(rad[:, 3] == 1.0) and np.all(escaped / len(rad) <= se)
    assert bool(shadow.any()) == option
    assert np.all(np.abs(mean - case.want) <= 5.0 * se), cf.report(name, option, mean, se, case.want)


def test_cases_are_the_listed_ones():
    assert tuple(cf.cases()) == cf.CASES
    for case in cf.cases().values():
        assert case.want.shape == (3,) and np.all(case.want > 0) and case.depth >= 2


def test_the_cases_meet_the_branches_they_are_for():
    """Conditions on the reference alone: the integrating sphere culls the light's far side and ends paths on the
    light after a diffuse vertex; inside the light no connection is culled as a far side and half face away; the
    box connects to all three lights."""
    n = 1024
    c = cf.cases()["sphere_D8"]
    ev = reference(c.scene.name, True).paths_events(*c.rays_seeds(n), c.depth)[4]
    assert np.count_nonzero(ev & nr.FAR_SIDE) > n // 2 and np.count_nonzero(ev & nr.LIGHT_AFTER_DIFFUSE) >= 30
    assert not np.any(ev & (nr.OCCLUDED | nr.BACKFACING | nr.LIGHT_SPECULAR))
    c = cf.cases()["inside_D5"]
    ref = reference(c.scene.name, True)
    assert ref.lights == [0]
    ev = ref.paths_events(*c.rays_seeds(n), c.depth)[4]
    assert not np.any(ev & (nr.FAR_SIDE | nr.LIGHT_SPECULAR)) and np.all(ev & nr.LIGHT_AFTER_DIFFUSE)
    assert n // 3 < np.count_nonzero(ev & nr.BACKFACING) < 2 * n // 3
    assert n // 3 < np.count_nonzero(ev & nr.VISIBLE) < 2 * n // 3
    ref = reference("three_light_box", True)
    assert ref.lights == [12, 13, 14, 15]


@pytest.mark.parametrize("point", list(cf.BOX_POINTS))
def test_no_light_hides_another_in_the_box(point):
    sc = cf.cases()[f"box_{point}"].scene
    assert cf.unoccluded(Ref(sc), point) == 14 + 7 + 9
    p = np.asarray(cf.BOX_POINTS[point][0])
    assert p[0] != p[2] if point.startswith("floor") else p[1] != p[2]  # off the face's diagonal


# ---- the closed forms' own pieces -----------------------------------------------------------------------
def area_integral(p, n, a, b, c, m=600):
    """Midpoint rule over the triangle (a, b, c): the integral of cos_p * |cos_q| / d^2 dA."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    total = 0.0
    ng = np.cross(b - a, c - a)
    area = 0.5 * np.linalg.norm(ng)
    ng = ng / np.linalg.norm(ng)
    # m^2 small triangles: (i, j) lower ones with i + j < m, upper ones with i + j < m - 1
    for (du, dv), keep in ((((1 / 3), (1 / 3)), i + j < m), (((2 / 3), (2 / 3)), i + j < m - 1)):
        u, v = (i[keep] + du) / m, (j[keep] + dv) / m
        q = a + u[:, None] * (b - a) + v[:, None] * (c - a)
        w = q - p
        d2 = (w * w).sum(axis=1)
        total += ((w @ n) * np.abs(w @ ng) / (d2 * d2)).sum() * area / (m * m)
    return total


@pytest.mark.parametrize("point", list(cf.BOX_POINTS))
def test_lamberts_formula_is_the_area_integral(point):
    p, n, _ = (np.asarray(x, np.float64) for x in cf.BOX_POINTS[point])
    q = cf.BOX_QUAD
    quad = area_integral(p, n, q[0], q[1], q[2]) + area_integral(p, n, q[0], q[2], q[3])
    assert abs(quad - cf.polygon_e(p, n, q)) <= 1e-6 * quad
    tri = area_integral(p, n, *cf.BOX_TRI)
    assert abs(tri - cf.polygon_e(p, n, cf.BOX_TRI)) <= 1e-6 * tri


@pytest.mark.parametrize("point", list(cf.BOX_POINTS))
def test_the_spheres_form_factor_is_the_solid_angle_integral(point):
    """pi (r / d)^2 cos(theta) against the midpoint rule over the cap of directions the sphere fills."""
    p, n, _ = (np.asarray(x, np.float64) for x in cf.BOX_POINTS[point])
    c, r = np.asarray(cf.BOX_SPHERE[:3], np.float64), cf.BOX_SPHERE[3]
    w = c - p
    d = np.linalg.norm(w)
    axis = w / d
    a = np.cross(axis, [0.3, 0.5, 0.8])
    a /= np.linalg.norm(a)
    b = np.cross(axis, a)
    m = 400
    cos_max = np.sqrt(1.0 - (r / d) ** 2)
    mu = 1.0 - (np.arange(m) + 0.5) / m * (1.0 - cos_max)  # uniform in cos: equal solid angles
    phi = (np.arange(m) + 0.5) / m * 2.0 * np.pi
    mu, phi = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1.0 - mu * mu)
    om = mu[..., None] * axis + s[..., None] * (np.cos(phi)[..., None] * a + np.sin(phi)[..., None] * b)
    got = (om @ n).mean() * 2.0 * np.pi * (1.0 - cos_max)
    assert abs(got - cf.sphere_e(p, n, cf.BOX_SPHERE)) <= 1e-6 * got


def test_the_integrating_spheres_series():
    """The closed form is the series' partial sum: it grows with the depth towards Le rho F / (1 - rho (1 - F))."""
    rho, le = float(cf.f64(cf.SPHERE_RHO)), cf.f64(cf.SPHERE_LE)
    ff = (cf.SPHERE_r / cf.SPHERE_R) ** 2
    assert abs(ff - 0.04) < 1e-15
    means = [cf.sphere_mean(d) for d in cf.SPHERE_DEPTHS]
    assert np.allclose(means[0], le * rho * ff, rtol=1e-15)
    assert all(np.all(a < b) for a, b in zip(means, means[1:]))
    assert np.all(means[-1] < le * rho * ff / (1.0 - rho * (1.0 - ff)))
    # the depths tell apart: neighbouring depths differ by far more than the GPU test's 1 % power condition
    assert np.all((means[-1] - means[-2]) / means[-1] > 0.05)
