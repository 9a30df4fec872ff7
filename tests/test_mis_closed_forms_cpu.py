"""Light sampling with MIS against closed forms, without a GPU: the statement of record of tests/mis_ref.py has
the analytic means of tests/light_closed_forms.py, before any GPU test relies on it.

Per case N_CPU = 8,192 paths with rays and RNG states from numpy.random.default_rng, and per channel
|mean - closed form| <= 5 SE, SE the sample standard deviation over sqrt(n).  With the weights both techniques
contribute: the connection's term and the light met by the scattered ray add up to the closed form's term, so a
weight that is wrong in either place (or a hit weighted where it must count whole) moves the mean."""
import functools

import numpy as np
import pytest

import light_closed_forms as cf
import mis_ref as mr
from test_gpu_ray_query import Ref


@functools.lru_cache(maxsize=None)
def reference(scene_name):
    sc = {c.scene.name: c.scene for c in cf.cases().values()}[scene_name]
    return mr.MisRef(sc, Ref(sc))


@pytest.mark.parametrize("name", cf.CASES)
def test_reference_has_the_closed_form_mean(name):
    case = cf.cases()[name]
    rays, seeds = case.rays_seeds(cf.N_CPU)
    rad, segs, ends, kinds, events, shadow = reference(case.scene.name).paths_events(rays, seeds, case.depth)
    mean, se = cf.statistics(rad)
    print(cf.report(name, True, mean, se, case.want).replace(" on :", " mis:"))
    # the scene is closed and every ray meets it; what float32 lets escape to the sky (light_closed_forms'
    # docstring) adds at most 1 per path and channel: less than the standard error
    escaped = int(np.count_nonzero(ends == mr.MISS))
    print(f"{name} mis: {escaped} of {len(rad)} paths reach the sky")
    assert np.all(rad[:, 3] == 1.0) and np.all(escaped / len(rad) <= se)
    assert shadow.any() and np.any(events & mr.WEIGHTED_CONNECTION)
    assert np.all(np.abs(mean - case.want) <= 5.0 * se), cf.report(name, True, mean, se, case.want)


def test_both_techniques_contribute_in_the_cases():
    """Conditions on the reference alone: in the integrating sphere and inside the light, paths end on weighted
    light hits that add to the result (under option 1 they add nothing), and no hit there counts whole."""
    n = 1024
    for name in ("sphere_D8", "inside_D5"):
        c = cf.cases()[name]
        rad, _, _, _, ev, _ = reference(c.scene.name).paths_events(*c.rays_seeds(n), c.depth)
        assert np.count_nonzero(ev & mr.WEIGHTED_HIT) >= 30, name
        assert not np.any(ev & (mr.UNWEIGHTED_HIT_AFTER_DIFFUSE | mr.LIGHT_SPECULAR | mr.INFINITE_G)), name
