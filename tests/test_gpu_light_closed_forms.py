"""Light sampling and emissive paths against closed forms (GPU): hipptTraceRadiance over the three closed scenes
of tests/light_closed_forms.py has their analytic mean radiance, with HIPPT_OPT_LIGHT_SAMPLING on and off.

Per case and option one call of N_GPU = 2^20 paths (rays and RNG states from numpy.random.default_rng), the mean
and the sample standard deviation accumulated in float64.  Per channel |mean - closed form| <= 5 SE: the bound
is against the closed form, never against the reference or the other option's run.  Power: SE <= 1 % of the
closed form with the option on and <= 2 % with it off, so an error of a factor (the sphere's area, the light
count, a dropped or doubled term of the depth series) cannot hide.  Each case runs with the scene in LDS and in
global memory.  The first N_BYTES = 4,097 paths of every run are also the bytes of tests/nee_ref.py over the same
rays and seeds: the statement of record (pinned to the same closed forms by
tests/test_light_closed_forms_cpu.py) and the device agree path by path.

Each run prints its mean, closed form, SE and z; profiles/lit_scenes/INDEX.md records them."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import hippt
import light_closed_forms as cf
import nee_ref as nr
import path_ref as pr
from test_gpu_ray_query import Ref, upload

pytestmark = pytest.mark.gpu

OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_QUERY_SLICE, 0),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_CHAIN_AUDIT, 0), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_SKY_RECT, 1),
        (hippt.OPT_PIXEL_FORMAT, hippt.PIXEL_ARGB), (hippt.OPT_LIGHT_SAMPLING, 0))


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    for k, v in OPTS:
        t.setOption(k, v)
    yield t
    for k, v in OPTS:
        t.setOption(k, v)
    hippt.load_library().cudaPathTracerShutdown()


@functools.lru_cache(maxsize=None)
def rays_seeds(name):
    """The case's N_GPU rays and seeds; computed once (both values of HIPPT_OPT_LDS_SCENE share them)."""
    rays, seeds = cf.cases()[name].rays_seeds(cf.N_GPU)
    rays.setflags(write=False)
    seeds.setflags(write=False)
    return rays, seeds


@functools.lru_cache(maxsize=None)
def reference_head(name, option):
    """(radiance, segments) of the first N_BYTES paths by tests/nee_ref.py; computed once, never modified."""
    case = cf.cases()[name]
    rays, seeds = rays_seeds(name)
    rad, segs = nr.NeeRef(case.scene, Ref(case.scene), sample=option).paths(rays[:cf.N_BYTES], seeds[:cf.N_BYTES],
                                                                            case.depth)[:2]
    rad.setflags(write=False)
    segs.setflags(write=False)
    return rad, segs


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", cf.CASES)
def test_mean_radiance_is_the_closed_form(pt, name, lds):
    case = cf.cases()[name]
    rays, seeds = rays_seeds(name)
    upload(pt, case.scene, lds)
    for option in cf.OPTIONS:
        pt.setOption(hippt.OPT_LIGHT_SAMPLING, int(option))
        rad, segs = pt.traceRadiance(rays, seeds, case.depth)
        mean, se = cf.statistics(rad)
        line = cf.report(name, option, mean, se, case.want) + f" lds={lds}"
        print(line)
        assert rad.shape == (cf.N_GPU, 4) and np.all(rad[:, 3] == 1.0), line  # every ray meets the scene
        assert np.all(np.abs(mean - case.want) <= 5.0 * se), line
        assert np.all(se <= (0.01 if option else 0.02) * case.want), line
        want_rad, want_segs = reference_head(name, option)
        pr.assert_paths(rad[:cf.N_BYTES], segs[:cf.N_BYTES], want_rad, want_segs, line)
