"""Light sampling with MIS against closed forms (GPU): hipptTraceRadiance over the three closed scenes of
tests/light_closed_forms.py has their analytic mean radiance with HIPPT_OPT_LIGHT_SAMPLING_MODE = HIPPT_LIGHT_SAMPLING_MIS.

Per case one call of N_GPU = 2^20 paths, the mean and the sample standard deviation accumulated in float64.  Per
channel |mean - closed form| <= 5 SE, against the closed form only.  Power: SE <= 2 % of the closed form, the
looser of the two conditions of tests/test_gpu_light_closed_forms.py (no bound on the power heuristic's variance
is derived here).  Each case runs with the scene in LDS and in global memory.  The first N_BYTES = 4,097 paths of
every run are also the bytes of tests/mis_ref.py over the same rays and seeds.

Each run prints its mean, closed form, SE and z; profiles/mis/INDEX.md records them."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import hippt
import light_closed_forms as cf
import mis_ref as mr
import path_ref as pr
from test_gpu_light_closed_forms import OPTS, rays_seeds
from test_gpu_ray_query import Ref, upload

pytestmark = pytest.mark.gpu


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
def reference_head(name):
    """(radiance, segments) of the first N_BYTES paths by tests/mis_ref.py; computed once, never modified."""
    case = cf.cases()[name]
    rays, seeds = rays_seeds(name)
    rad, segs = mr.MisRef(case.scene, Ref(case.scene)).paths(rays[:cf.N_BYTES], seeds[:cf.N_BYTES], case.depth)[:2]
    rad.setflags(write=False)
    segs.setflags(write=False)
    return rad, segs


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("name", cf.CASES)
def test_mean_radiance_is_the_closed_form(pt, name, lds):
    case = cf.cases()[name]
    rays, seeds = rays_seeds(name)
    upload(pt, case.scene, lds)
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, hippt.LIGHT_SAMPLING_MIS)
    rad, segs = pt.traceRadiance(rays, seeds, case.depth)
    mean, se = cf.statistics(rad)
    line = cf.report(name, True, mean, se, case.want).replace(" on :", " mis:") + f" lds={lds}"
    print(line)
    assert rad.shape == (cf.N_GPU, 4) and np.all(rad[:, 3] == 1.0), line  # every ray meets the scene
    assert np.all(np.abs(mean - case.want) <= 5.0 * se), line
    assert np.all(se <= 0.02 * case.want), line
    want_rad, want_segs = reference_head(name)
    pr.assert_paths(rad[:cf.N_BYTES], segs[:cf.N_BYTES], want_rad, want_segs, line)
