"""The C++ host's path queries (GPU): HipPathTracer::traceRadiance and HipPathTracer::cameraRays through the
hippt_render CLI's --radiance-in / --radiance-out, compared byte for byte with the Python calls."""
import json
import os
import subprocess

import numpy as np
import pytest

import hippt
from hippt import scenes
from test_gpu_ray_query import make_rays, pt, upload  # noqa: F401 (pt: the fixture)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "qt-raytracer_amd", "hippt_render")
W, H = 45, 26
OUT_DTYPE = np.dtype([("radiance", "<f4", (4,)), ("segments", "<i4")])


def run_cli(tmp_path, sc, source):
    obj = tmp_path / "cornell.obj"
    scenes.write_obj(sc, str(obj), style="plain")
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    out = tmp_path / "radiance.bin"
    r = subprocess.run([BIN, "--mesh", str(obj), "--albedo", albedo, "--width", str(W), "--height", str(H), "--spp", "1",
                        "--depth", "8", "--radiance-in", source, "--radiance-out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])["radiance_rays"], np.fromfile(str(out), OUT_DTYPE)


def test_cpp_host_trace_radiance_gives_the_python_calls_bytes(pt, tmp_path):
    sc = scenes.cornell34()
    rays = make_rays(sc, 257)
    seeds = hippt.path_seeds(257, 3)
    rec = np.zeros(257, np.dtype([("ray", "<f4", (8,)), ("seed", "<u4")]))
    rec["ray"], rec["seed"] = rays, seeds
    src = tmp_path / "rays.bin"
    rec.tofile(str(src))
    n, got = run_cli(tmp_path, sc, str(src))
    upload(pt, sc, w=W, h=H)
    rad, segs = pt.traceRadiance(rays, seeds, 8)
    assert np.count_nonzero(segs >= 2) > 64 and np.count_nonzero(segs == 0) == 14  # paths that bounce; the degenerate tail
    assert n == 257 and got.shape == (257,)
    assert np.ascontiguousarray(got["radiance"]).tobytes() == rad.tobytes()
    assert np.array_equal(got["segments"], segs)


def test_cpp_host_camera_rays_traced_give_the_python_calls_bytes(pt, tmp_path):
    sc = scenes.cornell34()
    n, got = run_cli(tmp_path, sc, "camera")
    upload(pt, sc, w=W, h=H)
    rad, segs = pt.traceRadiance(*pt.cameraRays(0), 8)
    assert n == W * H and got.shape == (W * H,)
    assert np.ascontiguousarray(got["radiance"]).tobytes() == rad.tobytes()
    assert np.array_equal(got["segments"], segs)
