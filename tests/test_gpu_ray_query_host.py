"""The C++ host's ray queries (GPU): HipPathTracer::pick and HipPathTracer::traceRays through the
hippt_render CLI, compared with the oracle's closest hit of the same rays."""
import json
import os
import subprocess

import numpy as np
import pytest

import hippt
from hippt import scenes
from test_gpu_ray_query import Ref, camera_rays

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "qt-raytracer_amd", "hippt_render")
W, H = 45, 26


@pytest.mark.parametrize("x,y", [(0, 0), (22, 13), (44, 25), (7, 19)])
def test_cpp_host_pick_and_trace_rays_match_oracle(tmp_path, x, y):
    sc = scenes.cornell34()
    obj = tmp_path / "cornell.obj"
    scenes.write_obj(sc, str(obj), style="plain")
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    r = subprocess.run([BIN, "--mesh", str(obj), "--albedo", albedo, "--width", str(W), "--height", str(H), "--spp", "1",
                        "--depth", "8", "--pick", f"{x},{y}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pick = json.loads(r.stdout.strip().splitlines()[-1])["pick"]
    ref = Ref(sc)
    # pick: sample 0's camera ray of the pixel
    rt, rp = ref.closest(camera_rays(sc, W, H, 0)[y * W + x:y * W + x + 1])
    assert (pick["x"], pick["y"]) == (x, y)
    assert pick["prim"] == int(rp[0]) and pick["t_bits"] == int(rt.view(np.uint32)[0])
    # traceRays: the pixel centre's pinhole ray, built as the CLI builds it (float32)
    cam = hippt.build_camera(sc.lookfrom, sc.lookat, sc.vup, sc.vfov, W / H, 0.0, 10.0)
    f = np.float32
    s, v = (f(x) + f(0.5)) / f(W - 1), (f(y) + f(0.5)) / f(H - 1)
    ray = np.zeros((1, 8), np.float32)
    for k in range(3):
        ray[0, k] = cam.origin[k]
        ray[0, 4 + k] = f(cam.llc[k]) + s * f(cam.horizontal[k]) + v * f(cam.vertical[k]) - f(cam.origin[k])
    ray[0, 3], ray[0, 7] = 0.001, np.inf
    et, ep = ref.closest(ray)
    assert pick["ray_prim"] == int(ep[0]) and pick["ray_t_bits"] == int(et.view(np.uint32)[0])
