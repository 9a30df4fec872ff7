"""The C++ host's hit records (GPU): HipPathTracer::traceHits through the hippt_render CLI's --pick, all 8
words of the record compared with the reference of tests/hit_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import hippt
from hippt import scenes
from hit_ref import HitRef
from test_gpu_ray_query import Ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "qt-raytracer_amd", "hippt_render")
W, H = 45, 26


@pytest.mark.parametrize("x,y,hit", [(22, 13, True), (15, 8, True), (7, 19, False)])
def test_cpp_host_trace_hits_matches_reference(tmp_path, x, y, hit):
    sc = scenes.cornell34()
    obj = tmp_path / "cornell.obj"
    scenes.write_obj(sc, str(obj), style="plain")
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    r = subprocess.run([BIN, "--mesh", str(obj), "--albedo", albedo, "--width", str(W), "--height", str(H), "--spp", "1",
                        "--depth", "8", "--pick", f"{x},{y}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pick = json.loads(r.stdout.strip().splitlines()[-1])["pick"]
    # the pixel centre's pinhole ray, built as the CLI builds it (float32)
    cam = hippt.build_camera(sc.lookfrom, sc.lookat, sc.vup, sc.vfov, W / H, 0.0, 10.0)
    f = np.float32
    s, v = (f(x) + f(0.5)) / f(W - 1), (f(y) + f(0.5)) / f(H - 1)
    ray = np.zeros((1, 8), np.float32)
    for k in range(3):
        ray[0, k] = cam.origin[k]
        ray[0, 4 + k] = f(cam.llc[k]) + s * f(cam.horizontal[k]) + v * f(cam.vertical[k]) - f(cam.origin[k])
    ray[0, 3], ray[0, 7] = 0.001, np.inf
    ref = Ref(sc)
    et, ep = ref.closest(ray)
    want = HitRef(sc, ref).records(ray, et, ep)
    assert (ep[0] >= 0) == hit  # a condition on the reference: two pixels in the box, one on the sky
    assert pick["ray_hit_words"] == [int(w) for w in want.view(np.uint32).reshape(-1)], (pick, want)
    assert pick["ray_hit_words"][:2] == [pick["ray_t_bits"], pick["ray_prim"] & 0xFFFFFFFF]  # traceRays' words
