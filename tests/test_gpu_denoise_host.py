"""The C++ host's denoiser (GPU): HipPathTracer::denoise through the hippt_render CLI's --denoise writes the
frame words PathTracer.denoise() returns for the same scene, size and sample count."""
import json
import os
import subprocess

import numpy as np
import pytest

import hippt
from hippt import scenes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "qt-raytracer_amd", "hippt_render")
W, H, SPP = 45, 26, 4


def test_cpp_host_denoise_writes_the_python_calls_bytes(tmp_path):
    sc = scenes.cornell34()
    obj, out, plain = tmp_path / "cornell.obj", tmp_path / "clean.bin", tmp_path / "noisy.bin"
    scenes.write_obj(sc, str(obj), style="plain")
    albedo = ";".join(",".join(f"{c:.9g}" for c in a) for a in sc.albedo)
    base = [BIN, "--mesh", str(obj), "--albedo", albedo, "--width", str(W), "--height", str(H), "--spp", str(SPP),
            "--depth", "8"]
    r = subprocess.run(base + ["--denoise", "5", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["frames"] == SPP
    r = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # the same scene through the Python interface: the file's triangles under the CLI's camera
    mesh = scenes.from_mesh_file(str(obj), albedo=sc.albedo, lookfrom=(278, 278, -800), lookat=(278, 278, 0),
                                 vup=(0, 1, 0), vfov=40.0, aperture=0.0, focus=10.0)
    pt = hippt.PathTracer()
    try:
        pt.setDevices([])
        pt.setRowRange(0, 0)
        pt.uploadMesh(mesh)
        assert pt.initialize(W, H) and pt.renderFrames(SPP, 8), pt.lastError()
        noisy, _ = pt.readback()
        px, _ = pt.denoise(passes=5)
    finally:
        hippt.load_library().cudaPathTracerShutdown()
    assert plain.read_bytes() == noisy.tobytes()  # (the two interfaces render the same image)
    assert out.read_bytes() == px.tobytes()
    assert px.tobytes() != noisy.tobytes()
