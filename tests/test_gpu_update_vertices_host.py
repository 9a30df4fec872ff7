"""The C++ host's vertex update (GPU): HipPathTracer::updateVertices through the hippt_render CLI
(--update-mesh: sample 0 over --mesh, the remaining samples over the same triangles at the second
file's vertices), compared with the oracle's frames continued across the update."""
import json
import os
import subprocess

import numpy as np
import pytest

import hippt
import pyoracle as po
from hippt import scenes
from refit_util import verts_of, with_verts, wobble

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "qt-raytracer_amd", "hippt_render")
W, H, SPP, DEPTH = 45, 26, 4, 6


def test_cpp_host_update_vertices_matches_oracle(tmp_path):
    sc = scenes.cornell34()
    a, b, out = tmp_path / "a.obj", tmp_path / "b.obj", tmp_path / "frame.argb"
    scenes.write_obj(sc, str(a), style="plain")
    scenes.write_obj(with_verts(sc, wobble(verts_of(sc))), str(b), style="plain")
    # the vertices as the host reads them back from the files
    v0, v1 = hippt.read_mesh(str(a))[0], hippt.read_mesh(str(b))[0]
    assert v0.shape == v1.shape == verts_of(sc).shape and not np.array_equal(v0, v1)
    albedo = ";".join(",".join(f"{c:.9g}" for c in x) for x in sc.albedo)
    r = subprocess.run([BIN, "--mesh", str(a), "--update-mesh", str(b), "--albedo", albedo, "--width", str(W),
                        "--height", str(H), "--spp", str(SPP), "--depth", str(DEPTH), "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    px = np.fromfile(out, np.uint32).reshape(H, W)
    _, acc0, segs0, _ = po.MeshScene(with_verts(sc, v0), W, H).frames(0, 1, DEPTH)
    opx, _, segs1, _ = po.MeshScene(with_verts(sc, v1), W, H).frames(1, SPP - 1, DEPTH, accum=acc0)
    assert np.array_equal(px, opx), f"{np.count_nonzero(px != opx)} pixels differ"
    assert info["frames"] == SPP and info["segments"] == segs0 + segs1
    # a mesh of another triangle count is refused
    c = tmp_path / "c.obj"
    scenes.write_obj(scenes.blob_scene(8, 5), str(c), style="plain")
    r = subprocess.run([BIN, "--mesh", str(a), "--update-mesh", str(c), "--albedo", albedo, "--width", str(W),
                        "--height", str(H), "--spp", "2", "--depth", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "numTris" in r.stderr
