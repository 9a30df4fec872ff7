"""The render pad (HIPPT_OPT_RENDER_PAD) from a host-compiled model of the kernels' box
test: tests/native/pad_model.cpp drives the product's own slab arithmetic
(qt-raytracer_amd/csrc/hippt_slab.h, the header the gfx950 kernels call) and the product's builder over
rays of the FP32 oracle (oracle/pt_oracle.c): the camera rays and every scattered segment of the oracle's
paths, plus adversarial families (grazing rays off every triangle, direction components at the 1e-20
clamp, origins at box corners and edges).  For each oracle-accepted closest hit every box on the
primitive's root-to-leaf path must pass the test with bestT = the hit's t, with v_rcp_f32 modelled as
the correctly rounded reciprocal moved by -1, 0, +1 ulp per axis.

The model reports the smallest pad that passes, in units of M * 2^-24 (M: the largest |coordinate| of
the scene and the camera).  The rule: renderPad = 4 x that, rounded up to a power of two
times M, never below M * 2^-21; the shipped default must be at least as loose.  No GPU.
"""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import hippt
import pyoracle
from hippt import scenes
from render_pad_scenes import GRAZING_SIZE, grazing_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")
ORACLE = os.path.join(REPO, "oracle")
SRC = os.path.join(REPO, "tests", "native", "pad_model.cpp")

WIDTH, HEIGHT, SPP, DEPTH = 64, 36, 8, 8


def _small_cornell():
    """cornell34 with every coordinate (and the camera) divided by 555: M ~ 1.44 instead of 800."""
    sc = scenes.cornell34()
    s = np.float32(555.0)
    sc.verts = (sc.verts / s).astype(np.float32)
    sc.lookfrom = tuple(float(np.float32(v) / s) for v in sc.lookfrom)
    sc.lookat = tuple(float(np.float32(v) / s) for v in sc.lookat)
    sc.name = "cornell34_div555"
    return sc


# scene: (maker, (width, height, spp) of its path rays); the grazing scene at its GPU test's size
SCENES = {"cornell34": (scenes.cornell34, (WIDTH, HEIGHT, SPP)), "cornell_mixed": (scenes.cornell_mixed, (WIDTH, HEIGHT, SPP)),
          "cornell34_div555": (_small_cornell, (WIDTH, HEIGHT, SPP)), "grazing": (grazing_scene, GRAZING_SIZE)}


def _write_scene(sc, path, size=(WIDTH, HEIGHT, SPP)):
    verts = np.ascontiguousarray(sc.verts, np.float32).reshape(-1, 9)
    sph = np.ascontiguousarray(sc.spheres, np.float32).reshape(-1, 4)
    mats = np.ascontiguousarray(sc.materials())
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", verts.shape[0], sph.shape[0], mats.shape[0], *size, DEPTH))
        f.write(struct.pack("<12d", *sc.lookfrom, *sc.lookat, *sc.vup, sc.vfov, sc.aperture, sc.focus))
        f.write(verts.tobytes())
        f.write(np.ascontiguousarray(sc.tri_mat, np.int32).tobytes())
        f.write(sph.tobytes())
        f.write(np.ascontiguousarray(sc.sph_mat, np.int32).tobytes())
        f.write(mats.tobytes())


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    pyoracle.lib()  # builds oracle/liboracle.so when missing
    exe = str(tmp_path_factory.mktemp("pad_model") / "pad_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-ffp-contract=off", "-I" + CSRC, "-I" + ORACLE,
                    "-o", exe, SRC, os.path.join(CSRC, "bvh_builder.cpp"), "-L" + ORACLE, "-loracle",
                    "-Wl,-rpath," + ORACLE], check=True)
    return exe


@pytest.fixture(scope="module")
def results(model, tmp_path_factory):
    """One model run per scene, shared by the tests: the parsed first line, the families, the text."""
    out = {}
    d = tmp_path_factory.mktemp("pad_scenes")
    for name, (make, size) in SCENES.items():
        path = str(d / (name + ".bin"))
        _write_scene(make(), path, size)
        r = subprocess.run([model, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        head = dict(re.findall(r"(\w+)=([-+.\deE]+)", r.stdout.splitlines()[0]))
        fam = {m.group(1): (int(m.group(2)), float(m.group(3)))
               for m in re.finditer(r"family (\w+) hits=(\d+) need_units=([\d.]+)", r.stdout)}
        out[name] = (head, fam, r.stdout)
    return out


def _rule_exponent(need_units):
    """renderPad = 4 x the measured requirement rounded up to a power of two times M, never below
    M * 2^-21: the exponent e of M * 2^-e."""
    units = max(4.0 * need_units, 8.0)  # 8 units = M * 2^-21
    return 24 - math.ceil(math.log2(units))


def test_default_matches_the_header():
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    slab = open(os.path.join(CSRC, "hippt_slab.h")).read()
    default = int(re.search(r"kRenderPadDefault = (\d+)", slab).group(1))
    assert re.search(r"HIPPT_OPT_RENDER_PAD\s*=\s*34\b", header) and hippt.OPT_RENDER_PAD == 34
    assert re.search(r"HIPPT_INFO_RENDER_PAD\s*=\s*105\b", header) and hippt.INFO_RENDER_PAD == 105
    assert re.search(r"Default %d \(DESIGN.md" % default, header)
    lib = hippt.load_library()
    assert lib.hipptGetOption(hippt.OPT_RENDER_PAD) == default
    try:
        for v in (0, 17, 21):
            assert lib.hipptSetOption(hippt.OPT_RENDER_PAD, v) and lib.hipptGetOption(hippt.OPT_RENDER_PAD) == v
        for v in (-1, 1, 16, 22):
            assert not lib.hipptSetOption(hippt.OPT_RENDER_PAD, v)
    finally:
        assert lib.hipptSetOption(hippt.OPT_RENDER_PAD, default)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_measured_requirement_and_the_rule(results, name):
    head, fam, text = results[name]
    print(text)
    slab = open(os.path.join(CSRC, "hippt_slab.h")).read()
    default = int(re.search(r"kRenderPadDefault = (\d+)", slab).group(1))
    need = float(head["need_units"])
    # the sample reaches the cases it is there for (the grazing scene: 4 triangles, a smaller image)
    if name == "grazing":
        assert fam["camera"][0] > 2000 and fam["scattered"][0] > 10000 and fam["grazing"][0] > 500, text
    else:
        assert int(head["hits"]) > 50000 and fam["camera"][0] > 5000 and fam["scattered"][0] > 20000, text
        assert fam["grazing"][0] > 10000 and fam["clamp"][0] > 1000 and fam["corners"][0] > 1000, text
    # shadow-acne self-hits (the oracle accepts t >= 0.001 on the ray's own triangle) occur and are
    # checked at the room's scale; at 1/555 of it tmin is 555 times longer against the error, none occur
    if float(head["M"]) > 100.0:
        assert int(head["self_hits"]) > 0, text
    if name == "grazing":  # in the oracle's own paths at the GPU test's size
        assert int(head["path_self_hits"]) > 0, text
    # the builder's pad itself passes everything (need_units is 1e9 otherwise)
    assert need <= 256.0, text
    # the shipped default is the rule's exponent or looser, and every ray passes at it and at every
    # looser option value (the option's exact arithmetic: slab::trim_scale, trim_of)
    rule = _rule_exponent(need)
    print(f"{name}: measured requirement {need} x M*2^-24, rule exponent {rule}, default {default}")
    assert default <= rule, text
    for e in range(17, default + 1):
        assert int(head[f"fail{e}"]) == 0, text
