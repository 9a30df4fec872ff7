"""The sky rectangle (HIPPT_OPT_SKY_RECT) from a host-compiled driver of the product's own
bound (qt-raytracer_amd/csrc/hippt_sky_rect.h) over the product's builder and the FP32 oracle:
tests/native/sky_rect_check.cpp.  Every oracle camera ray of a pixel outside the rectangle, and the
pixel's four footprint corners and its centre, must miss the scene; the rectangle must leave pixels
outside (it is not vacuous), and must not be wider than the projection of the builder-padded box plus
two pixels a side.  Cameras the bound does not cover give no rectangle.  No GPU.
"""
import dataclasses
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import hippt
import pyoracle
from hippt import scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")
ORACLE = os.path.join(REPO, "oracle")
SRC = os.path.join(REPO, "tests", "native", "sky_rect_check.cpp")

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


SCENES = {"cornell34": scenes.cornell34, "cornell_mixed": scenes.cornell_mixed, "blob70k": scenes.blob70k,
          "cornell34_div555": _small_cornell}

# cornell34 seen by cameras the bound does not cover (no rectangle) ...
DEGENERATE = {
    "inside": dict(lookfrom=(278.0, 278.0, 278.0), lookat=(278.0, 278.0, 555.0)),
    "looking_away": dict(lookfrom=(278.0, 278.0, -800.0), lookat=(278.0, 278.0, -1600.0)),
    # beside the box, looking along it: the corners at z < 278 are behind the image plane
    "corner_behind": dict(lookfrom=(-100.0, 278.0, 278.0), lookat=(-100.0, 278.0, 1000.0)),
    "aperture": dict(aperture=0.1, focus=1078.0),
}
# ... and by one turned 60 degrees off it: every corner in front of the camera and off-screen
SKY_ONLY = dict(lookfrom=(278.0, 278.0, -800.0), lookat=(278.0 + 866.0, 278.0, -800.0 + 500.0))


def _write_scene(sc, path, size=None):
    width, height, spp = size or (WIDTH, HEIGHT, SPP)
    verts = np.ascontiguousarray(sc.verts, np.float32).reshape(-1, 9)
    sph = np.ascontiguousarray(sc.spheres, np.float32).reshape(-1, 4)
    mats = np.ascontiguousarray(sc.materials())
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", verts.shape[0], sph.shape[0], mats.shape[0], width, height, spp, DEPTH))
        f.write(struct.pack("<12d", *sc.lookfrom, *sc.lookat, *sc.vup, sc.vfov, sc.aperture, sc.focus))
        f.write(verts.tobytes())
        f.write(np.ascontiguousarray(sc.tri_mat, np.int32).tobytes())
        f.write(sph.tobytes())
        f.write(np.ascontiguousarray(sc.sph_mat, np.int32).tobytes())
        f.write(mats.tobytes())


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    pyoracle.lib()  # builds oracle/liboracle.so when missing
    d = tmp_path_factory.mktemp("sky_rect")
    exe = str(d / "sky_rect_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-ffp-contract=off", "-I" + CSRC,
                    "-I" + ORACLE, "-o", exe, SRC, os.path.join(CSRC, "bvh_builder.cpp"), "-L" + ORACLE, "-loracle",
                    "-Wl,-rpath," + ORACLE], check=True)
    cache = {}

    def run(name, sc, *args, size=None):
        key = (name,) + args
        if key not in cache:
            path = str(d / (name + ".bin"))
            _write_scene(sc, path, size)
            r = subprocess.run([exe, path, *args], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            lines = r.stdout.splitlines()
            head = {k: float(v) for k, v in re.findall(r"(\w+)=([-+.\deE]+)", lines[0])}
            box = np.array(lines[1].split()[1:], np.float64)
            cam = np.array(lines[2].split()[1:], np.float64).reshape(4, 3)
            cache[key] = (head, box, cam, r.stdout)
        return cache[key]

    return run


def test_the_header_compiles_with_gpp_alone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "hippt_sky_rect.h"\nint main() { return hippt::skyrect::whole(4, 4).x1 == 4 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "t"), str(src)], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


def test_option_numbers_match_the_header():
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    assert re.search(r"HIPPT_OPT_SKY_RECT\s*=\s*35\b", header) and hippt.OPT_SKY_RECT == 35
    assert re.search(r"HIPPT_INFO_SKY_RECT_PIXELS\s*=\s*106\b", header) and hippt.INFO_SKY_RECT_PIXELS == 106
    lib = hippt.load_library()
    assert lib.hipptGetOption(hippt.OPT_SKY_RECT) == 1
    try:
        assert lib.hipptSetOption(hippt.OPT_SKY_RECT, 0) and lib.hipptGetOption(hippt.OPT_SKY_RECT) == 0
        for v in (-1, 2):
            assert not lib.hipptSetOption(hippt.OPT_SKY_RECT, v)
    finally:
        assert lib.hipptSetOption(hippt.OPT_SKY_RECT, 1)


# A far, oblique camera with a long lens.  The kernel's direction (llc + s*H + t*V) - origin carries an
# error of about an ulp of the origin's coordinates, 2^-11 here, whatever the focus distance; at focus 1 a
# pixel's pitch on the image plane is 5e-5, so the rays land pixels away from their ideal ones and the
# oracle hits the scene up to 4 pixels outside the projected rectangle at 1920x1080 (the image size at
# which the pitch is that small): such a camera must get no rectangle (the header's bound: 11.5 pixels,
# 1.1 at focus 10).  At focus 300 the bound is 0.04 pixels: the rectangle stands and every ray outside it
# misses.
FAR = dict(lookfrom=(5278.0, 2278.0, -6000.0), lookat=(278.0, 278.0, 278.0), vfov=6.0)
FULL_SIZE = (1920, 1080, 2)


@pytest.mark.parametrize("focus", [1.0, 10.0])
def test_far_camera_with_a_short_focus_gets_no_rectangle(check, focus):
    sc = dataclasses.replace(scenes.cornell34(), focus=focus, **FAR)
    head, _, _, text = check("cornell34_far_focus%g" % focus, sc, size=FULL_SIZE)
    assert head["whole"] == 1 and head["outside"] == 0, text


def test_far_camera_at_full_resolution(check):
    sc = dataclasses.replace(scenes.cornell34(), focus=300.0, **FAR)
    head, _, _, text = check("cornell34_far_focus300", sc, size=FULL_SIZE)
    print(text)
    w, h, spp = FULL_SIZE
    assert head["whole"] == 0 and head["outside"] * 2 >= w * h, text
    assert head["rays_outside"] == head["outside"] * (spp + 5), text
    assert head["violations"] == 0 and head["hit_outside"] == 0 and head["pixels_hit"] > 0, text


def test_direction_error_bound_of_the_default_camera(tmp_path):
    """The default camera's direction-error bound is a small fraction of a pixel (0.03 at 1080p, 0.07 at 4K):
    the rectangle stands at both sizes."""
    src = tmp_path / "t.cpp"
    src.write_text('''#include "hippt_sky_rect.h"
#include <cstdio>
struct Cam { float origin[3], llc[3], horizontal[3], vertical[3], u[3], v[3]; float lens_radius; };
int main() {
    // cornell34's default camera at 16:9 (focus 10): origin, llc, horizontal, vertical
    Cam c{{278, 278, -800}, {284.470581f, 274.360291f, -790}, {-12.941164f, 0, 0}, {0, 7.27940464f, 0},
          {1, 0, 0}, {0, 1, 0}, 0};
    const float lo[3] = {-0.0122f, -0.0122f, -0.0122f}, hi[3] = {555.0122f, 555.0122f, 555.0122f};
    const hippt::skyrect::Rect a = hippt::skyrect::sky_rect(c, 1920, 1080, lo, hi, 0.0122f, 34);
    const hippt::skyrect::Rect b = hippt::skyrect::sky_rect(c, 3840, 2160, lo, hi, 0.0122f, 34);
    std::printf("%d %d\\n", hippt::skyrect::is_whole(a, 1920, 1080), hippt::skyrect::is_whole(b, 3840, 2160));
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "t"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "0"]


def _projection(box, cam, pad):
    """The pixel-unit bounding rectangle of the box moved out by `pad`, projected in double through the
    camera's origin, llc, horizontal and vertical (numpy's solve, not the header's arithmetic)."""
    o, llc, h, v = cam
    A = np.stack([llc - o, h, v], axis=1)
    lo, hi = box[:3] - pad, box[3:] + pad
    px, py = [], []
    for c in range(8):
        q = np.array([hi[k] if (c >> k) & 1 else lo[k] for k in range(3)]) - o
        lam, ls, lt = np.linalg.solve(A, q)
        assert lam > 0
        px.append(ls / lam * max(1, WIDTH - 1))
        py.append(lt / lam * max(1, HEIGHT - 1))
    return min(px), min(py), max(px), max(py)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_rays_outside_the_rectangle_miss(check, name):
    head, box, cam, text = check(name, SCENES[name]())
    print(text)
    pixels = WIDTH * HEIGHT
    assert head["whole"] == 0 and head["none_whole"] == 1, text
    # every oracle camera ray, footprint corner and centre of a pixel outside the rectangle misses
    assert head["outside"] > 0 and head["rays_outside"] == head["outside"] * (SPP + 5), text
    assert head["violations"] == 0 and head["hit_outside"] == 0, text
    assert 0 < head["pixels_hit"] <= pixels - head["outside"], text
    if name == "cornell34":  # not vacuous: about 40% of the pixels are expected outside
        print("cornell34 pixels outside: %d of %d" % (head["outside"], pixels))
        assert head["outside"] * 3 >= pixels, text
    # no wider than the double-precision projection of the builder-padded box plus two pixels a side
    # (plus the rule's own 2^-20 of the image size, doubled here for the two roundings it sits between)
    x0, y0, x1, y1 = _projection(box, cam, 0.0)
    ex, ey = WIDTH * 2.0 ** -19, HEIGHT * 2.0 ** -19
    # ... and the extra pad the rule adds to the box: its own projection, measured
    wx0, wy0, wx1, wy1 = _projection(box, cam, head["pad"])
    assert head["x0"] >= min(max(x0 - 2 - ex - (x0 - wx0), 0), WIDTH), text
    assert head["y0"] >= min(max(y0 - 2 - ey - (y0 - wy0), 0), HEIGHT), text
    assert head["x1"] <= max(min(x1 + 2 + ex + (wx1 - x1), WIDTH), 0), text
    assert head["y1"] <= max(min(y1 + 2 + ey + (wy1 - y1), HEIGHT), 0), text
    # and it contains the projection itself
    assert head["x0"] <= max(x0, 0) and head["y0"] <= max(y0, 0), text
    assert head["x1"] >= min(x1, WIDTH) and head["y1"] >= min(y1, HEIGHT), text


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_cameras_without_a_rectangle(check, name):
    head, _, _, text = check("cornell34_" + name, dataclasses.replace(scenes.cornell34(), **DEGENERATE[name]))
    assert head["whole"] == 1 and head["outside"] == 0, text


def test_a_nan_component_gives_no_rectangle(check):
    head, _, _, text = check("cornell34", scenes.cornell34(), "nan")
    assert head["whole"] == 1 and head["outside"] == 0, text


def test_a_camera_that_sees_only_sky(check):
    head, _, _, text = check("cornell34_sky_only", dataclasses.replace(scenes.cornell34(), **SKY_ONLY))
    pixels = WIDTH * HEIGHT
    assert head["whole"] == 0 and head["x1"] <= head["x0"] and head["outside"] == pixels, text
    assert head["rays_outside"] == pixels * (SPP + 5) and head["violations"] == 0 and head["pixels_hit"] == 0, text
