"""HIPPT_OPT_SKY_COMBINE on the host (DESIGN.md §5 "Sky runs in the combine"): tests/native/sky_combine_model.cpp,
a stand-alone program over the product's predicate (hippt_sky_rect.h) and table builder (item_order.cpp),
built once with AddressSanitizer and UBSan.  Its sweep: every band pixel of every frame is in exactly one of
the compacted table (decoded with order_item's own arithmetic) and the combine's sky set, for widths 64, 100,
104 and 1920, heights that are no multiple of 8, both run shapes, row interleaves 1/2 and 3/8 and a row band,
and rectangles that are empty, full, interior, one pixel or touching each edge, and none.  The same program
checks the GPU tests' camera (tests/sky_combine_cam.py): whole sky tiles on all four sides at 104x72, and which
kernel variants have the combine's sky branch (plan::sky_combine_kernel).  No GPU (the option test loads the library
and sets an option; it starts nothing on a device).
"""
import os
import re
import shutil
import subprocess

import pytest

import hippt
import sky_combine_cam as scc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")

needs_gpp = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sky_combine") / "sky_combine_model")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", f"-I{CSRC}", "-I/opt/rocm/include",
                    os.path.join(REPO, "tests", "native", "sky_combine_model.cpp"), os.path.join(CSRC, "item_order.cpp"),
                    os.path.join(CSRC, "bvh_builder.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@needs_gpp
def test_every_sample_is_traced_or_combined_once(model):
    r = subprocess.run([model, "sweep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@needs_gpp
def test_the_gpu_tests_camera_leaves_sky_tiles_on_all_four_sides(model):
    sc = scc.pulled_back()
    w, h = scc.WIDTH, scc.HEIGHT
    cam = hippt.build_camera(lookfrom=sc.lookfrom, lookat=sc.lookat, vup=sc.vup, vfov=sc.vfov, aspect=w / h,
                             aperture=sc.aperture, focus=sc.focus)
    lo, hi, pad = scc.root_box(sc)
    nums = [*cam.origin, *cam.llc, *cam.horizontal, *cam.vertical, *lo, *hi, pad]
    r = subprocess.run([model, "camera", str(w), str(h)] + ["%.9g" % float(v) for v in nums], capture_output=True,
                       text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"rect (\d+) (\d+) (\d+) (\d+) sky_runs (\d+) of (\d+) sides (\d+) (\d+) (\d+) (\d+)", r.stdout)
    x0, y0, x1, y1, n, runs, *sides = (int(v) for v in m.groups())
    assert 8 <= x0 < x1 <= w - 8 and 8 <= y0 < y1 <= h - 8 and 0 < n < runs and all(s > 0 for s in sides)


def test_option_numbers_match_the_header():
    header = open(os.path.join(REPO, "include", "hippt.h")).read()
    assert re.search(r"HIPPT_OPT_SKY_COMBINE\s*=\s*41\b", header) and hippt.OPT_SKY_COMBINE == 41
    assert re.search(r"HIPPT_INFO_SKY_COMBINE\s*=\s*112\b", header) and hippt.INFO_SKY_COMBINE == 112
    lib = hippt.load_library()
    assert lib.hipptGetOption(hippt.OPT_SKY_COMBINE) == -1
    try:
        assert lib.hipptSetOption(hippt.OPT_SKY_COMBINE, 0) and lib.hipptGetOption(hippt.OPT_SKY_COMBINE) == 0
        for v in (1, 2, -2):
            assert not lib.hipptSetOption(hippt.OPT_SKY_COMBINE, v)
    finally:
        assert lib.hipptSetOption(hippt.OPT_SKY_COMBINE, -1)
