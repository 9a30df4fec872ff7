"""The ray and path queries' buffer table and staging layout (qt-raytracer_amd/csrc/hippt_query_layout.h)
from a host-compiled driver of the product's own header: tests/native/query_layout_check.cpp.  For every
kind of query call and slices of 1, 63, 64, 65 and 2^22 rays: the call's buffers are the ABI's
(include/hippt.h), every offset is a multiple of 16, the regions lie apart and inside the total, and the
total is at most what the formulas this layout replaced reserved (restated below).  No GPU.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "query_layout_check.cpp")

CAPS = (1, 63, 64, 65, 1 << 22)
RAYS, T, PRIM, OCCLUDED, HITS, SEEDS, RADIANCE, SEGMENTS, OUT_RAYS, OUT_SEEDS = range(10)
# include/hippt.h: bytes per ray, and whether the call writes the buffer
ABI = {RAYS: (32, 0), T: (4, 1), PRIM: (4, 1), OCCLUDED: (1, 1), HITS: (32, 1), SEEDS: (4, 0), RADIANCE: (16, 1),
       SEGMENTS: (4, 1), OUT_RAYS: (32, 1), OUT_SEEDS: (4, 1)}
# call -> (its buffers in order, the kind of the formula that sized its staging buffer before)
CALLS = {
    "closest_t": ((RAYS, T), "closest"),
    "closest_prim": ((RAYS, PRIM), "closest"),
    "closest_both": ((RAYS, T, PRIM), "closest"),
    "occlusion": ((RAYS, OCCLUDED), "closest"),
    "hits": ((RAYS, HITS), "records"),
    "path_segments": ((RAYS, SEEDS, RADIANCE, SEGMENTS), "path"),
    "path": ((RAYS, SEEDS, RADIANCE), "path"),
    "camrays_rays": ((OUT_RAYS,), "path"),
    "camrays_seeds": ((OUT_SEEDS,), "path"),
    "camrays_both": ((OUT_RAYS, OUT_SEEDS), "path"),
}


def up16(x):
    return (x + 15) & ~15


def stage_bytes_before(kind, cap):
    """query_locked's offT .. offG and stageBytes at the commit before the table."""
    off_t = cap * 32
    off_p = off_t + cap * 4
    off_o = off_p + cap * 4
    off_h = off_t
    off_s = cap * 32
    off_r = off_s + up16(cap * 4)
    off_g = off_r + cap * 16
    if kind == "path":  # hipptTraceRadiance, hipptCameraRays
        return off_g + cap * 4
    if kind == "records":
        return off_h + cap * 32
    return off_o + up16(cap)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("query_layout") / "query_layout_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        v = list(map(int, f[1:]))
        out[(f[0], v[0])] = (v[1], [tuple(v[i:i + 4]) for i in range(2, len(v), 4)])
    return out


def test_every_call_and_slice_is_laid_out(layouts):
    assert set(layouts) == {(name, cap) for name in CALLS for cap in CAPS}


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("cap", CAPS)
def test_layout(layouts, name, cap):
    slots, kind = CALLS[name]
    total, regions = layouts[(name, cap)]
    print(name, cap, total, regions, stage_bytes_before(kind, cap))
    assert tuple(r[0] for r in regions) == slots
    end = 0
    for slot, off, size, out in regions:
        assert (size, out) == (cap * ABI[slot][0], ABI[slot][1])
        assert off % 16 == 0
        assert off >= end, "regions overlap"
        end = off + size
    assert end <= total
    assert total <= stage_bytes_before(kind, cap)
