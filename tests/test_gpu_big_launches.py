"""Launches with more rays than lanes (GPU): hipptTraceRays, hipptOccluded, hipptTraceHits, hipptTraceRadiance and the
ray-per-lane render route at 2^20 items and above, bit for bit.

The other files compare at most 4,097 rays with the references, in launches of ceil(N / 256) blocks: a lane starts one
path there, rarely two.  Here the grid is capped at CUs x blocks per CU, every lane runs path after path through the
reset at the top of the persistent loop, and from N = 2^20 on a wave claims 256 indices at a time and serves them over
several refills.

A query's result depends on the ray (and its seed) alone, not on its index.  So a referenced set of n rays, n odd,
is tiled to N: big[i] = base[i % n], and out[i] must equal ref[i % n] word for word.  n is coprime with 64: every
repetition is shifted against the wave boundaries, and every referenced ray (the degenerate ones too) comes up in
every lane position, next to other neighbours and behind other predecessors in its lane.  The references are the
cached cases of the small tests; nothing is restated here.  The tiling and the comparison run on the device.

A failure names the first differing indices i, the referenced ray i % n, the lane i % 64, and in how many of its
places that ray is wrong: a ray wrong everywhere is an arithmetic error, one wrong in some lanes a state leak, and
indices left at the fill word (or zero) a claim error.  Every output is filled with SENTINEL words before its call."""
import ctypes

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import env_ref as ev
import envs_ref as es
import hippt
import hit_ref as hr
import path_ref as pr
import select_ref as sr
from hippt import scenes
from test_gpu_env_sampling import OPTS, assert_image, info, sampling
from test_gpu_environment import E5, want_image, want_paths
from test_gpu_ray_query import assert_same, case, upload

pytestmark = pytest.mark.gpu

# the largest launch that claims 64 indices at a time (a saturated grid, a last shard one ray short), the smallest that
# claims 256, and one of 256 with about six paths per lane
SIZES = (2 ** 20 - 1, 2 ** 20, 3 * 2 ** 20 + 1)
HOST_N = 2 ** 20 + 4097
SENTINEL = 0x7fc0dead
BYTE_FILL = 0xad  # (occlusion flags are bytes)
W, H = 32, 24
SMALL = 4096  # rays per launch of the regime the reference tests pin
# A failed test's traceback keeps its PathTracer until some later moment, and PathTracer.__del__ shuts the library down:
# in the middle of the next test, which then fails too.  Kept here, they go at the interpreter's exit.
_TRACERS = []


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    _TRACERS.append(t)
    t.setDevices([0])
    t.setRowRange(0, 0)
    t.useBuiltinScene(hippt.SCENE_SPHERE4)
    scratch_mb = info(hippt.OPT_SCRATCH_MB)
    for k, v in OPTS:
        t.setOption(k, v)
    t.setEnvironment(None)
    yield t
    t.setEnvironment(None)  # later files see the gradient
    for k, v in OPTS:  # (OPT_QUERY_SLICE among them)
        t.setOption(k, v)
    t.setOption(hippt.OPT_SCRATCH_MB, scratch_mb)
    t.setRowRange(0, 0)
    t.setDevices([])
    hippt.load_library().cudaPathTracerShutdown()


def device():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def assert_saturating(items, n=1):
    """More items than lanes can be resident (at most 8 blocks of 256 lanes per CU), and an odd tile."""
    lanes = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    assert items > lanes, f"{items} items do not outnumber the {lanes} lanes of this device"
    assert n % 2 == 1, f"a tile of {n} rays is not coprime with the wave"


# ---- queries into filled outputs -----------------------------------------------------------------------------
def _ptr(a):
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _filled(shape, like, fill=SENTINEL, byte=False):
    if isinstance(like, torch.Tensor):
        return torch.full(shape, fill, dtype=torch.uint8 if byte else torch.int32, device=like.device)
    return np.full(shape, fill, np.uint8 if byte else np.int32)


def _words(*outs):
    """The outputs' words side by side: int32 (N, k) on the device."""
    cols = []
    for a in outs:
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(device())
        cols.append(a.to(torch.int32).reshape(a.shape[0], -1))
    return cols[0] if len(cols) == 1 else torch.cat(cols, dim=1)


def query(kind, rays, seeds=None):
    """One call of the C entry point of `kind` over rays (and seeds) in host or device memory, into outputs filled
    with SENTINEL words (BYTE_FILL bytes): the outputs' words, int32 (N, k) on the device.  k: closest 2 (t, prim),
    occluded 1, hits 8, radiance 5 (rgba, segments)."""
    lib = hippt.load_library()
    n = int(rays.shape[0])
    on_device = isinstance(rays, torch.Tensor)
    flags = hippt.RAYS_DEVICE if on_device else 0
    e = ctypes.c_char_p()
    if kind == "closest":
        outs = (_filled((n,), rays), _filled((n,), rays))
    elif kind == "occluded":
        outs = (_filled((n,), rays, BYTE_FILL, byte=True),)
    elif kind == "hits":
        outs = (_filled((n, 8), rays),)
    else:
        outs = (_filled((n, 4), rays), _filled((n,), rays))
    if on_device:
        torch.cuda.synchronize()  # the fills, and what made the rays
    if kind == "closest":
        ok = lib.hipptTraceRays(_ptr(rays), n, flags, _ptr(outs[0]), _ptr(outs[1]), ctypes.byref(e))
    elif kind == "occluded":
        ok = lib.hipptOccluded(_ptr(rays), n, flags, _ptr(outs[0]), ctypes.byref(e))
    elif kind == "hits":
        ok = lib.hipptTraceHits(_ptr(rays), n, flags, _ptr(outs[0]), ctypes.byref(e))
    else:
        ok = lib.hipptTraceRadiance(_ptr(rays), _ptr(seeds), n, 8, flags, _ptr(outs[0]), _ptr(outs[1]), ctypes.byref(e))
    assert ok, (kind, n, e.value)
    return _words(*outs)


def ref_words(*arrays):
    """Reference arrays (float32, int32, uint32, bool or records of 4-byte fields) as int32 words (n, k) on the device."""
    cols = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        n = a.shape[0]
        a = a.astype(np.int32) if a.dtype == bool else a.view(np.int32)
        cols.append(np.array(a.reshape(n, -1)))
    return torch.from_numpy(np.concatenate(cols, axis=1)).to(device())


# ---- the comparison ----------------------------------------------------------------------------------------------
def _hex(row):
    return "[" + " ".join(f"{v & 0xffffffff:08x}" for v in row.tolist()) + "]"


def assert_tiled(got, ref, idx, what, fill=SENTINEL):
    """got[i] == ref[idx[i]] in every word (int32 (N, k) and (n, k) on the device)."""
    n = ref.shape[0]
    assert got.shape == (idx.shape[0], ref.shape[1]), (what, tuple(got.shape), tuple(ref.shape))
    want = ref[idx]
    bad = (got != want).any(dim=1)
    count = int(bad.sum())
    if count == 0:
        return
    where = torch.nonzero(bad).flatten()
    places = torch.bincount(idx, minlength=n)
    wrong = torch.bincount(idx[where], minlength=n)
    lines = [f"{what}: {count} of {got.shape[0]} results differ"]
    for i in where[:8].tolist():
        j = int(idx[i])
        lines.append(f"  i = {i}: ray {j}, lane {i % 64}: {_hex(got[i])} for {_hex(want[i])}; "
                     f"ray {j} is wrong in {int(wrong[j])} of its {int(places[j])} places")
    everywhere = int(((wrong == places) & (places > 0)).sum())
    lines.append(f"  {int((wrong > 0).sum())} of {n} referenced rays are wrong somewhere, {everywhere} of them everywhere")
    rows = got[where]
    untouched, zero = int((rows == fill).all(dim=1).sum()), int((rows == 0).all(dim=1).sum())
    lines.append(f"  of the wrong results {untouched} are the fill word (never written), {zero} all zero, "
                 f"{count - untouched - zero} other values")
    lanes = torch.bincount(where % 64, minlength=64)
    lines.append(f"  wrong results per lane 0..63: {lanes.tolist()}")
    pytest.fail("\n".join(lines), pytrace=False)


def tile(N, *base):
    """(idx, tiled tensors): idx[i] = i % n on the device, and base[k][idx] of each numpy array base[k] (n, ...)."""
    n = base[0].shape[0]
    idx = torch.arange(N, device=device()) % n
    out = []
    for a in base:
        a = np.ascontiguousarray(a)
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        out.append(torch.from_numpy(np.array(a)).to(device())[idx].contiguous())
    return (idx, *out)


# ---- 1. ray queries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name,lds,width", [("cornell_mixed", 1, 0), ("blob64x34", 0, 4), ("random_scene", 1, 2)])
def test_ray_queries_over_tiled_rays(pt, name, lds, width, N):
    """LDS scene with spheres; tree top in LDS with the per-lane spill area; spheres only, n = 257."""
    sc, rays, rt, rp = case(name)
    rec = hr.hit_case(name)[6]
    n = rays.shape[0]
    assert_saturating(N, n)
    upload(pt, sc, lds, width)
    t, prim = pt.traceRays(rays)  # the small launch is right: what fails below is the large one's
    assert_same(t, prim, rt, rp, f"{name}: {n} rays")
    what = f"{name} lds={lds} width={width} N={N} n={n}"
    idx, big = tile(N, rays)
    assert_tiled(query("closest", big), ref_words(rt, rp), idx, f"traceRays {what}")
    assert_tiled(query("occluded", big), ref_words(rp >= 0), idx, f"occluded {what}", BYTE_FILL)
    assert_tiled(query("hits", big), ref_words(rec), idx, f"traceHits {what}")
    del idx, big


# ---- 2. path queries -----------------------------------------------------------------------------------------
def check_paths(pt, sc, rays, seeds, rad, segs, lds, width, N, what):
    n = rays.shape[0]
    assert_saturating(N, n)
    upload(pt, sc, lds, width)
    got, gs = pt.traceRadiance(rays, seeds, 8)  # the small launch is right: what fails below is the large one's
    pr.assert_paths(got, gs, rad, segs, f"{what}: {n} rays")
    idx, big, big_seeds = tile(N, rays, seeds)
    assert_tiled(query("radiance", big, big_seeds), ref_words(rad, segs), idx,
                 f"traceRadiance {what} lds={lds} width={width} N={N} n={n}")
    del idx, big, big_seeds


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name,lds,width", [("cornell_mixed", 1, 0), ("blob64x34", 0, 4)])
def test_plain_paths_over_tiled_rays(pt, name, lds, width, N):
    sc, rays, seeds, rad, segs = pr.path_case(name)[:5]
    check_paths(pt, sc, rays, seeds, rad, segs, lds, width, N, name)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name,mode,select,lds,width", [("uneven_lamps", 1, 1, 1, 0), ("uneven_lamps", 2, 1, 1, 0),
                                                        ("blob64x34_lit", 2, 1, 0, 4), ("uneven_lamps", 1, 0, 1, 0)])
def test_light_sampled_paths_over_tiled_rays(pt, name, mode, select, lds, width, N):
    """Light sampling and MIS with the selection by power, in two layouts, and light sampling with the uniform choice."""
    sc, rays, seeds, rad, segs = (sr.case(name, mode) if select else sr.case(name, mode, 0))[:5]  # (as their tests call it)
    sampling(pt, mode, bool(select), on=0)
    check_paths(pt, sc, rays, seeds, rad, segs, lds, width, N, f"{name} mode={mode} select={select}")


@pytest.mark.parametrize("N", SIZES)
def test_paths_under_an_environment_over_tiled_rays(pt, N):
    sc, rays, seeds, rad, segs = want_paths("cornell_mixed", 5)
    pt.setEnvironment(ev.env_of(5))
    check_paths(pt, sc, rays, seeds, rad, segs, 1, 0, N, "cornell_mixed under env_of(5)")


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case_,lds,width", [pytest.param(es.PATH_CASES[1], 1, 0, id=es.case_id(es.PATH_CASES[1])),
                                             pytest.param(es.PATH_CASES[9], 0, 4, id=es.case_id(es.PATH_CASES[9]))])
def test_environment_sampled_paths_over_tiled_rays(pt, case_, lds, width, N):
    """MIS with environment sampling: a scene without lights, and a lit one with the selection by power (the coin)."""
    name, size, kind, select = case_
    sc, E, rays, seeds, rad, segs = es.case(name, 2, size, kind, select)[:6]
    sampling(pt, 2, select)
    pt.setEnvironment(E)
    check_paths(pt, sc, rays, seeds, rad, segs, lds, width, N, f"{es.case_id(case_)} mode 2")


# ---- 3. host-memory rays -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["closest", "radiance"])
def test_host_memory_rays_whole_and_in_slices(pt, kind):
    """The default staging (one launch of N rays, 256 indices a claim) and slices of 300,001 rays, which do not
    divide N: three launches of 64 a claim and a shorter last one."""
    name = "cornell_mixed"
    if kind == "closest":
        sc, rays, rt, rp = case(name)
        seeds, ref = None, ref_words(rt, rp)
    else:
        sc, rays, seeds, rad, segs = pr.path_case(name)[:5]
        ref = ref_words(rad, segs)
    n = rays.shape[0]
    assert_saturating(HOST_N, n)
    assert HOST_N % 300001 != 0 and HOST_N % 300001 < 2 ** 20 <= HOST_N
    upload(pt, sc)
    host_idx = np.arange(HOST_N) % n
    big = np.ascontiguousarray(rays[host_idx])
    big_seeds = None if seeds is None else np.ascontiguousarray(seeds[host_idx])
    idx = torch.from_numpy(host_idx).to(device())
    for qslice in (0, 300001):
        pt.setOption(hippt.OPT_QUERY_SLICE, qslice)
        assert_tiled(query(kind, big, big_seeds), ref, idx, f"{kind} of {HOST_N} host rays, slice {qslice}")
    del idx


# ---- 4. the render route at saturating sizes -----------------------------------------------------------------
def route_scene(pt, which):
    """Sets up the lit scene (MIS, selection by power) or the map-only one (plain paths under env_of(5))."""
    if which == "uneven_lamps":
        sampling(pt, 2, True, on=0)
        return sr.scene_refs("uneven_lamps")[0]
    pt.setEnvironment(ev.env_of(5))
    return scenes.cornell34()


def assert_route(which):
    if which == "uneven_lamps":
        assert info(hippt.INFO_LIGHT_SAMPLING) == 2 and info(hippt.INFO_LIGHT_SELECT) == hippt.LIGHT_SELECT_POWER
    else:
        assert info(hippt.INFO_LIGHT_SAMPLING) == 0 and info(hippt.INFO_ENVIRONMENT) == 5
    assert info(hippt.INFO_CHAIN_CAP) == 0 and info(hippt.INFO_RENDER_PAD) == 0 and info(hippt.INFO_SKY_RECT_PIXELS) == 0


@pytest.mark.parametrize("w,h,chunk", [(1024, 1024, 256), (1000, 1000, 64)])
@pytest.mark.parametrize("which", ["uneven_lamps", "cornell34_env"])
def test_a_saturating_render_is_its_camera_rays_traced(pt, which, w, h, chunk):
    """One frame of w x h pixels; its camera rays through the path query as one launch and as launches of 4,096 rays;
    all three the same bits, with the render's counters."""
    sc = route_scene(pt, which)
    items = w * h
    assert_saturating(items)
    upload(pt, sc, w=w, h=h)
    pt.resetStats()
    assert pt.renderFrames(1, 8), pt.lastError()
    assert info(hippt.INFO_CHUNK) == chunk
    assert_route(which)
    st, shadow = pt.stats(), pt.counters()["shadow_rays"]
    _, acc = pt.readback()  # frame 0 alone: by po_accumulate its average is the sample itself
    rays, seeds = pt.cameraRays(0, device=True)
    assert rays.shape[0] == items
    one = query("radiance", rays, seeds)
    parts = torch.cat([query("radiance", rays[a:a + SMALL], seeds[a:a + SMALL]) for a in range(0, items, SMALL)])
    idx = torch.arange(items, device=device())
    assert_tiled(one, parts, idx, f"{which} {w}x{h}: one launch against launches of {SMALL}")
    rgb = torch.from_numpy(np.ascontiguousarray(acc.reshape(-1, 4)[:, :3])).to(device()).view(torch.int32)
    assert_tiled(rgb, one[:, :3].contiguous(), idx, f"{which} {w}x{h}: the render's accumulation against its rays traced")
    assert st["segments"] == int(one[:, 4].sum()) and st["pixelSamples"] == items
    if which == "uneven_lamps":
        assert 0 < shadow < st["segments"]
    del rays, seeds, one, parts, idx, rgb


# ---- 5. several scratch batches on the render route -----------------------------------------------------------
def frames_per_batch(band_pixels, count, scratch_mb):
    """frames_per_batch() of hippt_api.cpp: the frames whose samples (3 floats a pixel) fit the budget."""
    fpb = max(1, (max(1, scratch_mb) << 20) // (band_pixels * 12))
    return max(1, min(fpb, count, (1 << 31) // max(1, band_pixels)))


def rendered(pt, frames, how, rows, want3, what):
    """Renders `frames` frames in one call or in single asynchronous ones (those compared with the reference's
    image `want3` after 3): (pixel words, accumulation, segments, shadow rays, trace launches)."""
    assert pt.initialize(W, H), pt.lastError()
    pt.resetStats()
    if how == "single":
        for f in range(frames):
            assert pt.renderFramesAsync(1, 8), pt.lastError()
            if f == 2:
                assert pt.synchronize(), pt.lastError()
                assert_image(pt.readback(*rows), want3, f"{what}: the first 3 frames")
        assert pt.synchronize(), pt.lastError()
    else:
        assert pt.renderFrames(frames, 8), pt.lastError()
    px, acc = pt.readback(*rows)
    st = pt.stats()
    assert st["pixelSamples"] == (rows[1] - rows[0]) * W * frames, what
    return px, acc, st["segments"], pt.counters()["shadow_rays"], st["traceLaunches"]


def check_batches(pt, which, rows, frames):
    sc = route_scene(pt, which)
    if which == "uneven_lamps":
        _, acc3, px3, _, _ = sr.render_case("uneven_lamps", 2)
    else:
        _, acc3, px3, _ = want_image(E5)
    want3 = (px3[rows[0]:rows[1]], acc3[rows[0]:rows[1]])
    band = (rows[1] - rows[0]) * W
    default_mb = info(hippt.OPT_SCRATCH_MB)
    first = frames_per_batch(band, frames, 1)
    assert 0 < first <= frames <= 2 * first and frames_per_batch(band, frames, default_mb) == frames
    pt.uploadMesh(sc)
    pt.setRowRange(rows[0], rows[1] if rows != (0, H) else 0)
    pt.setOption(hippt.OPT_SCRATCH_MB, 1)
    split = rendered(pt, frames, "call", rows, want3, f"{which} {first} + {frames - first}")
    assert_route(which)
    pt.setOption(hippt.OPT_SCRATCH_MB, default_mb)
    whole = rendered(pt, frames, "call", rows, want3, f"{which} one batch")
    single = rendered(pt, frames, "single", rows, want3, f"{which} single frames")
    assert (split[4], whole[4], single[4]) == (2 if first < frames else 1, 1, frames)
    for other, name in ((whole, "one batch"), (single, "single frames")):
        assert_image(split[:2], other[:2], f"{which}: {first} + {frames - first} frames against {name}")
        assert split[2:4] == other[2:4], (which, name, split[2:4], other[2:4])
    assert split[2] > 0 and (which != "uneven_lamps" or 0 < split[3] < split[2])
    return first


@pytest.mark.parametrize("which", ["uneven_lamps", "cornell34_env"])
def test_two_scratch_batches_give_one_batchs_image(pt, which):
    """32 x 24, 120 frames under a budget of 1 MiB: 2^20 / (768 x 12) = 113 frames, then 7."""
    assert check_batches(pt, which, (0, H), 120) == 113


@pytest.mark.parametrize("frames", [120, 255])
def test_scratch_batches_of_a_row_band(pt, frames):
    """Rows 0..10 of 32 x 24: 2^20 / (352 x 12) = 248 frames fit a batch.  The 120 frames of the whole image's test
    are one batch here under either budget; 255 frames are 248, then 7."""
    assert check_batches(pt, "uneven_lamps", (0, 11), frames) == min(frames, 248)
