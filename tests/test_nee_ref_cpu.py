"""Light sampling without a GPU: the reference of tests/nee_ref.py is emit_ref.EmitRef with sampling disabled and
path_ref.PathRef over a scene without a light, the GPU tests' ray sets meet every case of the rule often enough
(conditions on the reference alone), and the option's arguments are checked before any device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import emit_ref as er
import hippt
import nee_ref as nr
import path_ref as pr
from hippt import scenes
from test_gpu_ray_query import Ref

F = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hippt.h")


# ---- the reference is pinned -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_without_a_light_it_is_path_ref(name):
    sc, rays, seeds, rad, segs, ends, kinds = pr.path_case(name)
    ref = nr.NeeRef(sc, Ref(sc))
    assert ref.lights == []
    got, gsegs, gends, gkinds, events, shadow = ref.paths_events(rays, seeds, pr.MAX_DEPTH)
    assert got.tobytes() == rad.tobytes() and gsegs.tobytes() == segs.tobytes()
    assert np.array_equal(gends, ends) and np.array_equal(gkinds, kinds)
    assert not events.any() and not shadow.any()


@pytest.mark.parametrize("name", list(er.LIT))
def test_with_sampling_disabled_it_is_emit_ref(name):
    sc, rays, seeds, rad, segs, ends, kinds = er.emit_case(name)[:7]
    ref = nr.NeeRef(sc, Ref(sc), sample=False)
    assert len(ref.lights) == (3 if er.LIT[name][1] else 2) and ref.lights == sorted(ref.lights)
    got, gsegs, gends, gkinds, events, shadow = ref.paths_events(rays, seeds, pr.MAX_DEPTH)
    assert got.tobytes() == rad.tobytes() and gsegs.tobytes() == segs.tobytes()
    assert np.array_equal(gends, ends) and np.array_equal(gkinds, kinds)
    assert not shadow.any() and not (events & ~(nr.LIGHT_SPECULAR)).any()


@pytest.mark.parametrize("name", list(er.LIT))
def test_sampling_changes_paths_only_after_a_lambertian_vertex(name):
    """A path whose vertices are all Metal or Dielectric, or that has none, makes no connection: EmitRef's words."""
    sc, rays, seeds, rad, segs, ends, kinds = er.emit_case(name)[:7]
    _, nrays, nseeds, nrad, nsegs, nends, nkinds, events, shadow = nr.nee_case(name)
    assert nrays.tobytes() == rays.tobytes() and nseeds.tobytes() == seeds.tobytes()
    same = (kinds & (1 << scenes.MAT_LAMBERTIAN)) == 0
    assert same.any() and (~same).any()
    assert nrad[same].tobytes() == rad[same].tobytes() and np.array_equal(nsegs[same], segs[same])
    assert not shadow[same].any()
    # every shadow ray traced is a segment; nothing else is added or lost before the first light sample
    assert np.all(nsegs[~same] >= 1) and int(shadow.sum()) > 1000
    assert np.all(np.isfinite(nrad)) and np.all(nrad >= 0)


# ---- the ray sets of the GPU tests are not vacuous ---------------------------------------------------
@pytest.mark.parametrize("name", list(er.LIT))
def test_fixed_ray_sets_meet_every_case_of_the_rule(name):
    sc, rays, seeds, rad, segs, ends, kinds, events, shadow = nr.nee_case(name)
    assert len(rays) == 4097
    counts = {what: int(np.count_nonzero(events & bit)) for what, bit in nr.EVENTS.items()}
    print(f"{name}: paths with {counts}; shadow rays {int(shadow.sum())} of {int(segs.sum())} segments")
    for what, n in counts.items():
        if what == "far side" and not er.LIT[name][1]:
            assert n == 0 and sc.num_spheres == 0  # no sphere light in the scene
            continue
        assert n >= 10, (what, n)
    # a light met after a Lambertian bounce adds nothing: such a path that made no visible connection is black
    dark = (ends == nr.EMITTED) & ((events & (nr.LIGHT_AFTER_DIFFUSE | nr.VISIBLE)) == nr.LIGHT_AFTER_DIFFUSE)
    # (in the triangles-only scene whatever reaches the lamp by a bounce also saw it from the vertex before)
    assert (dark.any() or not er.LIT[name][1]) and not rad[dark, :3].any()
    # a light met at segment 0 shows its emission itself
    first = (ends == nr.EMITTED) & (segs == 1)
    assert first.any() and np.all(events[first] & nr.LIGHT_SPECULAR) and np.all(rad[first, :3].max(axis=1) >= 4.0)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depth_limits_on_the_reference(depth):
    """maxDepth means what it meant: a connection is made exactly when the next segment would exist."""
    sc, rays, seeds, rad, segs, ends, kinds, events, shadow = nr.nee_case("cornell_mixed_lit", depth)
    erad, esegs = er.emit_case("cornell_mixed_lit", depth)[3:5]
    assert int(shadow.max()) == max(0, depth - 1)
    if depth == 1:  # no vertex scatters: EmitRef's words
        assert rad.tobytes() == erad.tobytes() and segs.tobytes() == esegs.tobytes()
    else:
        assert int(np.count_nonzero(events & nr.VISIBLE)) >= 10 and int(segs.max()) == depth + (depth - 1)


@pytest.mark.parametrize("name", ["cornell34_lit", "cornell_mixed_lit"])
def test_camera_samples_make_connections(name):
    sc, acc, px, total, shadow = nr.render_case(name)
    eacc = er.render_case(name)[1]
    print(f"{name}: 32x24, frames 0..2: {shadow} shadow rays among {total} segments")
    assert shadow >= 1000 and total > shadow and acc.shape == (24, 32, 4) and px.shape == (24, 32)
    assert np.all(acc[..., 3] == 1.0) and np.all(np.isfinite(acc)) and float(acc[..., :3].max()) > 1.0
    # the image is another estimate of the same picture: most pixels differ from the option-off render,
    # and far fewer are black
    assert np.count_nonzero((acc != eacc).any(axis=-1)) > 24 * 32 // 2
    assert np.count_nonzero(~acc[..., :3].any(axis=-1)) < np.count_nonzero(~eacc[..., :3].any(axis=-1)) // 2


# ---- the option ----------------------------------------------------------------------------------------
def test_option_and_info_keys():
    header = open(HEADER).read()
    assert re.search(r"HIPPT_OPT_LIGHT_SAMPLING\s*=\s*37\b", header) and hippt.OPT_LIGHT_SAMPLING == 37
    assert re.search(r"HIPPT_INFO_LIGHTS\s*=\s*107\b", header) and hippt.INFO_LIGHTS == 107
    assert re.search(r"HIPPT_INFO_LIGHT_SAMPLING\s*=\s*108\b", header) and hippt.INFO_LIGHT_SAMPLING == 108
    lib = hippt.load_library()
    lib.cudaPathTracerShutdown()
    assert lib.hipptGetOption(hippt.OPT_LIGHT_SAMPLING) == 0  # the default
    assert lib.hipptSetOption(hippt.OPT_LIGHT_SAMPLING, 1) and lib.hipptGetOption(hippt.OPT_LIGHT_SAMPLING) == 1
    for bad in (-1, 2, 1 << 40):
        assert not lib.hipptSetOption(hippt.OPT_LIGHT_SAMPLING, bad)
        assert lib.hipptGetOption(hippt.OPT_LIGHT_SAMPLING) == 1
    assert lib.hipptSetOption(hippt.OPT_LIGHT_SAMPLING, 0) and lib.hipptGetOption(hippt.OPT_LIGHT_SAMPLING) == 0
    # the facts are read-only
    for key in (hippt.INFO_LIGHTS, hippt.INFO_LIGHT_SAMPLING):
        assert not lib.hipptSetOption(key, 1)
    assert lib.hipptGetOption(hippt.INFO_LIGHT_SAMPLING) == 0


def test_light_count_follows_the_upload_without_a_device():
    lib = hippt.load_library()
    lib.cudaPathTracerShutdown()
    pt = hippt.PathTracer()
    for name, want in (("cornell_mixed_lit", 3), ("cornell34_lit", 3), ("cornell34_lit_tris", 2)):
        pt.uploadMesh(er.lit_scene(name))
        assert lib.hipptGetOption(hippt.INFO_LIGHTS) == want
    pt.uploadMesh(scenes.cornell34())
    assert lib.hipptGetOption(hippt.INFO_LIGHTS) == 0
    # an emissive material that no primitive uses is no light
    sc = er.lit_scene("cornell34_lit_tris")
    sc.tri_mat = np.where(sc.tri_mat == len(sc.materials()) - 1, 0, sc.tri_mat).astype(np.int32)
    pt.uploadMesh(sc)
    assert lib.hipptGetOption(hippt.INFO_LIGHTS) == 0
    # no device was touched: the state is still "not initialized"
    e = ctypes.c_char_p()
    rays, out = np.zeros((1, 8), F), np.zeros((1, 4), F)
    seeds = np.zeros(1, np.uint32)
    assert not lib.hipptTraceRadiance(rays.ctypes.data, seeds.ctypes.data, 1, 8, 0, out.ctypes.data, None, ctypes.byref(e))
    assert b"not initialized" in e.value
    pt.useBuiltinScene(hippt.SCENE_SPHERE4)
    assert lib.hipptGetOption(hippt.INFO_LIGHTS) == 0


def test_cpp_host_knows_the_light_sampling_flag(tmp_path):
    """hippt_render --light-sampling is a flag without a value: the usage text names it, and it does not swallow
    the argument after it."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qt-raytracer_amd", "hippt_render")
    r = subprocess.run([exe, "--no-such-option", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--light-sampling" in r.stderr
    r = subprocess.run([exe, "--light-sampling", "--backend", "none"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2  # "--backend none" was parsed (and rejected), not taken as the flag's value
