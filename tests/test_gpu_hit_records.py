"""Hit records (GPU): hipptTraceHits and hipptTraceCameraHits against the reference of tests/hit_ref.py
(pinned to the oracle by tests/test_hit_records_cpu.py), all 8 words of every record bit for bit.

The scenes, rays and (t, prim) references are those of test_gpu_ray_query.case; the records on top
of them are computed once per scene (hit_ref.hit_case) and shared by the tests."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch  # before libhippt.so is loaded: both then share one HIP runtime (PathTracer.traceRays)

import chain_audit
import hippt
import pyoracle as po
from hit_ref import HitRef, assert_records, hit_case
from refit_util import verts_of, with_verts, wobble
from test_gpu_ray_query import N, Ref, camera_rays, degenerate_rays, pt, upload  # noqa: F401 (pt: the fixture)

pytestmark = pytest.mark.gpu

MISS = np.array([(np.inf, -1, (0.0, 0.0, 0.0), 0.0, 0.0, -1)], hippt.HIT_DTYPE)


# ---- 1. parity with the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("width", [0, 2])
@pytest.mark.parametrize("name,lds", [("cornell34", 1), ("cornell_mixed", 1), ("blob64x34", 0), ("random_scene", 1)])
def test_records_match_reference(pt, name, lds, width):
    sc, rays, rt, rp, _, _, rec = hit_case(name)
    upload(pt, sc, lds, width)
    sizes = (1, 63, 65, N) if rays.shape[0] == N else (rays.shape[0],)
    for n in sizes:
        hits = pt.traceHits(np.ascontiguousarray(rays[:n]))
        assert hits.shape == (n,)
        assert_records(hits, rec[:n], f"{name} n={n}")
        # words 0-1 are traceRays' bytes on the same batch
        t, prim = pt.traceRays(np.ascontiguousarray(rays[:n]))
        assert hits["t"].tobytes() == t.tobytes() and hits["prim"].tobytes() == prim.tobytes(), f"{name} n={n}"
    if rays.shape[0] == N:  # the degenerate rays at the tail: miss records
        tail = hits[N - degenerate_rays().shape[0]:]
        assert tail.tobytes() == np.repeat(MISS, tail.size).tobytes()


# ---- 2. camera records and guide buffers ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell34", "cornell_mixed"])
def test_camera_records_and_gbuffer(pt, name):
    w, h = 64, 48
    sc = hit_case(name)[0]
    if name == "cornell_mixed":
        sc = dataclasses.replace(sc, aperture=12.0, focus=900.0)  # a thin lens
    upload(pt, sc, w=w, h=h)
    ref = Ref(sc)
    href = HitRef(sc, ref)
    albedo = np.asarray(sc.albedo, np.float32).reshape(-1, 3)
    for frame in (0, 3):
        rays = camera_rays(sc, w, h, frame)
        rt, rp = ref.closest(rays)
        rec = href.records(rays, rt, rp)
        hits = pt.traceCameraHits(frame)
        assert hits.shape == (h, w)
        assert_records(hits, rec, f"{name} frame {frame}")
        g = pt.gbuffer(frame)
        hit = (rp >= 0).reshape(h, w)
        mat = np.where(hit, rec["matFlags"].reshape(h, w) & hippt.HIT_MATERIAL_MASK, -1)
        want = np.zeros((h, w, 3), np.float32)
        want[hit] = albedo[mat[hit]]
        assert g["albedo"].dtype == np.float32 and g["albedo"].tobytes() == want.tobytes()
        assert np.array_equal(g["material"], mat) and np.array_equal(g["prim"], rp.reshape(h, w))
        assert g["depth"].tobytes() == rt.tobytes() and np.all(np.isinf(g["depth"][~hit]))
        assert g["normal"].tobytes() == rec["normal"].tobytes()
        for x, y in ((0, 0), (w - 1, h - 1), (w // 2, h // 2), (7, 19)):
            p, r = pt.pickHit(x, y, frame), rec[y * w + x]
            assert (p["prim"], p["t"], p["u"], p["v"]) == (int(r["prim"]), float(r["t"]), float(r["u"]), float(r["v"]))
            assert p["normal"] == tuple(float(c) for c in r["normal"])
            assert p["material"] == int(mat[y, x]) and p["backface"] == (p["prim"] >= 0 and int(r["matFlags"]) < 0)
            assert p["sphere"] == (p["prim"] >= ref.ntris)
            assert pt.pick(x, y, frame) == (p["prim"], p["t"])


# ---- 3. slicing ----------------------------------------------------------------------------------------
def test_slices_give_the_same_bytes(pt):
    sc, rays, _, _, _, _, rec = hit_case("cornell_mixed")
    upload(pt, sc)
    whole = pt.traceHits(rays)
    pt.setOption(hippt.OPT_QUERY_SLICE, 64)
    sliced = pt.traceHits(rays)
    assert sliced.tobytes() == whole.tobytes()
    assert_records(sliced, rec, "slice 64")


# ---- 4. device memory ----------------------------------------------------------------------------------
def test_device_tensors(pt):
    assert torch.cuda.is_available()
    sc, rays, _, _, _, _, rec = hit_case("cornell_mixed")
    pt.setDevices([0])
    upload(pt, sc)
    host = pt.traceHits(rays)
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(np.array(rays)).to(dev)
    hits = pt.traceHits(dr)
    assert hits.device == dr.device and hits.dtype == torch.float32 and tuple(hits.shape) == (N, 8)
    assert hits.cpu().numpy().tobytes() == host.tobytes() == rec.tobytes()
    f = hippt.split_hits(hits)
    assert f["prim"].dtype == torch.int32 and np.array_equal(f["prim"].cpu().numpy(), rec["prim"])
    assert np.array_equal(f["matFlags"].cpu().numpy(), rec["matFlags"])
    assert f["normal"].cpu().numpy().tobytes() == rec["normal"].tobytes()
    assert f["t"].data_ptr() == hits.data_ptr()  # views, not copies
    # a record buffer that is not 32-byte aligned, or not device memory, or on another device
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    buf = torch.empty(8 * N + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 32 == 0
    assert not lib.hipptTraceHits(dr.data_ptr(), N, hippt.RAYS_DEVICE, buf.data_ptr() + 16, ctypes.byref(e))
    assert b"misaligned" in e.value
    h0 = np.empty(N, hippt.HIT_DTYPE)
    assert not lib.hipptTraceHits(dr.data_ptr(), N, hippt.RAYS_DEVICE, h0.ctypes.data, ctypes.byref(e))
    assert b"device memory" in e.value
    if torch.cuda.device_count() > 1:
        other = torch.empty(8 * N, dtype=torch.float32, device=torch.device("cuda", 1))
        assert not lib.hipptTraceHits(dr.data_ptr(), N, hippt.RAYS_DEVICE, other.data_ptr(), ctypes.byref(e))
        assert b"different devices" in e.value
        del other
    assert lib.hipptTraceHits(dr.data_ptr(), N, hippt.RAYS_DEVICE, buf.data_ptr(), ctypes.byref(e)), e.value
    assert buf[:8 * N].cpu().numpy().tobytes() == rec.tobytes()
    del dr, hits, buf, f


# ---- 5. animated mesh ----------------------------------------------------------------------------------
def test_records_follow_a_vertex_update(pt):
    sc, rays, _, _, _, _, rec0 = hit_case("cornell34")
    rays = np.ascontiguousarray(rays[:N - degenerate_rays().shape[0]])
    upload(pt, sc)
    v1 = wobble(verts_of(sc))
    pt.updateVertices(v1)
    sc1 = with_verts(sc, v1)
    ref = Ref(sc1)
    rt, rp = ref.closest(rays)
    rec = HitRef(sc1, ref).records(rays, rt, rp)
    # a condition on the reference alone (3763 of the 4083 rays): the update changes the normal most rays
    # report, so records that match are read from the refitted shade records
    moved = np.count_nonzero((rec["normal"] != rec0["normal"][:len(rays)]).any(axis=1))
    assert moved > len(rays) // 2, moved
    assert_records(pt.traceHits(rays), rec, "after updateVertices")


# ---- 6. queries do not disturb rendering ---------------------------------------------------------------
def test_hit_query_between_async_frames_leaves_the_image_alone(pt):
    w, h = 45, 26
    sc, rays, _, _, _, _, rec = hit_case("cornell34")
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 1)
    hippt.chain_audit()  # (drops records of earlier tests)
    upload(pt, sc, w=w, h=h)
    pt.resetStats()
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    hits = pt.traceHits(rays)
    for _ in range(3):
        assert pt.renderFramesAsync(1, 8), pt.lastError()
    assert pt.synchronize(), pt.lastError()
    px, acc = pt.readback()
    runs = hippt.chain_audit()
    pt.setOption(hippt.OPT_CHAIN_AUDIT, 0)
    assert_records(hits, rec)
    opx, oacc, segs, _ = po.MeshScene(sc, w, h).frames(0, 6, 8)
    assert np.array_equal(px, opx) and acc.tobytes() == oacc.tobytes()
    problems = chain_audit.check(runs)
    assert not problems, problems[:6]
    assert pt.stats()["segments"] == segs  # queries add nothing
