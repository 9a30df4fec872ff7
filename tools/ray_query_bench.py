#!/usr/bin/env python3
"""Throughput of the batched ray queries (hipptTraceRays / hipptOccluded / hipptTraceCamera) on
device-resident rays: G rays/s per scene, ray set and query kind.

Ray sets (2^24 rays each by default): `camera`, the pinhole rays through the pixel centres of a
4096 x 4096 image of the scene's camera, in image order (coherent); `inbox`, origins uniform in the
scene's box with uniform random directions (incoherent).  `camera_kernel` is hipptTraceCamera on the
same image: the rays generated in the kernel, no ray buffer read.

Each figure: warm-up calls, then the median of --runs calls, each a host clock around the blocking
call (so it includes the launch and the wait, as a caller sees it).  Writes one JSON file per scene
into --out and prints one summary line per measurement.

--hits: hit records against the closest-hit query they extend.  In one process, on the same rays,
hipptTraceRays and hipptTraceHits alternate call by call (so that clock and thermal drift fall on both
alike); per ray set the median of --runs calls of each and the ratio traceHits / traceRays of the
medians, written to profiles/hit_records/ unless --out says otherwise."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before libhippt.so is loaded: one HIP runtime for both

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qt-raytracer_amd"))

import hippt  # noqa: E402
from hippt import scenes  # noqa: E402


def camera_rays(sc, side):
    cam = hippt.build_camera(sc.lookfrom, sc.lookat, sc.vup, sc.vfov, 1.0, 0.0, sc.focus)
    org, llc = np.array(cam.origin[:], np.float32), np.array(cam.llc[:], np.float32)
    hor, ver = np.array(cam.horizontal[:], np.float32), np.array(cam.vertical[:], np.float32)
    u = ((np.arange(side, dtype=np.float32) + 0.5) / np.float32(side - 1))
    rays = np.empty((side, side, 8), np.float32)
    rays[..., 0:3] = org
    rays[..., 3] = 0.001
    rays[..., 4:7] = llc + u[None, :, None] * hor + u[:, None, None] * ver - org
    rays[..., 7] = np.inf
    return rays.reshape(-1, 8)


def inbox_rays(sc, n, seed=3):
    rng = np.random.default_rng(seed)
    v = np.asarray(sc.verts, np.float32).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(lo, hi, size=(n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3] = 0.001
    rays[:, 7] = np.inf
    return rays


def timed(call, warmup, runs):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def alternated(calls, warmup, runs):
    """{name: [ms]}: `runs` rounds, each timing every call once, in the order given."""
    for _ in range(warmup):
        for _, call in calls:
            call()
    ms = {name: [] for name, _ in calls}
    for _ in range(runs):
        for name, call in calls:
            t0 = time.perf_counter()
            call()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def hits_mode(args, lib, dev, n):
    for name in args.scenes.split(","):
        sc = scenes.get_scene(name)
        pt = hippt.PathTracer()
        pt.setDevices([args.device])
        pt.uploadMesh(sc)
        if not pt.initialize(args.side, args.side):
            raise SystemExit(pt.lastError())
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
        e = ctypes.c_char_p()
        rows = []

        def check(ok):
            if not ok:
                raise SystemExit(e.value.decode() if e.value else "query failed")

        for rayset, make in (("camera", lambda: camera_rays(sc, args.side)), ("inbox", lambda: inbox_rays(sc, n))):
            rays = torch.from_numpy(make()).to(dev)
            torch.cuda.synchronize(dev)
            ms = alternated((
                ("traceRays", lambda: check(lib.hipptTraceRays(rays.data_ptr(), n, hippt.RAYS_DEVICE, t.data_ptr(),
                                                               prim.data_ptr(), ctypes.byref(e)))),
                ("traceHits", lambda: check(lib.hipptTraceHits(rays.data_ptr(), n, hippt.RAYS_DEVICE, hits.data_ptr(),
                                                               ctypes.byref(e))))), args.warmup, args.runs)
            f = hippt.split_hits(hits)
            if not (torch.equal(f["prim"], prim) and torch.equal(f["t"].view(torch.int32), t.view(torch.int32))):
                raise SystemExit(f"{name} {rayset}: traceHits and traceRays disagree")
            med = {k: statistics.median(v) for k, v in ms.items()}
            rows.append({"rays": rayset, "n": n, "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                         "median_ms": {k: round(v, 4) for k, v in med.items()},
                         "grays_per_s": {k: round(n / v / 1e6, 3) for k, v in med.items()},
                         "ratio_hits_over_rays": round(med["traceHits"] / med["traceRays"], 4),
                         "hit_share": round(int((prim >= 0).sum()) / n, 4),
                         "backface_share": round(int((f["matFlags"] < 0).logical_and(prim >= 0).sum()) / n, 4)})
            del rays, f
        out = {"scene": name, "triangles": sc.num_tris, "side": args.side, "warmup": args.warmup, "runs": args.runs,
               "device": torch.cuda.get_device_name(dev), "order": "traceRays, traceHits alternating per call",
               "lds_scene": bool(lib.hipptGetOption(hippt.OPT_LDS_SCENE)), "results": rows}
        with open(os.path.join(args.out, f"{name}.json"), "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")
        for r in rows:
            print(f"{name:10s} {r['rays']:7s} traceRays {r['median_ms']['traceRays']:8.3f} ms "
                  f"{r['grays_per_s']['traceRays']:7.3f} G/s  traceHits {r['median_ms']['traceHits']:8.3f} ms "
                  f"{r['grays_per_s']['traceHits']:7.3f} G/s  ratio {r['ratio_hits_over_rays']:.3f}", flush=True)
        del pt, t, prim, hits
        lib.cudaPathTracerShutdown()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell34,blob70k")
    ap.add_argument("--side", type=int, default=4096, help="camera image side; rays = side^2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hits", action="store_true", help="traceHits against traceRays, alternating (see above)")
    ap.add_argument("--out", default=None, help="default profiles/ray_query, with --hits profiles/hit_records")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "hit_records" if args.hits else "ray_query")
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible to torch")
    os.makedirs(args.out, exist_ok=True)
    lib = hippt.load_library()
    dev = torch.device("cuda", args.device)
    n = args.side * args.side
    if args.hits:
        return hits_mode(args, lib, dev, n)
    for name in args.scenes.split(","):
        sc = scenes.get_scene(name)
        pt = hippt.PathTracer()
        pt.setDevices([args.device])
        pt.uploadMesh(sc)
        if not pt.initialize(args.side, args.side):
            raise SystemExit(pt.lastError())
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        e = ctypes.c_char_p()
        rows = []

        def check(ok):
            if not ok:
                raise SystemExit(e.value.decode() if e.value else "query failed")

        for rayset, make in (("camera", lambda: camera_rays(sc, args.side)), ("inbox", lambda: inbox_rays(sc, n))):
            rays = torch.from_numpy(make()).to(dev)
            torch.cuda.synchronize(dev)
            for kind, call in (
                    ("closest", lambda: check(lib.hipptTraceRays(rays.data_ptr(), n, hippt.RAYS_DEVICE, t.data_ptr(),
                                                                 prim.data_ptr(), ctypes.byref(e)))),
                    ("occluded", lambda: check(lib.hipptOccluded(rays.data_ptr(), n, hippt.RAYS_DEVICE, occ.data_ptr(),
                                                                 ctypes.byref(e))))):
                ms = timed(call, args.warmup, args.runs)
                hits = int((prim >= 0).sum()) if kind == "closest" else int(occ.sum())
                rows.append({"rays": rayset, "query": kind, "n": n, "ms": [round(x, 4) for x in ms],
                             "median_ms": round(statistics.median(ms), 4),
                             "grays_per_s": round(n / statistics.median(ms) / 1e6, 3), "hit_share": round(hits / n, 4)})
            del rays
        ms = timed(lambda: check(lib.hipptTraceCamera(0, hippt.RAYS_DEVICE, t.data_ptr(), prim.data_ptr(),
                                                      ctypes.byref(e))), args.warmup, args.runs)
        rows.append({"rays": "camera_kernel", "query": "closest", "n": n, "ms": [round(x, 4) for x in ms],
                     "median_ms": round(statistics.median(ms), 4),
                     "grays_per_s": round(n / statistics.median(ms) / 1e6, 3),
                     "hit_share": round(int((prim >= 0).sum()) / n, 4)})
        out = {"scene": name, "triangles": sc.num_tris, "side": args.side, "warmup": args.warmup, "runs": args.runs,
               "device": torch.cuda.get_device_name(dev), "bvh_width": 4,
               "lds_scene": bool(lib.hipptGetOption(hippt.OPT_LDS_SCENE)), "results": rows}
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        for r in rows:
            print(f"{name:10s} {r['rays']:13s} {r['query']:8s} {r['median_ms']:9.3f} ms  {r['grays_per_s']:8.3f} G rays/s  "
                  f"hits {r['hit_share']:.3f}", flush=True)
        del pt
        lib.cudaPathTracerShutdown()


if __name__ == "__main__":
    main()
