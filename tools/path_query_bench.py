#!/usr/bin/env python3
"""Throughput of the path queries (hipptTraceRadiance) on one device, against the renderer's own two code
paths on the same work.  No oracle and no reference tree: it measures, it does not check.

Per scene (a child process of its own, ended after --limit seconds; the tool stops at the first child that
fails): a 1920x1080 image's camera rays and seeds of frame 0 (hipptCameraRays, device memory: 2^21 rays),
then, alternating call by call so that clock and thermal drift fall on all alike,
  path_query   hipptTraceRadiance of those rays at depth 8 (HIPPT_RAYS_DEVICE): segments = the sum of
               its `segments` output
  megakernel   hipptRenderFrames(0, 1) after a hipptResetAccumulation, no host copy: segments from
               hipptGetStats
  wavefront    the same under HIPPT_OPT_PATH_MODE 1
each timed by a host clock around the blocking call (launch and wait included, as a caller sees it), after
--warmup untimed rounds.  Reports segments/s of the median of --runs calls.  The three trace the same
2^21 paths, so their segment counts agree; the render calls also accumulate and tonemap the image.

Writes <out>/<scene>.json and prints one summary line per scene.

--thresholds=-1,63,48,32,16,0: instead, hipptTraceRadiance alone on the same rays under each
HIPPT_OPT_WAVE_THRESHOLD value (lanes still traversing at or below which a wave leaves the traversal loop
and shades its finished lanes: 63 = whenever a lane has finished, 0 = only when all have, -1 = the plan's),
alternating call by call, every result compared bit for bit with the first; writes
<out>/wave_threshold.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, DEPTH = 1920, 1080, 8


def child(args):
    import torch  # before libhippt.so is loaded: one HIP runtime for both
    sys.path.insert(0, os.path.join(REPO, "qt-raytracer_amd"))
    import hippt
    from hippt import scenes

    sc = scenes.get_scene(args.scene)
    pt = hippt.PathTracer()
    pt.setDevices([args.device])
    pt.uploadMesh(sc)
    if not pt.initialize(W, H):
        raise SystemExit(pt.lastError())
    dev = torch.device("cuda", args.device)
    rays, seeds = pt.cameraRays(0, device=True)
    torch.cuda.synchronize(dev)
    n = int(rays.shape[0])
    last = {}

    def path_query():
        t0 = time.perf_counter()
        _, segs = pt.traceRadiance(rays, seeds, DEPTH)
        dt = time.perf_counter() - t0
        last["path_query"] = int(segs.sum(dtype=torch.int64))
        return dt

    def render(mode):
        def call():
            pt.setOption(hippt.OPT_PATH_MODE, mode)
            if not pt.resetAccumulation():
                raise SystemExit(pt.lastError())
            pt.resetStats()
            t0 = time.perf_counter()
            ok = pt.renderFrames(1, DEPTH, copy=False)
            dt = time.perf_counter() - t0
            if not ok:
                raise SystemExit(pt.lastError())
            last["megakernel" if mode == 0 else "wavefront"] = int(pt.stats()["segments"])
            return dt
        return call

    calls = (("path_query", path_query), ("megakernel", render(0)), ("wavefront", render(1)))
    for _ in range(args.warmup):
        for _, c in calls:
            c()
    ms = {name: [] for name, _ in calls}
    for _ in range(args.runs):
        for name, c in calls:
            ms[name].append(c() * 1e3)
    pt.setOption(hippt.OPT_PATH_MODE, 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"scene": args.scene, "primitives": sc.num_tris + sc.num_spheres, "width": W, "height": H, "rays": n,
           "max_depth": DEPTH, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(dev),
           "order": "path_query, megakernel, wavefront alternating per call",
           "segments": dict(last), "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "median_ms": {k: round(v, 4) for k, v in med.items()},
           "gsegments_per_s": {k: round(last[k] / med[k] / 1e6, 3) for k in med}}
    hippt.load_library().cudaPathTracerShutdown()
    print(json.dumps(out))


def thresholds_child(args):
    import torch  # before libhippt.so is loaded: one HIP runtime for both
    sys.path.insert(0, os.path.join(REPO, "qt-raytracer_amd"))
    import hippt
    from hippt import scenes

    values = [int(t) for t in args.thresholds.split(",")]
    sc = scenes.get_scene(args.scene)
    pt = hippt.PathTracer()
    pt.setDevices([args.device])
    pt.uploadMesh(sc)
    if not pt.initialize(W, H):
        raise SystemExit(pt.lastError())
    rays, seeds = pt.cameraRays(0, device=True)
    ms = {t: [] for t in values}
    ref = None
    for rnd in range(args.warmup + args.runs):
        for t in values:
            pt.setOption(hippt.OPT_WAVE_THRESHOLD, t)
            t0 = time.perf_counter()
            rad, segs = pt.traceRadiance(rays, seeds, DEPTH)
            dt = time.perf_counter() - t0
            if ref is None:
                ref = (rad.clone(), segs.clone())
            if not (torch.equal(rad.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(segs, ref[1])):
                raise SystemExit(f"{args.scene}: the result changed at threshold {t}")
            if rnd >= args.warmup:
                ms[t].append(dt * 1e3)
    pt.setOption(hippt.OPT_WAVE_THRESHOLD, -1)
    nseg = int(ref[1].sum(dtype=torch.int64))
    med = {t: statistics.median(v) for t, v in ms.items()}
    out = {"scene": args.scene, "segments": nseg, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(torch.device("cuda", args.device)),
           "median_ms": {str(t): round(v, 4) for t, v in med.items()},
           "min_ms": {str(t): round(min(v), 4) for t, v in ms.items()},
           "gsegments_per_s": {str(t): round(nseg / v / 1e6, 3) for t, v in med.items()}}
    hippt.load_library().cudaPathTracerShutdown()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell34,blob70k,random_scene")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a scene's child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "path_query"))
    ap.add_argument("--thresholds", help="comma-separated HIPPT_OPT_WAVE_THRESHOLD values: the path query alone under each")
    ap.add_argument("--scene", help=argparse.SUPPRESS)  # the child's
    args = ap.parse_args()
    if args.scene:
        return thresholds_child(args) if args.thresholds else child(args)
    os.makedirs(args.out, exist_ok=True)
    sweep = {}
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", name, "--device", str(args.device), "--warmup",
               str(args.warmup), "--runs", str(args.runs)] + (["--thresholds=" + args.thresholds] if args.thresholds else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {args.limit:.0f} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"{name}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if args.thresholds:
            sweep[name] = res
            print(f"{name:13s} " + "  ".join(f"{t}: {g:.3f}" for t, g in res["gsegments_per_s"].items()) + "  Gseg/s", flush=True)
            continue
        with open(os.path.join(args.out, f"{name}.json"), "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")
        g, m = res["gsegments_per_s"], res["median_ms"]
        print(f"{name:13s} " + "  ".join(f"{k} {m[k]:8.3f} ms {g[k]:7.3f} Gseg/s" for k in g), flush=True)
    if args.thresholds:
        with open(os.path.join(args.out, "wave_threshold.json"), "w") as fo:
            json.dump({"what": "hipptTraceRadiance, 1920x1080 camera rays of frame 0, depth 8, by HIPPT_OPT_WAVE_THRESHOLD; "
                               "alternating per call", "results": sweep}, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
