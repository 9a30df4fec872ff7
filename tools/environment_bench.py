#!/usr/bin/env python3
"""What an environment map (hipptSetEnvironment) costs per frame, on one device.  No oracle and no reference tree:
it measures, it does not check.

Per scene of hippt.scenes.SCENES (a child process of its own, ended after --limit seconds; the tool stops at the
first child that fails), at 1920x1080 and depth 8, for each entry n of --spp (default 1,64):
  frame time   hipptRenderFrames of n frames from an empty accumulation with no host copy, under
               hippt.scenes.sun_sky(--size) (the ray-per-lane route: a path kernel launch over the camera's
               samples) and with the environment removed (the sky gradient: the render megakernel), alternating
               call by call after --warmup untimed rounds, each timed by a host clock around the blocking call;
               the median of --runs calls, every call's figure kept
  segments     per call from hipptGetStats (the paths are the same paths: the counts must agree)
  set time     hipptSetEnvironment of the map (same size as the one before: validation, the host copy, one
               staged copy per context), host clock, the median of --runs calls

With --env-sampling 0,1 it measures instead what HIPPT_OPT_ENV_SAMPLING buys under HIPPT_LIGHT_SAMPLING_MIS and the same
map: 1-frame calls with the option 0 and 1 alternating call by call (the median of --runs), and the mean squared
error of both against the tool's own --reference-spp image with the option off, at each entry of --frames and, for
the option on, at the frames that take the option-off frames' time.

Writes <out>/environment_<scene>.json (env_sampling_<scene>.json) and prints one summary line per scene."""
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
    import torch  # noqa: F401 (before libhippt.so is loaded: one HIP runtime for both)
    sys.path.insert(0, os.path.join(REPO, "qt-raytracer_amd"))
    import hippt
    from hippt import scenes

    sc = scenes.get_scene(args.scene)
    env = scenes.sun_sky(args.size, sun_radiance=args.sun_radiance, sun_cos=args.sun_cos)
    pt = hippt.PathTracer()
    pt.setDevices([args.device])
    pt.uploadMesh(sc) if sc.lambertian_triangles else pt.uploadScene(sc)
    if not pt.initialize(W, H):
        raise SystemExit(pt.lastError())
    lib = hippt.load_library()

    def render(on, frames):
        """(seconds, segments) of `frames` frames from an empty accumulation."""
        pt.setEnvironment(env if on else None)
        if not pt.resetAccumulation() or not pt.synchronize():
            raise SystemExit(pt.lastError())
        pt.resetStats()
        t0 = time.perf_counter()
        ok = pt.renderFrames(frames, DEPTH, copy=False)
        dt = time.perf_counter() - t0
        if not ok:
            raise SystemExit(pt.lastError())
        if int(lib.hipptGetOption(hippt.INFO_ENVIRONMENT)) != (args.size if on else 0):
            raise SystemExit(f"{args.scene}: the render did not take the route asked for")
        return dt, int(pt.counters()["segments"])

    if args.env_sampling:
        return child_env_sampling(args, pt, hippt, env)
    result = {"scene": args.scene, "size": args.size, "width": W, "height": H, "depth": DEPTH, "frames": {}}
    for n in [int(x) for x in args.spp.split(",")]:
        for _ in range(args.warmup):
            for on in (0, 1):
                render(on, n)
        ms, segs = {0: [], 1: []}, {}
        for _ in range(args.runs):
            for on in (0, 1):
                dt, segs[on] = render(on, n)
                ms[on].append(round(dt * 1e3, 4))
        med = {on: statistics.median(v) for on, v in ms.items()}
        result["frames"][str(n)] = {"gradient_ms": ms[0], "environment_ms": ms[1], "gradient_median_ms": med[0],
                                    "environment_median_ms": med[1], "ratio": round(med[1] / med[0], 4),
                                    "gradient_segments": segs[0], "environment_segments": segs[1]}
    pt.setEnvironment(env)
    sets = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        pt.setEnvironment(env)
        sets.append(round((time.perf_counter() - t0) * 1e3, 4))
    pt.synchronize()
    result["set_ms"] = sets
    result["set_median_ms"] = statistics.median(sets)
    pt.setEnvironment(None)
    print(json.dumps(result))


def child_env_sampling(args, pt, hippt, env):
    import numpy as np
    lib = hippt.load_library()
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, hippt.LIGHT_SAMPLING_MIS)
    pt.setEnvironment(env)

    def render(on, frames, timed=False):
        """(seconds, image (H, W, 3) float64) of `frames` frames from an empty accumulation."""
        pt.setOption(hippt.OPT_ENV_SAMPLING, on)
        if not pt.resetAccumulation() or not pt.synchronize():
            raise SystemExit(pt.lastError())
        t0 = time.perf_counter()
        done = 0
        while done < frames:
            n = min(256, frames - done)
            if not pt.renderFrames(n, DEPTH, copy=False):
                raise SystemExit(pt.lastError())
            done += n
        dt = time.perf_counter() - t0
        if int(lib.hipptGetOption(hippt.INFO_ENV_SAMPLING)) != on:
            raise SystemExit(f"{args.scene}: the render did not apply the option as asked")
        return dt, (None if timed else pt.readback()[1][..., :3].astype(np.float64))

    for _ in range(args.warmup):
        for on in (0, 1):
            render(on, 1, True)
    ms = {0: [], 1: []}
    for _ in range(args.runs):
        for on in (0, 1):
            ms[on].append(round(render(on, 1, True)[0] * 1e3, 4))
    med = {on: statistics.median(v) for on, v in ms.items()}
    ref = render(0, args.reference_spp)[1]
    result = {"scene": args.scene, "size": args.size, "sun_radiance": args.sun_radiance, "sun_cos": args.sun_cos,
              "sun_texels": int((env[..., 0] > 0.5 * args.sun_radiance).sum()),
              "width": W, "height": H, "depth": DEPTH, "mode": 2,
              "reference_spp": args.reference_spp, "ms": {str(k): v for k, v in ms.items()},
              "median_ms": {str(k): v for k, v in med.items()}, "mse": {}}
    for n in [int(x) for x in args.frames.split(",")]:
        equal = max(1, int(n * med[0] / med[1]))
        row = {"0": float(((render(0, n)[1] - ref) ** 2).mean()), "1": float(((render(1, n)[1] - ref) ** 2).mean()),
               "equal_time_frames": equal}
        row["1_at_equal_time"] = row["1"] if equal == n else float(((render(1, equal)[1] - ref) ** 2).mean())
        result["mse"][str(n)] = row
    pt.setOption(hippt.OPT_ENV_SAMPLING, 0)
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 0)
    pt.setEnvironment(None)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell34,blob70k")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", default="1,64")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--limit", type=int, default=240, help="seconds per scene")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "environment"))
    ap.add_argument("--env-sampling", default="", help="0,1: HIPPT_OPT_ENV_SAMPLING off against on under MIS")
    ap.add_argument("--sun-radiance", type=float, default=60.0, help="hippt.scenes.sun_sky's sun_radiance")
    ap.add_argument("--sun-cos", type=float, default=0.995, help="hippt.scenes.sun_sky's sun_cos (the disc's half angle)")
    ap.add_argument("--frames", default="1,4,16,64", help="with --env-sampling: frames at which the error is taken")
    ap.add_argument("--reference-spp", type=int, default=16384)
    ap.add_argument("--scene", default=None, help=argparse.SUPPRESS)  # the child's
    args = ap.parse_args()
    if args.scene:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", name, "--size", str(args.size), "--spp", args.spp,
               "--runs", str(args.runs), "--warmup", str(args.warmup), "--device", str(args.device),
               "--sun-radiance", str(args.sun_radiance), "--sun-cos", str(args.sun_cos)]
        if args.env_sampling:
            if args.env_sampling != "0,1":
                raise SystemExit("--env-sampling takes 0,1")
            cmd += ["--env-sampling", "0,1", "--frames", args.frames, "--reference-spp", str(args.reference_spp)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{name}: the child failed ({r.returncode})")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if args.env_sampling:
            with open(os.path.join(args.out, f"env_sampling_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)
            print(name, "ms per frame", res["median_ms"], "mse", res["mse"], flush=True)
            continue
        with open(os.path.join(args.out, f"environment_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(name, {n: (v["gradient_median_ms"], v["environment_median_ms"], v["ratio"]) for n, v in res["frames"].items()},
              "set", res["set_median_ms"], flush=True)


if __name__ == "__main__":
    main()
