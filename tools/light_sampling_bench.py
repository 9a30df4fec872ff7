#!/usr/bin/env python3
"""What light sampling (HIPPT_OPT_LIGHT_SAMPLING) costs per frame and buys per unit of time, on one device.  No
oracle and no reference tree: it measures, it does not check.

Per scene (hippt.scenes.cornell_lit of a base scene, or for a name BASE_lamps hippt.scenes.cornell_lamps of BASE; a
child process of its own, ended after --limit seconds; the tool stops at the first child that fails), at 1920x1080
and depth 8:
  frame time    hipptRenderFrames(f, 1) with no host copy, the option off (the render megakernel), on (the
                light-sampling route) and, with --modes 0,1,2 (the default), with MIS (HIPPT_LIGHT_SAMPLING_MIS, the
                same route), alternating call by call after --warmup untimed rounds, each timed by a host clock
                around the blocking call; the median of --runs calls
  segments      per frame from hipptGetStats, and with the option on the shadow rays among them (counter 27)
  equal time    a reference image of --ref-spp samples with the option off; then, per entry n of --spp, n frames
                with the option on and as many frames with it off as take the same time (n * ms_on / ms_off,
                rounded, at least 1) and n frames with MIS, each from an empty accumulation, timed again; the mean squared error of
                the accumulated rgb against the reference, the same without the 0.1 % of pixels that err most, and
                the largest absolute error of a channel.  The reference holds the option-off render's own
                samples (frames 0..): a share of n / ref-spp of it.
  light choice  with --select 0,1: under MIS, HIPPT_OPT_LIGHT_SELECT 0 (uniform) against 1 (by power): the frame time
                of each, alternating call by call as above, and per entry n of --spp the errors above of n frames
                with the first value against as many frames with each other value as take the same time, all
                against the same option-off reference image ("select" in the result).

Writes <out>/<base>.json and prints one summary line per scene."""
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
    import numpy as np
    import torch  # before libhippt.so is loaded: one HIP runtime for both
    sys.path.insert(0, os.path.join(REPO, "qt-raytracer_amd"))
    import hippt
    from hippt import scenes

    lamps = args.scene.endswith("_lamps")
    sc = scenes.cornell_lamps(args.scene[:-len("_lamps")]) if lamps else scenes.cornell_lit(args.scene)
    pt = hippt.PathTracer()
    pt.setDevices([args.device])
    pt.uploadMesh(sc)
    if not pt.initialize(W, H):
        raise SystemExit(pt.lastError())
    lib = hippt.load_library()

    def render(on, frames):
        """(seconds, segments, shadow rays) of `frames` frames from an empty accumulation."""
        pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, on)
        if not pt.resetAccumulation():
            raise SystemExit(pt.lastError())
        pt.resetStats()
        t0 = time.perf_counter()
        ok = pt.renderFrames(frames, DEPTH, copy=False)
        dt = time.perf_counter() - t0
        if not ok:
            raise SystemExit(pt.lastError())
        c = pt.counters()
        if int(lib.hipptGetOption(hippt.INFO_LIGHT_SAMPLING)) != on:
            raise SystemExit(f"{args.scene}: the render did not take the route asked for")
        return dt, int(c["segments"]), int(c["shadow_rays"])

    modes = tuple(int(x) for x in args.modes.split(","))
    key = {0: "off", 1: "on", 2: "mis"}
    for _ in range(args.warmup):
        for on in modes:
            render(on, 1)
    ms = {on: [] for on in modes}
    segs, shadow = {}, {}
    for _ in range(args.runs):
        for on in modes:
            dt, segs[on], shadow[on] = render(on, 1)
            ms[on].append(dt * 1e3)
    med = {on: statistics.median(v) for on, v in ms.items()}
    # the reference: the option off, the parent's behaviour
    t_ref, _, _ = render(0, args.ref_spp)
    ref = pt.readback()[1][..., :3].astype(np.float64)
    equal = []
    for n_on in [int(x) for x in args.spp.split(",")]:
        n_off = max(1, int(round(n_on * med[1] / med[0])))
        row = {}
        for on, n in ((1, n_on), (0, n_off)) + (((2, n_on),) if 2 in modes else ()):
            dt, s, _ = render(on, n)
            img = pt.readback()[1][..., :3].astype(np.float64)
            err = np.sort(((img - ref) ** 2).mean(axis=-1).ravel())  # per pixel
            row[key[on]] = {"frames": n, "ms": round(dt * 1e3, 3), "segments": s, "mse": float(err.mean()),
                                          # where the error sits: without the 0.1 % of pixels that err most
                                          "mse_without_worst_permille": float(err[:len(err) - len(err) // 1000].mean()),
                                          "max_abs_error": float(np.abs(img - ref).max())}
        equal.append(row)
    select = None
    if args.select:
        vals = tuple(int(x) for x in args.select.split(","))

        def render_select(sel, frames):
            pt.setOption(hippt.OPT_LIGHT_SELECT, sel)
            got = render(2, frames)
            if int(lib.hipptGetOption(hippt.INFO_LIGHT_SELECT)) != sel:
                raise SystemExit(f"{args.scene}: the render did not apply light selection {sel}")
            return got

        for _ in range(args.warmup):
            for sel in vals:
                render_select(sel, 1)
        sms = {sel: [] for sel in vals}
        for _ in range(args.runs):
            for sel in vals:
                sms[sel].append(render_select(sel, 1)[0] * 1e3)
        smed = {sel: statistics.median(v) for sel, v in sms.items()}
        rows = []
        for n0 in [int(x) for x in args.spp.split(",")]:
            row = {}
            for sel in vals:
                n = max(1, int(round(n0 * smed[vals[0]] / smed[sel])))
                dt, s, sh = render_select(sel, n)
                img = pt.readback()[1][..., :3].astype(np.float64)
                err = np.sort(((img - ref) ** 2).mean(axis=-1).ravel())
                row[str(sel)] = {"frames": n, "ms": round(dt * 1e3, 3), "segments": s, "shadow_rays": sh,
                                 "mse": float(err.mean()),
                                 "mse_without_worst_permille": float(err[:len(err) - len(err) // 1000].mean()),
                                 "max_abs_error": float(np.abs(img - ref).max())}
            rows.append(row)
        pt.setOption(hippt.OPT_LIGHT_SELECT, 0)
        select = {"mode": 2, "order": ", ".join(str(v) for v in vals) + " alternating per call",
                  "ms": {str(sel): [round(x, 4) for x in sms[sel]] for sel in vals},
                  "median_ms": {str(sel): round(smed[sel], 4) for sel in vals}, "equal_time": rows}
    pt.setOption(hippt.OPT_LIGHT_SAMPLING, 0)
    out = {"scene": sc.name, "primitives": sc.num_tris + sc.num_spheres, "lights": int(lib.hipptGetOption(hippt.INFO_LIGHTS)),
           "width": W, "height": H, "max_depth": DEPTH, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(torch.device("cuda", args.device)),
           "order": ", ".join(key[on] for on in modes) + " alternating per call",
           "ms": {key[on]: [round(x, 4) for x in ms[on]] for on in modes},
           "median_ms": {key[on]: round(med[on], 4) for on in modes},
           "segments_per_frame": {key[on]: segs[on] for on in modes},
           "shadow_rays_per_frame": shadow[1], "shadow_share": round(shadow[1] / max(1, segs[1]), 4),
           "gsegments_per_s": {key[on]: round(segs[on] / med[on] / 1e6, 3) for on in modes},
           "reference": {"spp": args.ref_spp, "option": 0, "seconds": round(t_ref, 3)},
           "equal_time": equal}
    if select:
        out["select"] = select
    lib.cudaPathTracerShutdown()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell34,cornell_mixed", help="base scenes of hippt.scenes.cornell_lit")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--spp", default="1,4,16,64", help="frames with the option on of the equal-time comparisons")
    ap.add_argument("--modes", default="0,1,2", help="values of the option to time: 0,1 or 0,1,2")
    ap.add_argument("--select", default="", help="values of HIPPT_OPT_LIGHT_SELECT to compare under MIS: 0,1 (default: none)")
    ap.add_argument("--limit", type=float, default=500.0, help="seconds a scene's child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "light_sampling"))
    ap.add_argument("--scene", help=argparse.SUPPRESS)  # the child's
    args = ap.parse_args()
    if args.scene:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", name, "--device", str(args.device), "--warmup",
               str(args.warmup), "--runs", str(args.runs), "--ref-spp", str(args.ref_spp), "--spp", args.spp, "--modes",
               args.modes] + (["--select", args.select] if args.select else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {args.limit:.0f} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"{name}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        with open(os.path.join(args.out, f"{name}.json" if name.endswith("_lamps") else f"{name}_lit.json"), "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")
        m = res["median_ms"]
        cols = [k for k in ("on", "off", "mis") if k in res["equal_time"][0]]
        eq = "  ".join(f"{e['on']['frames']}v{e['off']['frames']}: " + "/".join(f"{e[k]['mse']:.4g}" for k in cols) + " (" +
                       "/".join(f"{e[k]['mse_without_worst_permille']:.4g}" for k in cols) + ") max " +
                       "/".join(f"{e[k]['max_abs_error']:.4g}" for k in cols) for e in res["equal_time"])
        print(f"{res['scene']:18s} " + "  ".join(f"{k} {v:7.3f} ms" for k, v in m.items()) +
              f"  shadow share {res['shadow_share']:.3f}  mse {'/'.join(cols)} at equal time, frames on v off (without the "
              f"worst 0.1 % of pixels) and the largest error: {eq}", flush=True)
        if "select" in res:
            sel = res["select"]
            print(f"{res['scene']:18s} light choice under MIS: " + "  ".join(f"{k} {v:7.3f} ms" for k, v in sel["median_ms"].items()) +
                  "  mse at equal time: " + "  ".join("v".join(str(r["frames"]) for r in e.values()) + ": " +
                                                      "/".join(f"{r['mse']:.4g}" for r in e.values()) for e in sel["equal_time"]),
                  flush=True)


if __name__ == "__main__":
    main()
