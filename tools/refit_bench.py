#!/usr/bin/env python3
"""What an animated mesh costs per frame with hipptUpdateVertices (in-place refit) against the only
path there was before it, hipptUploadScene (host SAH rebuild, stream drain, reallocation).

(a) loop: per scene at --width x --height, the host time per iteration of
        {wobble step, new vertices in, one 1-spp hipptRenderFramesPresent of frame 0}
    ended by one hipptSynchronize, for `update` (hipptUpdateVertices) and `upload` (hipptUploadScene),
    with host vertices (numpy: V0 + a * S_i, S_i one of 8 precomputed sine fields) and device
    vertices (a torch tensor deformed on the device; `upload` has to bring it to the host first).
    The two modes alternate (update, upload, update, upload, ...) after a warm-up; medians of --runs.
    Also: the host time of the hipptUpdateVertices call alone (host path: the scan for non-finite
    values and the copy into pinned staging), and update-to-idle on an idle device (call + staging
    transfer + primitive pass + refit passes + synchronise).
(b) decay: the render rate (ms per 8-spp depth-8 batch) after 1, 10 and 100 cumulative wobble steps
    applied by refit, against a fresh hipptUploadScene of the same vertices.
--kernels N runs N update+render iterations and nothing else (for a kernel trace of the passes).
--lights N runs measurement (c) and nothing else: the scene with every Nth triangle emissive (6, 4, 2), under
    HIPPT_LIGHT_SAMPLING_MIS: hipptUpdateVertices (host memory) plus a 1-spp frame to idle with
    HIPPT_OPT_LIGHT_SELECT 0 and 1 alternating, and the update alone to idle on that scene against the same
    triangles without a light (no selection table to rebuild): the difference is the table's share of an update.
    Written to <out>/<scene>_lights.json.

Writes one JSON file per scene into --out and prints one line per figure."""
import argparse
import copy
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


def with_verts(sc, v):
    out = copy.copy(sc)
    out.verts = v
    return out


def lights(args, lib, dev):
    """Measurement (c): the selection table's rebuild behind the refit."""
    for name in args.scenes.split(","):
        plain = scenes.get_scene(name)
        v0 = np.ascontiguousarray(plain.verts, np.float32).reshape(-1, 9)
        p = v0.reshape(-1, 3)
        ext = float((p.max(axis=0) - p.min(axis=0)).max())
        phase = 0.7 * (np.arange(9) % 3)
        moved = [v0 + np.float32(0.02 * ext) * np.sin(7.0 / ext * v0.astype(np.float64) + phase + 0.37 * i).astype(np.float32)
                 for i in range(8)]
        lit = copy.copy(plain)
        m = plain.materials()
        k = len(m)
        tm = np.array(plain.tri_mat, np.int32)
        tm[np.arange(args.lights // 2, len(tm), args.lights)] = k
        lit.tri_mat = tm
        lit.albedo = np.concatenate([m["albedo"], [(6.0, 4.0, 2.0)]]).astype(np.float32)
        lit.mat_kind = np.concatenate([m["kind"], [scenes.MAT_EMISSIVE]]).astype(np.int32)
        lit.fuzz = np.concatenate([m["fuzz"], [0.0]]).astype(np.float32)
        lit.ir = np.concatenate([m["ir"], [1.0]]).astype(np.float32)
        pt = hippt.PathTracer()
        pt.setDevices([args.device])
        pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, hippt.LIGHT_SAMPLING_MIS)

        def loop(frame):
            t0 = time.perf_counter()
            for i in range(args.iters):
                pt.updateVertices(moved[i % 8])
                if frame:
                    assert pt.renderFramesAsync(1, args.depth), pt.lastError()
                assert pt.synchronize(), pt.lastError()
            return (time.perf_counter() - t0) * 1e3 / args.iters

        out = {"scene": name, "triangles": len(v0), "every": args.lights, "width": args.width, "height": args.height,
               "depth": args.depth, "iters": args.iters, "warmup": args.warmup, "runs": args.runs,
               "device": torch.cuda.get_device_name(dev), "unit": "ms per iteration to idle (host clock)"}
        # the update alone: with lights (the table is rebuilt behind the refit) against without (no table)
        alone = {}
        for what, sc in (("with_lights", lit), ("without_lights", plain)):
            pt.uploadScene(sc)
            if not pt.initialize(args.width, args.height):
                raise SystemExit(pt.lastError())
            if what == "with_lights":
                out["lights"] = int(lib.hipptGetOption(hippt.INFO_LIGHTS))
            for _ in range(args.warmup):
                loop(False)
            alone[what] = [round(loop(False), 4) for _ in range(args.runs)]
        out["update_alone_ms"] = alone
        # update + one frame, the light choice off and on, alternating
        pt.uploadScene(lit)
        if not pt.initialize(args.width, args.height):
            raise SystemExit(pt.lastError())
        frame = {"0": [], "1": []}
        for r in range(args.warmup + args.runs):
            for sel in (0, 1):
                pt.setOption(hippt.OPT_LIGHT_SELECT, sel)
                ms = loop(True)
                if int(lib.hipptGetOption(hippt.INFO_LIGHT_SELECT)) != sel:
                    raise SystemExit("the render did not apply the light choice asked for")
                if r >= args.warmup:
                    frame[str(sel)].append(round(ms, 4))
        pt.setOption(hippt.OPT_LIGHT_SELECT, 0)
        out["update_plus_frame_ms"] = frame
        med = {w: statistics.median(v) for w, v in alone.items()}
        fmed = {w: statistics.median(v) for w, v in frame.items()}
        out["median_ms"] = {"update_with_lights": med["with_lights"], "update_without_lights": med["without_lights"],
                            "table": round(med["with_lights"] - med["without_lights"], 4),
                            "update_plus_frame_select_0": fmed["0"], "update_plus_frame_select_1": fmed["1"],
                            "table_share_of_update_plus_frame": round((med["with_lights"] - med["without_lights"]) / fmed["1"], 4)}
        with open(os.path.join(args.out, f"{name}_lights.json"), "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")
        print(f"{name}: {out['lights']} lights; update alone {med['with_lights']:.3f} ms with lights, "
              f"{med['without_lights']:.3f} ms without (table {out['median_ms']['table']:.3f} ms); update + frame "
              f"{fmed['0']:.3f} ms uniform, {fmed['1']:.3f} ms by power", flush=True)
    pt.setOption(hippt.OPT_LIGHT_SAMPLING_MODE, 0)
    lib.cudaPathTracerShutdown()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="blob70k,cornell34")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iters", type=int, default=12, help="iterations per timed loop")
    ap.add_argument("--warmup", type=int, default=2, help="untimed loops per mode")
    ap.add_argument("--runs", type=int, default=5, help="timed loops per mode (alternating)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--decay", default="blob70k", help="scenes of measurement (b)")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--lights", type=int, default=0, help="measurement (c): every Nth triangle emissive")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refit"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible to torch")
    os.makedirs(args.out, exist_ok=True)
    lib = hippt.load_library()
    dev = torch.device("cuda", args.device)
    e = ctypes.c_char_p()

    def check(ok):
        if not ok:
            raise SystemExit(e.value.decode() if e.value else "call failed")

    if args.lights:
        return lights(args, lib, dev)
    for name in args.scenes.split(","):
        sc = scenes.get_scene(name)
        v0 = np.ascontiguousarray(sc.verts, np.float32).reshape(-1, 9)
        n = len(v0)
        p = v0.reshape(-1, 3)
        ext = float((p.max(axis=0) - p.min(axis=0)).max())
        amp, k = np.float32(0.02 * ext), 7.0 / ext
        # a displacement field of position alone (one phase per axis), so that triangles keep their shared
        # vertices: the mesh stays a surface and a frame's cost stays the scene's
        phase = 0.7 * (np.arange(9) % 3)
        fields = [np.sin(k * v0.astype(np.float64) + phase + 0.37 * i).astype(np.float32) for i in range(8)]
        dv0 = torch.from_numpy(v0).to(dev)
        dphase = torch.from_numpy(phase.astype(np.float32)).to(dev)
        pt = hippt.PathTracer()
        pt.setDevices([args.device])
        pt.uploadScene(sc)
        if not pt.initialize(args.width, args.height):
            raise SystemExit(pt.lastError())

        def present():
            check(lib.hipptRenderFramesPresent(0, 1, args.depth, ctypes.byref(e)))

        def host_verts(i):
            return v0 + amp * fields[i % 8]

        def dev_verts(i):
            return dv0 + float(amp) * torch.sin(float(k) * dv0 + dphase + 0.37 * (i % 8))

        def step(mode, where, i):
            if where == "host":
                v = host_verts(i)
                if mode == "update":
                    pt.updateVertices(v)
                else:
                    pt.uploadScene(with_verts(sc, v))
            else:
                v = dev_verts(i)
                if mode == "update":
                    pt.updateVertices(v)
                else:
                    pt.uploadScene(with_verts(sc, v.cpu().numpy()))
            present()
            return v

        def loop(mode, where):
            keep = []  # device vertices stay unchanged (alive) until the synchronise
            t0 = time.perf_counter()
            for i in range(args.iters):
                keep.append(step(mode, where, i))
            assert pt.synchronize(), pt.lastError()
            return (time.perf_counter() - t0) * 1e3 / args.iters

        if args.kernels:
            for i in range(args.kernels):
                step("update", "host", i)
            assert pt.synchronize(), pt.lastError()
            lib.cudaPathTracerShutdown()
            continue

        out = {"scene": name, "triangles": n, "width": args.width, "height": args.height, "depth": args.depth,
               "iters": args.iters, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(dev),
               "unit": "ms per iteration (host clock)", "loop": {}}
        # first, before any re-upload starts run-cost jobs on the host's threads: the render alone (no new
        # vertices), the call alone, and update-to-idle on an idle device
        for i in range(20):
            present()
        assert pt.synchronize()
        time.sleep(1.0)  # (the first camera's run-cost estimate: its table is in place from here on)
        alone = {"render_only": [], "call_host": [], "call_device": [], "idle_host": [], "idle_device": []}
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            for i in range(args.iters):
                present()
            assert pt.synchronize()
            t = {"render_only": (time.perf_counter() - t0) * 1e3 / args.iters}
            for where, make in (("host", host_verts), ("device", dev_verts)):
                v = make(r)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                pt.updateVertices(v)
                t1 = time.perf_counter()
                assert pt.synchronize()
                t2 = time.perf_counter()
                t["call_" + where], t["idle_" + where] = (t1 - t0) * 1e3, (t2 - t0) * 1e3
            if r >= args.warmup:
                for key in alone:
                    alone[key].append(round(t[key], 4))
        out["alone"] = {key: {"ms": v, "median_ms": round(statistics.median(v), 4)} for key, v in alone.items()}
        print(f"{name:10s} alone " + "  ".join(f"{key} {v['median_ms']:.3f}" for key, v in out["alone"].items()), flush=True)

        for where in ("host", "device"):
            ms = {"update": [], "upload": []}
            for r in range(args.warmup + args.runs):
                for mode in ("update", "upload"):
                    t = loop(mode, where)
                    if r >= args.warmup:
                        ms[mode].append(round(t, 4))
            row = {m: {"ms": ms[m], "median_ms": round(statistics.median(ms[m]), 4), "min_ms": min(ms[m])} for m in ms}
            row["speedup"] = round(row["upload"]["median_ms"] / row["update"]["median_ms"], 2)
            out["loop"][where] = row
            print(f"{name:10s} loop {where:6s} update {row['update']['median_ms']:9.3f} ms  upload "
                  f"{row['upload']['median_ms']:9.3f} ms  x{row['speedup']}", flush=True)
        if name in args.decay.split(","):
            def rate():
                ms = []
                for r in range(2 + args.runs):
                    t0 = time.perf_counter()
                    check(lib.hipptRenderFramesAsync(0, 8, args.depth, ctypes.byref(e)))
                    assert pt.synchronize()
                    if r >= 2:
                        ms.append(round((time.perf_counter() - t0) * 1e3, 4))
                return ms
            pt.uploadScene(sc)
            base = rate()
            decay = {"what": "ms per 8-spp batch; cumulative steps v += 0.01 * extent * sin(7 / extent * v + axis phase + 0.37 i)",
                     "fresh_v0": {"ms": base, "median_ms": round(statistics.median(base), 4)}, "steps": {}}
            v = v0.astype(np.float64)
            done = 0
            for target in (1, 10, 100):
                while done < target:
                    v = v + 0.01 * ext * np.sin(k * v + phase + 0.37 * done)
                    done += 1
                v32 = np.ascontiguousarray(v, np.float32)
                pt.uploadScene(sc)
                pt.updateVertices(v32)
                refit = rate()
                pt.uploadScene(with_verts(sc, v32))
                fresh = rate()
                row = {"refit_ms": refit, "fresh_ms": fresh, "refit_median_ms": round(statistics.median(refit), 4),
                       "fresh_median_ms": round(statistics.median(fresh), 4)}
                row["refit_over_fresh"] = round(row["refit_median_ms"] / row["fresh_median_ms"], 3)
                decay["steps"][str(target)] = row
                print(f"{name:10s} decay after {target:3d} steps: refit {row['refit_median_ms']:.3f} ms  fresh "
                      f"{row['fresh_median_ms']:.3f} ms  x{row['refit_over_fresh']}", flush=True)
            out["decay"] = decay
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        del pt
        lib.cudaPathTracerShutdown()


if __name__ == "__main__":
    main()
