#!/usr/bin/env python3
"""What hipptDenoise costs beside the frame it cleans.

Per scene at --width x --height with the default parameters, after --warmup untimed calls, the medians
over --runs calls (a 1-spp render and a denoise alternating, so that both see the same machine state) of
  * the device time of each stage of the call (HIPPT_OPT_DENOISE_TIMING: HIP events around the guide
    query, prepare, each pass and finish; read with HIPPT_INFO_DENOISE_NS),
  * the host time of the whole blocking call (it ends in the wait for its own event), with the timing
    events off,
  * the host time of the blocking 1-spp hipptRenderFrames call of the same scene (no host copy).
Each pass is set against its compulsory traffic (48 B per pixel: colour and guide in, colour out) at the
achievable HBM bandwidth of MI355X_MICROARCH.md (6.3 TB/s).

Writes one JSON file per scene into --out and prints one line per figure."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qt-raytracer_amd"))

import hippt  # noqa: E402
from hippt import scenes  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
PASS_BYTES_PER_PIXEL = 48


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell34,blob70k")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=41)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise"))
    args = ap.parse_args()
    if hippt.device_count() < 1:
        raise SystemExit("no HIP device")
    os.makedirs(args.out, exist_ok=True)
    lib = hippt.load_library()
    e = ctypes.c_char_p()
    w, h = args.width, args.height
    floor_ms = w * h * PASS_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    for name in args.scenes.split(","):
        sc = scenes.get_scene(name)
        pt = hippt.PathTracer()
        pt.setDevices([0])
        pt.uploadMesh(sc)
        if not pt.initialize(w, h) or not pt.renderFrames(1, args.depth, copy=False):
            raise SystemExit(pt.lastError())
        import numpy as np
        px = np.empty((h, w), np.uint32)

        def denoise():
            t0 = time.perf_counter()
            if not lib.hipptDenoise(None, px.ctypes.data, None, ctypes.byref(e)):
                raise SystemExit(e.value.decode() if e.value else "denoise failed")
            return (time.perf_counter() - t0) * 1e3

        def frame(k):
            t0 = time.perf_counter()
            if not lib.hipptRenderFrames(k, 1, args.depth, None, ctypes.byref(e)):
                raise SystemExit(e.value.decode() if e.value else "render failed")
            return (time.perf_counter() - t0) * 1e3

        stages = {}
        calls, timed_calls, frames = [], [], []
        k = 1
        for run in range(args.warmup + args.runs):
            pt.setOption(hippt.OPT_DENOISE_TIMING, 0)
            f = frame(k)
            k += 1
            c = denoise()
            pt.setOption(hippt.OPT_DENOISE_TIMING, 1)
            tc = denoise()
            if run < args.warmup:
                continue
            frames.append(f)
            calls.append(c)
            timed_calls.append(tc)
            for stage, ms in pt.denoiseTimes().items():
                stages.setdefault(stage, []).append(ms)
        pt.setOption(hippt.OPT_DENOISE_TIMING, 0)
        med = {s: statistics.median(v) for s, v in stages.items()}
        spread = {s: (min(v), max(v)) for s, v in stages.items()}
        res = {
            "scene": name, "width": w, "height": h, "depth": args.depth, "runs": args.runs, "warmup": args.warmup,
            "stage_ms_median": med, "stage_ms_min_max": spread,
            "stages_sum_ms": sum(med.values()),
            "call_ms_median": statistics.median(calls), "call_ms_min_max": (min(calls), max(calls)),
            "call_with_events_ms_median": statistics.median(timed_calls),
            "frame_1spp_ms_median": statistics.median(frames), "frame_1spp_ms_min_max": (min(frames), max(frames)),
            "call_over_frame": statistics.median(calls) / statistics.median(frames),
            "pass_floor_ms": floor_ms,
            "pass_over_floor": {s: med[s] / floor_ms for s in med if s.startswith("pass")},
            "output_copy_bytes": w * h * 4,
        }
        with open(os.path.join(args.out, f"{name}.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        for s, ms in med.items():
            extra = f"  ({ms / floor_ms:.1f} x the {floor_ms:.4f} ms floor)" if s.startswith("pass") else ""
            print(f"{name} {s:8s} {ms:8.4f} ms  [{spread[s][0]:.4f} .. {spread[s][1]:.4f}]{extra}")
        print(f"{name} stages   {res['stages_sum_ms']:8.4f} ms (sum of medians)")
        print(f"{name} call     {res['call_ms_median']:8.4f} ms  [{min(calls):.4f} .. {max(calls):.4f}] (host clock, words to the host)")
        print(f"{name} frame    {res['frame_1spp_ms_median']:8.4f} ms  [{min(frames):.4f} .. {max(frames):.4f}] (1 spp, host clock)")
        print(f"{name} call / frame {res['call_over_frame']:.2f}")
        lib.cudaPathTracerShutdown()


if __name__ == "__main__":
    main()
