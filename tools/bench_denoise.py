#!/usr/bin/env python3
"""Time of the denoiser (include/srt_denoise.h) on a rendered Rubik frame at WIDTH x HEIGHT.

For each setting of SRT_DENOISE_TILE (0 = every pass reads its taps from global memory, the default crossover,
and the larger tiled steps) it times srt_denoise_run with passes = 1 .. PASSES by torch.cuda.Event pairs around
the enqueued call (--warmup runs unmeasured, median of --reps).  A run of k passes is k launches whose last
writes the float output instead of a ping-pong buffer (the same bytes), so pass i's own time is reported as
t(i + 1 passes) - t(i passes).  Beside them, timed the same way in the same process: a float4 copy of one frame
(the bandwidth floor one pass is to be read against), and the guide (primary rays + srt_query_closest).
Nothing is asserted: this is a measurement tool.  --out writes the JSON document (profiles/denoise.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)


def time_calls(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.current_stream().synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--knobs", nargs="+", default=["default", "0", "1", "4", "8"], help="SRT_DENOISE_TILE settings")
    ap.add_argument("--out", help="write the results to this JSON file")
    a = ap.parse_args()
    if a.warmup < 3 or a.reps < 10:
        ap.error("at least 3 warm-up runs and 10 measured ones")
    import torch

    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query

    W, H = a.width, a.height
    setup = R.make_setup(W, H, show_model=True, models=[R.rubik_model(ROOT / "tests" / "golden" / "objects")])
    rdr = R.Renderer(setup)
    lib = _lib.lib()
    doc = {"tool": "tools/bench_denoise.py", "width": W, "height": H, "spp": a.spp, "scene": "rubik",
           "device": torch.cuda.get_device_name(0), "code_hash": lib.srt_code_hash().decode(),
           "warmup": a.warmup, "reps": a.reps,
           "timing": "torch.cuda.Event pairs around the enqueued calls on one stream; median [min, max] ms; "
                     "pass_ms[i] = t(i + 1 passes) - t(i passes)"}
    try:
        rdr.render(a.spp)
        rdr.finish()
        frames = rdr.accum_frames
        acc_ptr, _ = rdr.compute.image_pointers()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
            src = torch.rand((H, W, 4), dtype=torch.float32, device="cuda")
            doc["copy_float4_frame_ms"] = time_calls(torch, lambda: out.copy_(src), a.warmup, a.reps)
            doc["frame_bytes"] = W * H * 16
            with Query(setup.scene, stream=stream) as q:
                q.set_bvh_count(setup.bvh_count)
                hits = None
                runs = []
                for knob in a.knobs:
                    if knob == "default":
                        os.environ.pop("SRT_DENOISE_TILE", None)
                    else:
                        os.environ["SRT_DENOISE_TILE"] = knob
                    with Denoiser(W, H, stream=stream) as dn:
                        if hits is None:
                            rays = dn.primary_rays(setup.camera)
                            hits = q.closest(rays)
                            doc["guide_ms"] = time_calls(
                                torch, lambda: (lib.srt_denoise_primary_rays(dn.handle, *cam_ptrs(setup.camera), C.c_void_p(rays.data_ptr())),
                                                lib.srt_query_closest(q.handle, C.c_void_p(rays.data_ptr()), W * H, C.c_void_p(hits.raw.data_ptr()))),
                                a.warmup, a.reps)
                            doc["hit_fraction"] = round(float(hits.hit.float().mean()), 4)
                        r = {"SRT_DENOISE_TILE": knob, "tile_max_step": dn.get_int("tile.max_step"),
                             "tile_lds_bytes": dn.get_int("tile.lds_bytes"), "cumulative_ms": [], "pass_ms": [], "kernel": []}
                        args = (dn.handle, C.c_void_p(acc_ptr), frames, C.c_void_p(hits.raw.data_ptr()), C.c_void_p(out.data_ptr()), None)
                        prev = 0.0
                        for k in range(1, a.passes + 1):
                            dn.set_params(passes=k)
                            t = time_calls(torch, lambda: lib.srt_denoise_run(*args), a.warmup, a.reps)
                            r["cumulative_ms"].append(t)
                            r["pass_ms"].append(round(t[0] - prev, 4))
                            r["kernel"].append("tiled" if (1 << (k - 1)) <= r["tile_max_step"] else "direct")
                            prev = t[0]
                        r["total_ms"] = r["cumulative_ms"][-1]
                        r["total_over_copy"] = round(r["total_ms"][0] / doc["copy_float4_frame_ms"][0], 2)
                        print(json.dumps(r), flush=True)
                        runs.append(r)
                doc["runs"] = runs
                # which kernel won at which step: the all-direct run against the run that tiles the step
                direct = next((r for r in runs if r["tile_max_step"] == 0), None)
                if direct:
                    doc["per_step"] = []
                    for i in range(a.passes):
                        step = 1 << i
                        tiled = [r["pass_ms"][i] for r in runs if r["tile_max_step"] >= step]
                        doc["per_step"].append({"step": step, "direct_ms": direct["pass_ms"][i],
                                                "tiled_ms": min(tiled) if tiled else None,
                                                "faster": ("tiled" if tiled and min(tiled) < direct["pass_ms"][i] else "direct")})
    finally:
        rdr.close()
    print(json.dumps({k: v for k, v in doc.items() if k != "runs"}), flush=True)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


_keep = []


def cam_ptrs(cam):
    import numpy as np

    vec = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(3)) for v in
           (cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector())]
    _keep[:] = vec
    return [C.c_void_p(v.ctypes.data) for v in vec]


if __name__ == "__main__":
    main()
