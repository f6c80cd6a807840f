#!/usr/bin/env python3
"""Time of the temporal moments and the variance-guided filter (include/srt_variance.h) on a rendered Rubik frame
at WIDTH x HEIGHT, beside the calls they extend, in the same process.

torch.cuda.Event pairs around the enqueued call on one stream (--warmup runs unmeasured, median of --reps with
[min, max]), two series in one process (the first series of a process reads slow; DESIGN.md, "Denoiser"):
  srt_temporal_accumulate_moments against srt_temporal_accumulate, each with the history of a camera one small step
  away (the interactive case);
  srt_denoise_run_variance at passes = 1..5 against srt_denoise_run at 5 passes, both fed the temporal output; the
  per-pass times are differences of consecutive pass counts (the last pass of each count also writes the outputs),
  and the resolve launch is what one pass's total leaves after the first difference is taken off -- it is also timed
  directly as the 1-pass run minus a plain 1-pass run's difference, so read it as an estimate.
Nothing is asserted: this is a measurement tool.  --out writes the JSON document (profiles/variance.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

# from -Rpass-analysis=kernel-resource-usage on the gfx950 build (VGPRs, SGPRs, scratch bytes, waves per SIMD)
KERNELS = {
    "temporal_accumulate_moments_kernel": {"vgprs": 73, "sgprs": 62, "scratch": 0, "waves_per_simd": 6},
    "temporal_accumulate_motion_moments_kernel": {"vgprs": 73, "sgprs": 62, "scratch": 0, "waves_per_simd": 6},
    "variance_resolve_kernel": {"vgprs": 38, "sgprs": 44, "scratch": 0, "waves_per_simd": 8},
    "variance_pass_kernel": {"vgprs": 48, "sgprs": 70, "scratch": 0, "waves_per_simd": 8},
}


def time_calls(torch, fn, warmup, reps, before=None):
    """Median, min and max ms of `fn` over `reps` runs; `before` (untimed) is enqueued ahead of each."""
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.current_stream().synchronize()
    ms = []
    for _ in range(reps):
        if before:
            before()
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
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", help="write the results to this JSON file")
    a = ap.parse_args()
    if a.warmup < 3 or a.reps < 10:
        ap.error("at least 3 warm-up runs and 10 measured ones")
    import torch

    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.temporal import Temporal, _camera

    W, H = a.width, a.height
    setup = R.make_setup(W, H, show_model=True, models=[R.rubik_model(ROOT / "tests" / "golden" / "objects")])
    rdr = R.Renderer(setup)
    lib = _lib.lib()
    doc = {"tool": "tools/bench_variance.py", "width": W, "height": H, "spp": a.spp, "scene": "rubik",
           "device": torch.cuda.get_device_name(0), "code_hash": lib.srt_code_hash().decode(),
           "warmup": a.warmup, "reps": a.reps, "kernels": KERNELS, "counters_collected": False,
           "scope": "one scene and one size were measured",
           "timing": "torch.cuda.Event pairs around the enqueued call on one stream; median [min, max] ms; the calls "
                     "that set a state up (the previous frame) are enqueued before the first event"}
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    try:
        rdr.render(a.spp)
        rdr.finish()
        frames = rdr.accum_frames
        acc_ptr, _ = rdr.compute.image_pointers()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out, mom, den = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3))
            var = torch.empty((H, W), dtype=torch.float32, device="cuda")
            with Query(setup.scene, stream=stream) as q, Denoiser(W, H, stream=stream) as dn, \
                    Temporal(W, H, stream=stream) as tp, Temporal(W, H, stream=stream) as plain:
                tp.enable_moments()
                dn.enable_variance()
                q.set_bvh_count(setup.bvh_count)
                cam0 = _camera(setup.camera)
                hits0 = q.closest(dn.primary_rays(setup.camera))
                setup.camera.MoveRight(0.5)
                setup.camera.Rotate(-1.0, 0.0)
                cam1 = _camera(setup.camera)
                hits1 = q.closest(dn.primary_rays(setup.camera))
                doc["hit_fraction"] = round(float(hits0.hit.float().mean()), 4)
                doc["moments_bytes"], doc["variance_bytes"] = tp.get_int("moments.bytes"), dn.get_int("variance.bytes")

                def acc_plain(hits, cam):
                    return lib.srt_temporal_accumulate(plain.handle, C.c_void_p(acc_ptr), frames, P(hits.raw), C.byref(cam), P(out))

                def acc_moments(hits, cam):
                    return lib.srt_temporal_accumulate_moments(tp.handle, C.c_void_p(acc_ptr), frames, P(hits.raw), C.byref(cam),
                                                               P(out), P(mom))

                def run_plain():
                    return lib.srt_denoise_run(dn.handle, P(out), 1, P(hits1.raw), P(den), None)

                def run_var():
                    return lib.srt_denoise_run_variance(dn.handle, P(out), 1, P(hits1.raw), P(mom), P(den), None, P(var))

                series = []
                for _ in range(2):
                    row = {}
                    row["accumulate_moved_camera_ms"] = time_calls(torch, lambda: acc_plain(hits1, cam1), a.warmup, a.reps,
                                                                   before=lambda: acc_plain(hits0, cam0))
                    row["accumulate_moments_moved_camera_ms"] = time_calls(torch, lambda: acc_moments(hits1, cam1), a.warmup,
                                                                           a.reps, before=lambda: acc_moments(hits0, cam0))
                    # `out` and `mom` now hold the moved frame's temporal output and moments: the filters' input
                    for passes in (1, 2, 3, 4, 5):
                        dn.set_params(passes=passes)
                        row[f"run_variance_{passes}_passes_ms"] = time_calls(torch, run_var, a.warmup, a.reps)
                        row[f"run_{passes}_passes_ms"] = time_calls(torch, run_plain, a.warmup, a.reps)
                    for kind in ("run_variance", "run"):
                        t = [row[f"{kind}_{p}_passes_ms"][0] for p in (1, 2, 3, 4, 5)]
                        row[f"{kind}_per_added_pass_ms"] = [round(t[i] - t[i - 1], 4) for i in range(1, 5)]
                    # a 1-pass variance run is the resolve plus one pass at step 1; a later pass costs about what the
                    # second difference shows, so the resolve is what remains (an estimate: step 1 is not step 2)
                    row["resolve_estimate_ms"] = round(row["run_variance_1_passes_ms"][0] - row["run_variance_per_added_pass_ms"][0], 4)
                    series.append(row)
                doc["series"] = series
                tp.synchronize()
                # the alternating cameras above let N grow: the steady state of an interactive session
                n = mom[..., 3][hits1.hit.reshape(H, W)]
                doc["young_fraction_of_hits"] = round(float((n < 4).float().mean()), 4)
                # the other extreme: two frames after a reset every hit pixel is young and takes the 7 x 7 estimate
                lib.srt_temporal_reset(tp.handle)
                acc_moments(hits0, cam0)
                acc_moments(hits1, cam1)
                doc["all_young"] = {f"run_variance_{p}_passes_ms": None for p in (1, 5)}
                for passes in (1, 5):
                    dn.set_params(passes=passes)
                    doc["all_young"][f"run_variance_{passes}_passes_ms"] = time_calls(torch, run_var, a.warmup, a.reps)
                tp.synchronize()
                n = mom[..., 3][hits1.hit.reshape(H, W)]
                doc["all_young"]["young_fraction_of_hits"] = round(float((n < 4).float().mean()), 4)
        s = series[1]
        doc["moments_over_accumulate"] = round(s["accumulate_moments_moved_camera_ms"][0] / s["accumulate_moved_camera_ms"][0], 3)
        doc["run_variance_over_run_5_passes"] = round(s["run_variance_5_passes_ms"][0] / s["run_5_passes_ms"][0], 3)
    finally:
        rdr.close()
    print(json.dumps(doc), flush=True)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
