#!/usr/bin/env python3
"""Times of guided upsampling (include/srt_upsample.h) at WIDTH x HEIGHT (default 1920 x 1080).

Per call, by torch.cuda.Event pairs around the enqueued calls on one stream (--warmup calls unmeasured, the median of
--reps): srt_upsample_run for f = 2 and f = 4 with both kernel variants (SRT_UPSAMPLE_STAGED = 1: the footprint staged
in LDS, = 0: every tap from global memory), the guide pair (primary rays + srt_query_closest at the low and at the full
size), and a float4 copy of one full frame (the bandwidth floor).

Whole frames on Rubik and on the 262k-triangle knot, by the host's wall clock from the first call to the end of the
last (the render's srt_finish, then a synchronise of the stage stream):
  low   render f^2 spp at (W / f) x (H / f), both guides, srt_upsample_run
  full  render 1 spp at W x H, one guide
`--mode full` times the full leg alone and needs nothing of this feature, so it also runs on a checkout of the parent
commit: `--parent-root DIR` (such a checkout, built) makes the tool run parent, this build, parent in child processes
and report all three.  Nothing is asserted: this is a measurement tool.  --out writes the JSON document
(profiles/upsample.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
FACTORS = (2, 4)


def stats(ms):
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


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
    return stats(ms)


def time_wall(torch, fn, warmup, reps):
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def models(R):
    return (("rubik", lambda: R.rubik_model(ROOT / "tests" / "golden" / "objects")), ("knot", R.torus_knot_model))


def full_leg(torch, R, model, W, H, warmup, reps):
    """1 spp at W x H + one guide."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query

    setup = R.make_setup(W, H, show_model=True, models=[model])
    rdr = R.Renderer(setup)
    try:
        with Denoiser(W, H) as dn, Query(setup.scene) as q:
            q.set_bvh_count(setup.bvh_count)

            def frame():
                rdr.render(1)
                rdr.finish()
                q.closest(dn.primary_rays(setup.camera))

            return {"triangles": len(setup.scene.tris), "full_ms": time_wall(torch, frame, warmup, reps)}
    finally:
        rdr.close()


def low_leg(torch, R, model, W, H, f, warmup, reps):
    """f^2 spp at (W / f) x (H / f) + both guides + the upsampling."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.upsample import Upsampler

    w, h = W // f, H // f
    setup = R.make_setup(w, h, show_model=True, models=[model])
    rdr = R.Renderer(setup)
    try:
        with Denoiser(w, h) as dl, Denoiser(W, H) as dn, Query(setup.scene) as q, Upsampler(w, h, f) as up:
            q.set_bvh_count(setup.bvh_count)
            rdr.render(1)
            rdr.finish()
            acc_ptr, _ = rdr.compute.image_pointers()

            def frame():
                rdr.render(f * f)
                rdr.finish()
                up.run(acc_ptr, rdr.accum_frames, q.closest(dl.primary_rays(setup.camera)),
                       q.closest(dn.primary_rays(setup.camera)))

            def render_only():
                rdr.render(f * f)
                rdr.finish()

            return {"low_ms": time_wall(torch, frame, warmup, reps), "low_render_ms": time_wall(torch, render_only, warmup, reps)}
    finally:
        rdr.close()


def per_call(torch, R, lib, W, H, warmup, reps):
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.upsample import Upsampler

    doc = {}
    model = R.rubik_model(ROOT / "tests" / "golden" / "objects")
    setup = R.make_setup(W, H, show_model=True, models=[model])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), Query(setup.scene, stream=stream) as q, Denoiser(W, H, stream=stream) as dn:
        q.set_bvh_count(setup.bvh_count)
        out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        src = torch.rand((H, W, 4), dtype=torch.float32, device="cuda")
        doc["copy_float4_frame_ms"] = time_calls(torch, lambda: out.copy_(src), warmup, reps)
        full_rays = dn.primary_rays(setup.camera)
        full_hits = q.closest(full_rays)
        cam = cam_ptrs(setup.camera)
        doc["factors"] = []
        for f in FACTORS:
            w, h = W // f, H // f
            low_setup = R.make_setup(w, h, show_model=True, models=[model])
            rdr = R.Renderer(low_setup)
            try:
                rdr.render(f * f)
                rdr.finish()
                acc_ptr, _ = rdr.compute.image_pointers()
                r = {"factor": f, "low": [w, h], "spp": f * f}
                with Denoiser(w, h, stream=stream) as dl:
                    low_rays = dl.primary_rays(setup.camera)
                    low_hits = q.closest(low_rays)

                    def guides():
                        lib.srt_denoise_primary_rays(dl.handle, *cam, C.c_void_p(low_rays.data_ptr()))
                        lib.srt_query_closest(q.handle, C.c_void_p(low_rays.data_ptr()), w * h, C.c_void_p(low_hits.raw.data_ptr()))
                        lib.srt_denoise_primary_rays(dn.handle, *cam, C.c_void_p(full_rays.data_ptr()))
                        lib.srt_query_closest(q.handle, C.c_void_p(full_rays.data_ptr()), W * H, C.c_void_p(full_hits.raw.data_ptr()))

                    r["guide_pair_ms"] = time_calls(torch, guides, warmup, reps)
                    for knob, name in (("1", "staged"), ("0", "direct")):
                        os.environ["SRT_UPSAMPLE_STAGED"] = knob
                        with Upsampler(w, h, f, stream=stream) as up:
                            args = (up.handle, C.c_void_p(acc_ptr), rdr.accum_frames, C.c_void_p(low_hits.raw.data_ptr()),
                                    C.c_void_p(full_hits.raw.data_ptr()), C.c_void_p(out.data_ptr()), None)
                            r[name + "_ms"] = time_calls(torch, lambda: lib.srt_upsample_run(*args), warmup, reps)
                    os.environ.pop("SRT_UPSAMPLE_STAGED", None)
                    r["faster"] = "staged" if r["staged_ms"][0] <= r["direct_ms"][0] else "direct"
                print(json.dumps(r), flush=True)
                doc["factors"].append(r)
            finally:
                rdr.close()
    return doc


_keep = []


def cam_ptrs(cam):
    import numpy as np

    vec = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(3)) for v in
           (cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector())]
    _keep.extend(vec)
    return [C.c_void_p(v.ctypes.data) for v in vec]


def run_mode(a):
    root = pathlib.Path(a.root) if a.root else ROOT
    for p in (str(root / "simple-ray-tracer_amd"), str(root)):
        sys.path.insert(0, p)
    import torch

    from srt_amd import _lib
    from srt_amd import render as R

    lib = _lib.lib()
    W, H = a.width, a.height
    doc = {"mode": a.mode, "code_hash": lib.srt_code_hash().decode(), "device": torch.cuda.get_device_name(0)}
    if a.mode == "all":
        doc["per_call"] = per_call(torch, R, lib, W, H, a.warmup, a.reps)
    doc["frames"] = []
    for name, make in models(R):
        model = make()
        r = {"scene": name, **full_leg(torch, R, model, W, H, a.warmup, a.reps)}
        if a.mode == "all":
            for f in FACTORS:
                r[f"f{f}"] = low_leg(torch, R, model, W, H, f, a.warmup, a.reps)
        print(json.dumps(r), flush=True)
        doc["frames"].append(r)
    print("RESULT " + json.dumps(doc), flush=True)


def child(a, mode, root):
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--mode", mode, "--width", str(a.width), "--height", str(a.height),
           "--warmup", str(a.warmup), "--reps", str(a.reps)] + (["--root", str(root)] if root else [])
    try:  # a leg that hangs ends the tool: the next child is not started
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired as e:
        raise SystemExit(f"{' '.join(cmd)} did not end within {a.child_timeout} s:\n{e.stdout}\n{e.stderr}")
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    sys.stdout.write("".join(l + "\n" for l in r.stdout.splitlines() if not l.startswith("RESULT ")))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=("bracket", "all", "full"), default="bracket",
                    help="bracket: child processes (parent, this build, parent); all / full: one measurement in this process")
    ap.add_argument("--root", help="with --mode all / full: the checkout whose package and library are timed")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit, for the bracket's outer legs")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds a child process of the bracket may take")
    ap.add_argument("--out", help="write the results to this JSON file")
    a = ap.parse_args()
    if a.warmup < 3 or a.reps < 10:
        ap.error("at least 3 warm-up runs and 10 measured ones")
    if a.width % 4 or a.height % 4:
        ap.error("width and height must be multiples of 4: the factors timed are 2 and 4")
    if a.mode != "bracket":
        return run_mode(a)
    doc = {"tool": "tools/bench_upsample.py", "width": a.width, "height": a.height, "warmup": a.warmup, "reps": a.reps,
           "timing": "per call: torch.cuda.Event pairs around the enqueued calls on one stream; frames: host wall clock, "
                     "synchronised before and after; median [min, max] ms",
           "order": []}
    if a.parent_root:
        doc["parent_before"] = child(a, "full", a.parent_root)
        doc["order"].append("parent_before")
    doc["this_build"] = child(a, "all", None)
    doc["order"].append("this_build")
    if a.parent_root:
        doc["parent_after"] = child(a, "full", a.parent_root)
        doc["order"].append("parent_after")
    print(json.dumps(doc))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
