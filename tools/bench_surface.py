#!/usr/bin/env python3
"""Time of the surface-attribute stage and of albedo-demodulated denoising (include/srt_surface.h) at WIDTH x HEIGHT.

Per scene -- Rubik (constant albedo) and the Airplane-material stand-in (bench.py's knot carrying the Airplane's six
sampled 1024 x 1024 textures) -- it renders --spp frames, traces the guide, and times by torch.cuda.Event pairs around
the enqueued calls on one stream (--warmup runs unmeasured, median [min, max] of --reps): srt_surface_shade,
srt_denoise_run_albedo and srt_denoise_run with the default parameters, and beside them in the same process a float4
copy of one frame and the guide (primary rays + srt_query_closest).  Nothing is asserted: this is a measurement tool.
--out writes the JSON document (profiles/surface.json).

--refit-out (profiles/surface_refit.json) times, per scene, srt_surface_refit (include/srt_surface_refit.h) to waved
vertices already on the device against what the frame loop had to do without it: destroy the surface object and create
it again from the host arrays (wall clock, the textures' upload included when the scene samples them).
--refit-baseline-only times only destroy + create and uses nothing that header added, so the same script run from a
checkout of the parent commit gives the baseline; --refit-baseline FILE folds that file in.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scenes", nargs="+", default=["rubik", "airplane_knot"])
    ap.add_argument("--out", help="write the results to this JSON file")
    ap.add_argument("--refit-out", help="time srt_surface_refit against destroy + create only; write this JSON file")
    ap.add_argument("--refit-baseline-only", action="store_true", help="with --refit-out: destroy + create only")
    ap.add_argument("--refit-baseline", help="with --refit-out: a --refit-baseline-only file of the parent commit to fold in")
    a = ap.parse_args()
    if a.warmup < 3 or a.reps < 10:
        ap.error("at least 3 warm-up runs and 10 measured ones")
    if a.refit_out:
        return refit_main(a)
    import torch

    import bench
    from bench_denoise import cam_ptrs, time_calls
    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.denoise import ALBEDO_FLOOR, Denoiser
    from srt_amd.query import Query
    from srt_amd.surface import Surface

    W, H = a.width, a.height
    lib = _lib.lib()
    doc = {"tool": "tools/bench_surface.py", "width": W, "height": H, "spp": a.spp, "frame_bytes": W * H * 16,
           "device": torch.cuda.get_device_name(0), "code_hash": lib.srt_code_hash().decode(), "warmup": a.warmup,
           "reps": a.reps, "albedo_floor": ALBEDO_FLOOR,
           "timing": "torch.cuda.Event pairs around the enqueued calls on one stream; median [min, max] ms",
           "scenes": []}
    for name in a.scenes:
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else bench.airplane_knot_model()
        setup = R.make_setup(W, H, show_model=True, models=[model])
        rdr = R.Renderer(setup)
        r = {"scene": name, "triangles": len(setup.scene.tris), "sampled_textures": bool(setup.scene.sample_textures)}
        try:
            rdr.render(a.spp)
            rdr.finish()
            frames = rdr.accum_frames
            acc_ptr, _ = rdr.compute.image_pointers()
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
                src = torch.rand((H, W, 4), dtype=torch.float32, device="cuda")
                r["copy_float4_frame_ms"] = time_calls(torch, lambda: out.copy_(src), a.warmup, a.reps)
                with Query(setup.scene, stream=stream) as q, Surface(setup.scene, stream=stream) as surf, \
                        Denoiser(W, H, stream=stream) as dn:
                    q.set_bvh_count(setup.bvh_count)
                    rays = dn.primary_rays(setup.camera)
                    hits = q.closest(rays)
                    attrs = surf.shade(rays, hits)
                    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
                    r["hit_fraction"] = round(float(hits.hit.float().mean()), 4)
                    r["textures"] = surf.get_int("textures")
                    r["guide_ms"] = time_calls(
                        torch, lambda: (lib.srt_denoise_primary_rays(dn.handle, *cam_ptrs(setup.camera), P(rays)),
                                        lib.srt_query_closest(q.handle, P(rays), W * H, P(hits.raw))), a.warmup, a.reps)
                    r["surface_shade_ms"] = time_calls(
                        torch, lambda: lib.srt_surface_shade(surf.handle, P(rays), P(hits.raw), W * H, P(attrs)),
                        a.warmup, a.reps)
                    r["shade_bytes_streamed"] = W * H * 96
                    r["passes"] = dn.get_int("passes")
                    r["run_ms"] = time_calls(
                        torch, lambda: lib.srt_denoise_run(dn.handle, C.c_void_p(acc_ptr), frames, P(hits.raw), P(out), None),
                        a.warmup, a.reps)
                    r["run_albedo_ms"] = time_calls(
                        torch, lambda: lib.srt_denoise_run_albedo(dn.handle, C.c_void_p(acc_ptr), frames, P(hits.raw), P(attrs),
                                                                  C.c_float(ALBEDO_FLOOR), P(out), None), a.warmup, a.reps)
                    r["run_albedo_over_run"] = round(r["run_albedo_ms"][0] / r["run_ms"][0], 3)
                    r["shade_over_copy"] = round(r["surface_shade_ms"][0] / r["copy_float4_frame_ms"][0], 2)
        finally:
            rdr.close()
        print(json.dumps(r), flush=True)
        doc["scenes"].append(r)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


def refit_main(a):
    """--refit-out: see the module docstring."""
    import statistics
    import time

    import numpy as np
    import torch

    import bench
    from bench_denoise import time_calls
    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.surface import Surface

    lib = _lib.lib()
    doc = {"tool": "tools/bench_surface.py --refit-out", "device": torch.cuda.get_device_name(0),
           "code_hash": lib.srt_code_hash().decode(), "warmup": a.warmup, "reps": a.reps,
           "timing": "refit: torch.cuda.Event pairs around the enqueued call, median [min, max] ms; destroy + create: wall "
                     "clock around close() and Surface(scene), which waits for its uploads, median [min, max] ms",
           "scenes": []}
    for name in a.scenes:
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else bench.airplane_knot_model()
        scene = R.make_setup(64, 48, show_model=True, models=[model]).scene
        r = {"scene": name, "triangles": len(scene.tris), "vertices": len(scene.verts), "sampled_textures": bool(scene.sample_textures)}
        ms = []
        surf = Surface(scene)
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            surf.close()
            surf = Surface(scene)
            surf.synchronize()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        surf.close()
        r["destroy_create_ms"] = [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]
        if not a.refit_baseline_only:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream), Surface(scene, stream=stream, refit=True) as s:
                extent = float(np.ptp(scene.verts["pos"], axis=0).max())
                v = R.wave_vertices(scene.verts, 0.014 * extent, 0.3)
                vd = torch.from_numpy(np.ascontiguousarray(v).view(np.float32).reshape(-1, 8)).cuda()
                r["surface_refit_ms"] = time_calls(torch, lambda: lib.srt_surface_refit(s.handle, C.c_void_p(vd.data_ptr()), len(v)),
                                                   a.warmup, a.reps)
                r["refit_bytes"] = s.get_int("refit.bytes")
        print(json.dumps(r), flush=True)
        doc["scenes"].append(r)
    if a.refit_baseline:
        base = json.loads(pathlib.Path(a.refit_baseline).read_text())
        doc["parent_commit_baseline"] = {"code_hash": base["code_hash"], "scenes": base["scenes"],
                                         "what": "the same script with --refit-baseline-only, run in the same session from a "
                                                 "checkout of the parent commit with its own library"}
    pathlib.Path(a.refit_out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.refit_out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
