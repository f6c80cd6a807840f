#!/usr/bin/env python3
"""Time of the path tracer's device scene refit (include/srt_scene_refit.h) against the host path it replaces.

Two meshes: Rubik and the 262k-triangle torus knot (the surface mesh of bench.py --full), each displaced by
srt_amd.render.wave_vertices at --wave.  One JSON line per mesh:

  refit_ms        srt_scene_refit (flags 0) in the steady state, after the context's first render: from a
                  torch.cuda.Event pair around --batch back-to-back calls on the context's stream, divided by the
                  batch (--warmup batches unmeasured, median of --reps);
  host_path_ms    srt_bvh_refit on a copy of the host nodes, then srt_upload_scene of the result (which
                  synchronises): host wall clock, median and range.  --host-only measures nothing else and runs in
                  a checkout without the feature: profiles/scene_refit.json holds that run at the parent commit
                  beside this build's;
  frame_*_ms      host wall clock of one 1-spp frame at --width x --height, reset included, ended by srt_finish:
                  Compute.refit + render against refit_scene + bind_scene + render, the wave's phase advancing.

Nothing here is asserted: this is a measurement tool.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

WAVE_AMPLITUDE = 0.25  # tests/refit_ref.py
PHASE_STEP = 0.3       # tools/render.py WAVE_PHASE_STEP


def stats(ms):
    return round(statistics.median(ms), 5), [round(min(ms), 5), round(max(ms), 5)]


def time_refit(torch, c, vdev, batch, warmup, reps):
    from srt_amd import _lib

    lib, vp, n = _lib.lib(), C.c_void_p(vdev.data_ptr()), vdev.shape[0]
    ext = torch.cuda.ExternalStream(int(lib.srt_stream(c.ctx) or 0))

    def run():
        for _ in range(batch):
            rc = lib.srt_scene_refit(c._refit, vp, n, 0)
            assert rc == _lib.SRT_OK, _lib.last_error()

    ms = []
    with torch.cuda.stream(ext):
        for _ in range(warmup):
            run()
        ext.synchronize()
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / batch)
    return stats(ms)


def time_host_path(c, scene, verts, warmup, reps):
    import srt_amd as S
    from srt_amd import _lib

    lib = _lib.lib()
    tex = None if scene.sample_textures else np.ascontiguousarray(scene.tex_albedo, np.float32)
    ms = []
    for k in range(warmup + reps):
        nodes = scene.nodes.copy()
        t0 = time.perf_counter()
        rc = lib.srt_bvh_refit(S._ptr(scene.bvhs), len(scene.bvhs), S._ptr(nodes), len(nodes), S._ptr(scene.tris),
                               len(scene.tris), S._ptr(verts), len(verts))
        assert rc == _lib.SRT_OK, _lib.last_error()
        rc = lib.srt_upload_scene(c.ctx, S._ptr(scene.bvhs), len(scene.bvhs), S._ptr(nodes), len(nodes), S._ptr(scene.mats),
                                  S._ptr(tex), len(scene.mats), S._ptr(scene.tris), len(scene.tris), S._ptr(verts), len(verts))
        assert rc == _lib.SRT_OK, _lib.last_error()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            ms.append(dt)
    return stats(ms)


def time_frames(torch, r, scene, wave, device_refit, warmup, reps):
    import srt_amd as S
    from srt_amd import render as R

    c = r.compute
    c.bind_scene(scene, refit=device_refit)
    ms = []
    for k in range(warmup + reps):
        verts = R.wave_vertices(scene.verts, wave, PHASE_STEP * k)
        vdev = torch.from_numpy(np.ascontiguousarray(verts).view(np.float32).reshape(-1, 8)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if device_refit:
            c.refit(vdev)
        else:
            c.bind_scene(S.refit_scene(scene, verts))
        r.render(1)
        r.finish()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            ms.append(dt)
    return stats(ms)


def run(args):
    import torch

    import srt_amd as S
    from srt_amd import _lib
    from srt_amd import render as R

    results = []
    for name in ("rubik", "knot"):
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else R.torus_knot_model()
        setup = R.make_setup(args.width, args.height, show_model=True, models=[model])
        scene = setup.scene
        verts = R.wave_vertices(scene.verts, args.wave)
        rdr = R.Renderer(setup)
        try:
            c = rdr.compute
            res = {"mesh": name, "triangles": len(scene.tris), "vertices": len(verts), "wave": args.wave}
            res["host_path_ms"], res["host_path_ms_min_max"] = time_host_path(c, scene, verts, args.warmup, args.reps)
            if not args.host_only:
                c.bind_scene(scene, refit=True)
                rdr.render(1)  # the context's first pipelined launch creates the slot streams: a refit before it
                rdr.finish()   # waits for its own kernels (srt_scene_refit.h), the steady state only enqueues
                vdev = torch.from_numpy(verts.view(np.float32).reshape(-1, 8).copy()).cuda()
                torch.cuda.synchronize()
                res["refit_ms"], res["refit_ms_min_max"] = time_refit(torch, c, vdev, args.batch, args.warmup, args.reps)
                res["refit_batch"] = args.batch
                for k in ("launches", "heights", "bytes", "treelets"):
                    res["refit_" + k] = c.refit_get_int("refit." + k)
                res["host_path_over_refit"] = round(res["host_path_ms"] / res["refit_ms"], 1)
                res["frame"] = [args.width, args.height, 1]
                res["frame_device_refit_ms"], res["frame_device_refit_ms_min_max"] = time_frames(
                    torch, rdr, scene, args.wave, True, args.warmup, args.reps)
                res["frame_host_path_ms"], res["frame_host_path_ms_min_max"] = time_frames(
                    torch, rdr, scene, args.wave, False, args.warmup, args.reps)
                res["frame_host_over_device"] = round(res["frame_host_path_ms"] / res["frame_device_refit_ms"], 2)
            res["warmup"], res["reps"] = args.warmup, args.reps
        finally:
            rdr.close()
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        doc = {"tool": "tools/bench_scene_refit.py", "device": torch.cuda.get_device_name(0),
               "code_hash": _lib.lib().srt_code_hash().decode(),
               "timing": "refit: torch.cuda.Event pair around a batch of enqueued srt_scene_refit calls on the context's "
                         "stream, per call; host path: host wall clock of srt_bvh_refit + srt_upload_scene; frames: host "
                         "wall clock from the refit (or refit_scene + bind_scene) to the end of srt_finish, 1 spp",
               "meshes": results}
        pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wave", type=float, default=WAVE_AMPLITUDE)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=20, help="srt_scene_refit calls between two events")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-only", action="store_true",
                    help="only srt_bvh_refit + srt_upload_scene: what a checkout without the feature can run")
    ap.add_argument("--out", help="write the results to this JSON file")
    args = ap.parse_args()
    if args.warmup < 3 or args.reps < 10 or args.batch < 1:
        ap.error("at least 3 warm-up rounds and 10 measured ones")
    import torch  # noqa: F401  (before the library: one HIP runtime per process)

    run(args)


if __name__ == "__main__":
    main()
