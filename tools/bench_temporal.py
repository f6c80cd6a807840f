#!/usr/bin/env python3
"""Time of the temporal reprojection (include/srt_temporal.h) on a rendered Rubik frame at WIDTH x HEIGHT.

It times srt_temporal_accumulate by torch.cuda.Event pairs around the enqueued call (--warmup runs unmeasured,
median of --reps), in three states: without history (the first call after a reset: no taps), with the history of
the same camera (every hit pixel gathers its four taps), and with the history of a camera one small step away
(the interactive case: most hit pixels gather, the taps are no longer aligned with the lanes).  Beside them, timed
the same way in the same process: a float4 copy of one frame (the bandwidth floor) and one a-trous pass of the
denoiser (srt_denoise_run with passes = 1), which the call is to be read against.
Nothing is asserted: this is a measurement tool.  --out writes the JSON document (profiles/temporal.json).

--motion-out (profiles/temporal_motion.json) adds the moving-model instance (include/srt_temporal_motion.h), timed
the same way after the rows above: the call with one pose stated and unchanged (every record static: the upload
launch plus the motion kernel), the call with the cube turned by --spin degrees since the previous frame (guides
queried under each pose), the static instance once more beside them, and the upload launches by themselves as
nearly as the interface allows: a 1 x 1 object's call with 0, 1 and 256 poses (its one-pixel kernel is the rest).

--deform-out (profiles/temporal_deform.json) measures the deforming-mesh instances (include/srt_temporal_deform.h) by
themselves: per scene (Rubik and the 262,144-triangle knot) frames under `wave` with an advancing phase, the guide
from a refit query per phase; ms per frame of the deform instance without and with moments (each includes its copy of
V into V'), the copy nearly by itself (a 1 x 1 object's call over the same mesh), and the motion instance on the same
frames.  --deform-baseline-only writes only the motion-instance rows and uses nothing this header added, so the same
script run from a checkout of the parent commit gives the baseline; --deform-baseline FILE folds that file in.
--resource-usage FILE (hipcc -Rpass-analysis=kernel-resource-usage of csrc/temporal.hip) supplies the occupancy.
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
    ap.add_argument("--motion-out", help="also time the moving-model instance and write its rows to this JSON file")
    ap.add_argument("--spin", type=float, default=2.0, help="degrees the cube turns per frame in the moving rows")
    ap.add_argument("--deform-out", help="time the deforming-mesh instances only and write their rows to this JSON file")
    ap.add_argument("--deform-baseline-only", action="store_true", help="with --deform-out: the motion-instance rows only")
    ap.add_argument("--deform-baseline", help="with --deform-out: a --deform-baseline-only file of the parent commit to fold in")
    ap.add_argument("--resource-usage", help="with --deform-out: the compiler's kernel-resource-usage remarks of temporal.hip")
    ap.add_argument("--wave", type=float, default=0.014, help="--deform-out: the wave's amplitude as a share of the bounds' extent")
    a = ap.parse_args()
    if a.warmup < 3 or a.reps < 10:
        ap.error("at least 3 warm-up runs and 10 measured ones")
    if a.deform_out:
        return deform_main(a)
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
    doc = {"tool": "tools/bench_temporal.py", "width": W, "height": H, "spp": a.spp, "scene": "rubik",
           "device": torch.cuda.get_device_name(0), "code_hash": lib.srt_code_hash().decode(),
           "warmup": a.warmup, "reps": a.reps,
           "timing": "torch.cuda.Event pairs around the enqueued call on one stream; median [min, max] ms; the "
                     "calls that set a state up (reset, the previous frame) are enqueued before the first event"}
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
            with Query(setup.scene, stream=stream) as q, Denoiser(W, H, stream=stream) as dn, \
                    Temporal(W, H, stream=stream) as tp:
                q.set_bvh_count(setup.bvh_count)
                cam0 = _camera(setup.camera)
                hits0 = q.closest(dn.primary_rays(setup.camera))
                setup.camera.MoveRight(0.5)
                setup.camera.Rotate(-1.0, 0.0)
                cam1 = _camera(setup.camera)
                hits1 = q.closest(dn.primary_rays(setup.camera))
                doc["hit_fraction"] = round(float(hits0.hit.float().mean()), 4)
                doc["scratch_bytes"] = tp.get_int("scratch.bytes")
                # bytes a call must move per pixel: accum 16 + srt_hit 32 read; out 16 + history 16 + 16 + 4 written;
                # a hit pixel with history also gathers 4 x 36 B, mostly shared with its neighbours through the caches
                doc["bytes_min_per_pixel"] = 100

                def call(hits, cam):
                    return lib.srt_temporal_accumulate(tp.handle, C.c_void_p(acc_ptr), frames, C.c_void_p(hits.raw.data_ptr()),
                                                       C.byref(cam), C.c_void_p(out.data_ptr()))

                doc["accumulate_no_history_ms"] = time_calls(torch, lambda: call(hits0, cam0), a.warmup, a.reps,
                                                             before=lambda: lib.srt_temporal_reset(tp.handle))
                doc["accumulate_same_camera_ms"] = time_calls(torch, lambda: call(hits0, cam0), a.warmup, a.reps)
                doc["accumulate_moved_camera_ms"] = time_calls(torch, lambda: call(hits1, cam1), a.warmup, a.reps,
                                                               before=lambda: call(hits0, cam0))
                tp.synchronize()
                n = out[..., 3]
                doc["moved_camera_reuse_fraction_of_hits"] = round(float((n[hits1.hit.reshape(H, W)] >= 2).float().mean()), 4)
                dn.set_params(passes=1)
                out2 = torch.empty_like(out)
                doc["atrous_one_pass_ms"] = time_calls(
                    torch, lambda: lib.srt_denoise_run(dn.handle, C.c_void_p(acc_ptr), frames, C.c_void_p(hits0.raw.data_ptr()),
                                                       C.c_void_p(out2.data_ptr()), None), a.warmup, a.reps)
                # the same three once more: the first series of a process reads slow ("Denoiser")
                doc["second_series"] = {
                    "copy_float4_frame_ms": time_calls(torch, lambda: out2.copy_(src), a.warmup, a.reps),
                    "accumulate_same_camera_ms": time_calls(torch, lambda: call(hits0, cam0), a.warmup, a.reps),
                    "accumulate_moved_camera_ms": time_calls(torch, lambda: call(hits1, cam1), a.warmup, a.reps,
                                                             before=lambda: call(hits0, cam0)),
                }
                if a.motion_out:
                    motion = motion_rows(torch, a, doc, setup, q, dn, tp, call, cam0, hits0, time_calls)
        m = doc["second_series"]["accumulate_moved_camera_ms"][0]
        doc["moved_over_copy"] = round(m / doc["second_series"]["copy_float4_frame_ms"][0], 2)
        doc["moved_over_atrous_pass"] = round(m / doc["atrous_one_pass_ms"][0], 2)
        doc["moved_min_bytes_GBps"] = round(W * H * doc["bytes_min_per_pixel"] / (m * 1e-3) / 1e9, 1)
    finally:
        rdr.close()
    print(json.dumps(doc), flush=True)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    if a.motion_out:
        print(json.dumps(motion), flush=True)
        pathlib.Path(a.motion_out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.motion_out).write_text(json.dumps(motion, indent=1) + "\n")


def motion_rows(torch, a, doc, setup, q, dn, tp, call, cam0, hits0, time_calls):
    """The rows of --motion-out; `call(hits, cam)` enqueues srt_temporal_accumulate on `tp`."""
    import numpy as np

    from srt_amd import _lib
    from srt_amd.temporal import Temporal

    W, H = a.width, a.height
    v = setup.scene.verts["pos"].astype(np.float64)
    centre = (v.min(0) + v.max(0)) / 2

    def frame_of(deg):  # world -> model with the cube turned by `deg` about the vertical axis through its centre
        c, s = np.cos(np.radians(-deg)), np.sin(np.radians(-deg))
        m = np.eye(4)
        m[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        m[:3, 3] = centre - m[:3, :3] @ centre
        return m.T.reshape(16).astype(np.float32)

    frames = [frame_of(0.0), frame_of(a.spin)]
    hits = []
    for f in frames:
        q.update_model_matrix(0, f)
        hits.append(q.closest(dn.primary_rays(setup.camera)))
    q.update_model_matrix(0, frames[0])
    out = {k: doc[k] for k in ("tool", "width", "height", "scene", "device", "code_hash", "warmup", "reps", "timing")}
    out["spin_degrees"] = a.spin
    out["records"] = 1

    def moved_before():
        tp.set_models([frames[0]])
        call(hits[0], cam0)
        tp.set_models([frames[1]])

    series = []
    for _ in range(2):  # twice: the spread between the series is the run-to-run spread the rows are read against
        row = {}
        tp.set_models([])
        row["static_instance_same_camera_ms"] = time_calls(torch, lambda: call(hits0, cam0), a.warmup, a.reps)
        tp.set_models([frames[0]])
        row["motion_instance_all_static_ms"] = time_calls(torch, lambda: call(hits0, cam0), a.warmup, a.reps)
        row["motion_instance_cube_moving_ms"] = time_calls(torch, lambda: call(hits[1], cam0), a.warmup, a.reps,
                                                           before=moved_before)
        tp.synchronize()
        series.append(row)
    out["series"] = series
    moved_before()  # the share of the moved frame's hit pixels that found history
    res = tp.accumulate(torch.ones((H, W, 4), dtype=torch.float32, device="cuda"), 1, hits[1],
                        [list(getattr(cam0, n)) for n in ("origin", "front", "right", "up")])
    tp.synchronize()
    out["cube_moving_reuse_fraction_of_hits"] = round(float((res[..., 3][hits[1].hit.reshape(H, W)] >= 2).float().mean()), 4)
    tp.set_models([])
    with Temporal(1, 1, stream=torch.cuda.current_stream()) as tiny:
        acc1 = torch.ones((1, 1, 4), dtype=torch.float32, device="cuda")
        out1 = torch.empty_like(acc1)
        hit1 = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
        for n_poses in (0, 1, 256):
            tiny.set_models([frames[0]] * n_poses)
            out[f"tiny_object_{n_poses}_poses_ms"] = time_calls(
                torch, lambda: _lib.lib().srt_temporal_accumulate(tiny.handle, C.c_void_p(acc1.data_ptr()), 1,
                                                                  C.c_void_p(hit1.data_ptr()), C.byref(cam0),
                                                                  C.c_void_p(out1.data_ptr())), a.warmup, a.reps)
            out[f"tiny_object_{n_poses}_poses_launches"] = tiny.get_int("launches")
    return out


def occupancy_of(path):
    """{kernel: [VGPRs, waves per SIMD]} of the two deform instances from hipcc's kernel-resource-usage remarks."""
    import re

    out, name = {}, None
    for line in pathlib.Path(path).read_text().splitlines():
        if "Function Name:" in line:
            m = re.search(r"(temporal_accumulate_\w+?_kernel)E", line)
            name = m.group(1) if m else None
        m = re.search(r"\bVGPRs: (\d+)", line)
        if m and name:
            out.setdefault(name, [0, 0])[0] = int(m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            out.setdefault(name, [0, 0])[1] = int(m.group(1))
    return {k: v for k, v in out.items() if "deform" in k or "motion" in k}


def deform_main(a):
    """--deform-out: see the module docstring."""
    import numpy as np
    import torch

    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.temporal import Temporal, _camera

    W, H = a.width, a.height
    lib = _lib.lib()
    full = not a.deform_baseline_only
    doc = {"tool": "tools/bench_temporal.py --deform-out", "width": W, "height": H, "device": torch.cuda.get_device_name(0),
           "code_hash": lib.srt_code_hash().decode(), "warmup": a.warmup, "reps": a.reps, "phase_step": 0.3,
           "timing": "torch.cuda.Event pairs around the enqueued call on one stream; median [min, max] ms; the previous "
                     "frame (set_vertices + accumulate at the previous phase) is enqueued before the first event",
           "scenes": []}
    ident = np.eye(4, dtype=np.float32).reshape(16)
    for name in ("rubik", "knot"):
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else R.torus_knot_model()
        setup = R.make_setup(W, H, show_model=True, models=[model])
        scene = setup.scene
        extent = float(np.ptp(scene.verts["pos"], axis=0).max())
        row = {"scene": name, "triangles": len(scene.tris), "vertices": len(scene.verts), "wave_amplitude": round(a.wave * extent, 4)}
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream), Query(scene, stream=stream, refit=True) as q, Denoiser(W, H, stream=stream) as dn, \
                Temporal(W, H, stream=stream) as tp:
            q.set_bvh_count(setup.bvh_count)
            cam = _camera(setup.camera)
            rays = dn.primary_rays(setup.camera)
            verts, hits = [], []
            for k in range(2):
                v = R.wave_vertices(scene.verts, a.wave * extent, 0.3 * k)
                verts.append(torch.from_numpy(np.ascontiguousarray(v).view(np.float32).reshape(-1, 8)).cuda())
                q.refit(verts[-1])
                hits.append(q.closest(rays))
            acc = torch.rand((H, W, 4), dtype=torch.float32, device="cuda")
            out, mom = torch.empty_like(acc), torch.empty_like(acc)
            row["hit_fraction"] = round(float(hits[1].hit.float().mean()), 4)

            def call(t, k, moments=False):
                if moments:
                    return lib.srt_temporal_accumulate_moments(t.handle, C.c_void_p(acc.data_ptr()), 1, C.c_void_p(hits[k].raw.data_ptr()),
                                                               C.byref(cam), C.c_void_p(out.data_ptr()), C.c_void_p(mom.data_ptr()))
                return lib.srt_temporal_accumulate(t.handle, C.c_void_p(acc.data_ptr()), 1, C.c_void_p(hits[k].raw.data_ptr()),
                                                   C.byref(cam), C.c_void_p(out.data_ptr()))

            def reuse():
                tp.synchronize()
                return round(float((out[..., 3][hits[1].hit.reshape(H, W)] >= 2).float().mean()), 4)

            tp.enable_moments()
            tp.set_models([ident])  # one pose, unchanged: the motion instance, every record static
            for moments, key in ((False, "motion_instance_ms"), (True, "motion_moments_instance_ms")):
                row[key] = time_calls(torch, lambda: call(tp, 1, moments), a.warmup, a.reps, before=lambda: call(tp, 0, moments))
            row["motion_instance_launches"] = tp.get_int("launches")
            row["motion_instance_reuse_fraction_of_hits"] = reuse()
            if full:
                tp.set_mesh(scene)
                for moments, key in ((False, "deform_instance_ms"), (True, "deform_moments_instance_ms")):
                    def before():
                        tp.set_vertices(verts[0])
                        call(tp, 0, moments)
                        tp.set_vertices(verts[1])
                    row[key] = time_calls(torch, lambda: call(tp, 1, moments), a.warmup, a.reps, before=before)
                row["deform_instance_launches"] = tp.get_int("launches")
                row["deform_instance_reuse_fraction_of_hits"] = reuse()
                row["mesh_bytes"] = tp.get_int("mesh.bytes")
                tp.set_vertices(None)
                with Temporal(1, 1, stream=stream) as tiny:  # a one-pixel kernel and the copy of the whole mesh's positions
                    a1 = torch.ones((1, 1, 4), dtype=torch.float32, device="cuda")
                    o1, h1 = torch.empty_like(a1), torch.zeros((1, 8), dtype=torch.int32, device="cuda")
                    fn = lambda: lib.srt_temporal_accumulate(tiny.handle, C.c_void_p(a1.data_ptr()), 1, C.c_void_p(h1.data_ptr()),  # noqa: E731
                                                             C.byref(cam), C.c_void_p(o1.data_ptr()))
                    row["tiny_object_no_mesh_ms"] = time_calls(torch, fn, a.warmup, a.reps)
                    tiny.set_mesh(scene)
                    tiny.set_vertices(verts[1])
                    row["tiny_object_with_copy_ms"] = time_calls(torch, fn, a.warmup, a.reps)
                    row["copy_bytes"] = 32 * len(scene.verts)
        print(json.dumps(row), flush=True)
        doc["scenes"].append(row)
    if full and a.resource_usage:
        doc["vgprs_and_waves_per_simd"] = occupancy_of(a.resource_usage)
        doc["occupancy_source"] = "hipcc -Rpass-analysis=kernel-resource-usage, gfx950"
    if full and a.deform_baseline:
        base = json.loads(pathlib.Path(a.deform_baseline).read_text())
        doc["parent_commit_baseline"] = {"code_hash": base["code_hash"], "scenes": base["scenes"],
                                         "what": "the same script with --deform-baseline-only, run in the same session from a "
                                                 "checkout of the parent commit with its own library"}
    pathlib.Path(a.deform_out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.deform_out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
