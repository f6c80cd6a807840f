#!/usr/bin/env python3
"""Throughput of the ray-query service (include/srt_query.h) against the closest-hit test kernel it succeeds.

Four legs: {Rubik, the 262k-triangle torus knot} x {(a) the model camera's pixel-centre rays at
WIDTH x HEIGHT, (b) as many rays started on the surface in random directions}.  One JSON line per leg:
Mrays/s of srt_query_closest and srt_query_occluded from torch.cuda.Event pairs around the enqueued calls
(--warmup launches unmeasured, median of --reps).

The old closest_kernel only runs inside srt_trace_closest's host round trip, so its kernel-only time comes
from a profiler run of its own (no counters in it):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_queries.py --legacy
    python tools/bench_queries.py --legacy-trace DIR --out profiles/queries.json

--legacy traces every leg's rays LEGACY_REPS times through srt_trace_closest, in leg order; --legacy-trace
reads the closest_kernel dispatches of that run (median per leg) and reports legacy_ms / closest_ms.

--sorted times every leg through the sorted calls too (include/srt_query_sort.h), in the same process: per leg the
sorted totals beside the unsorted times, and the cost of the ordering alone (bounds + keys + sort) with the traversal
left out -- at bvh_count 0 the traversal kernel only writes every ray's miss record, so the sorted call minus the
unsorted call there is what the ordering adds.  --legs picks legs, --rebuild-leaf N measures on a device-rebuilt tree
(include/srt_rebuild_leaf.h).  The raw runs of DESIGN.md's "Sorted ray queries" are profiles/query_sort.json.
Nothing here is asserted: this is a measurement tool.
"""
from __future__ import annotations

import argparse
import csv
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGACY_REPS = 3
LEGS = [(scene, rays) for scene in ("rubik", "knot") for rays in ("camera", "surface")]


def camera_rays(setup, W, H):
    import srt_amd as S

    cam = setup.camera
    o = np.asarray(cam.getOrigin(), np.float32)
    right, up, front = (np.asarray(v, np.float32) for v in (cam.getRightVector(), cam.getUpVector(), cam.getForward()))
    du, dv = right / np.float32(W), up / np.float32(H)
    p00 = (o + front - right / 2 - up / 2) + np.float32(0.5) * (du + dv)
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    ps = p00 + x.reshape(-1, 1) * du + y.reshape(-1, 1) * dv
    rays = np.zeros(W * H, S.RAY_DTYPE)
    rays["o"] = o
    rays["d"] = (ps - o).astype(np.float32)
    rays["t"] = np.float32(1e30)
    return rays


def surface_rays(scene, n, seed=1234):
    import srt_amd as S

    rng = np.random.default_rng(seed)
    corners = scene.verts["pos"][scene.tris["v"][rng.integers(0, len(scene.tris), n)]].astype(np.float64)
    w = rng.dirichlet((1, 1, 1), n)
    d = rng.normal(size=(n, 3))
    rays = np.zeros(n, S.RAY_DTYPE)
    rays["o"] = (corners * w[:, :, None]).sum(1).astype(np.float32)
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["t"] = np.float32(1e30)
    return rays


def build_legs(W, H):
    from srt_amd import render as R

    out = {}
    for name in ("rubik", "knot"):
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else R.torus_knot_model()
        setup = R.make_setup(W, H, show_model=True, models=[model])
        out[(name, "camera")] = (setup.scene, camera_rays(setup, W, H))
        out[(name, "surface")] = (setup.scene, surface_rays(setup.scene, W * H))
    return out


def run_legacy(legs):
    import srt_amd as S

    for leg in LEGS:
        scene, rays = legs[leg]
        c = S.Compute().Init()
        try:
            c.bind_scene(scene)
            c.SetUInt("bvh_count", 1)
            for _ in range(LEGACY_REPS):
                hits, _ = c.trace_closest(rays)
        finally:
            c.close()
        print(json.dumps({"leg": "/".join(leg), "legacy_runs": LEGACY_REPS, "rays": len(rays),
                          "hit_fraction": round(float((hits != 0xFFFFFFFF).mean()), 4)}), flush=True)


def legacy_times(trace_dir):
    """Median closest_kernel duration (ms) per leg from a --legacy profiler run's kernel trace."""
    rows = []
    for f in pathlib.Path(trace_dir).rglob("*kernel_trace.csv"):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "closest_kernel" in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) != LEGACY_REPS * len(LEGS):
        raise SystemExit(f"{trace_dir}: {len(rows)} closest_kernel dispatches, expected {LEGACY_REPS * len(LEGS)}")
    ms = [(e - s) * 1e-6 for s, e in rows]
    return {leg: statistics.median(ms[i * LEGACY_REPS:(i + 1) * LEGACY_REPS]) for i, leg in enumerate(LEGS)}


def time_calls(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def sorted_times(torch, lib, q, h, rp, n, hp, op, args):
    """The sorted calls of one leg: the totals, and the ordering alone from the calls at bvh_count 0."""
    r = {}
    for name, fn, out in (("closest", lib.srt_query_closest_sorted, hp), ("occluded", lib.srt_query_occluded_sorted, op)):
        med, lo, hi = time_calls(torch, lambda: fn(h, rp, n, out), args.warmup, args.reps)
        r[f"{name}_sorted_ms"], r[f"{name}_sorted_ms_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        r[f"{name}_sorted_mrays_s"] = round(n / med / 1e3, 1)
    q.set_bvh_count(0)  # no BVH to walk: the traversal kernel writes the miss records and nothing else
    empty_sorted, _, _ = time_calls(torch, lambda: lib.srt_query_closest_sorted(h, rp, n, hp), args.warmup, args.reps)
    empty_plain, _, _ = time_calls(torch, lambda: lib.srt_query_closest(h, rp, n, hp), args.warmup, args.reps)
    q.set_bvh_count(1)
    lib.srt_query_closest_sorted(h, rp, n, hp)  # the hits the caller checks against `occ` are a sorted call's again
    r["sorted_empty_ms"], r["unsorted_empty_ms"] = round(empty_sorted, 4), round(empty_plain, 4)
    r["sort_ms"] = round(empty_sorted - empty_plain, 4)
    r.update({k: q.get_int(k) for k in ("sort.origin_bits", "sort.dir_bits", "sort.bytes", "sort.launches")})
    return r


def run_new(legs, args):
    import torch
    from srt_amd import _lib
    from srt_amd.query import Query
    import ctypes as C

    legacy = legacy_times(args.legacy_trace) if args.legacy_trace else {}
    results = []
    for leg in [l for l in LEGS if not args.legs or "/".join(l) in args.legs.split(",")]:
        scene, rays = legs[leg]
        n = len(rays)
        stream = torch.cuda.current_stream()
        kw = dict(refit=True, rebuild=True, rebuild_leaf=args.rebuild_leaf) if args.rebuild_leaf else {}
        with Query(scene, stream=stream.cuda_stream or None, **kw) as q:
            q.set_bvh_count(1)
            if args.rebuild_leaf:
                q.rebuild(torch.from_numpy(scene.verts.view(np.float32).reshape(-1, 8).copy()).cuda())
            dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
            hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
            occ = torch.empty((n,), dtype=torch.uint8, device="cuda")
            lib, h = _lib.lib(), q.handle
            rp, hp, op = C.c_void_p(dev.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(occ.data_ptr())
            if q._own_stream:  # torch's default stream: time on the object's own stream through events on it
                ext = torch.cuda.ExternalStream(int(lib.srt_query_stream(h)))
                ctx = torch.cuda.stream(ext)
            else:
                ctx = torch.cuda.stream(stream)
            with ctx:
                c_med, c_min, c_max = time_calls(torch, lambda: lib.srt_query_closest(h, rp, n, hp), args.warmup, args.reps)
                o_med, o_min, o_max = time_calls(torch, lambda: lib.srt_query_occluded(h, rp, n, op), args.warmup, args.reps)
                extra = sorted_times(torch, lib, q, h, rp, n, hp, op, args) if args.sorted else {}
            torch.cuda.synchronize()
            hit_fraction = float((hits[:, 0] != -1).float().mean())
            assert bool(((hits[:, 0] != -1) == (occ != 0)).all())
            r = {"leg": "/".join(leg), "rays": n, "triangles": len(scene.tris), "hit_fraction": round(hit_fraction, 4),
                 "closest_ms": round(c_med, 4), "closest_ms_min_max": [round(c_min, 4), round(c_max, 4)],
                 "closest_mrays_s": round(n / c_med / 1e3, 1),
                 "occluded_ms": round(o_med, 4), "occluded_ms_min_max": [round(o_min, 4), round(o_max, 4)],
                 "occluded_mrays_s": round(n / o_med / 1e3, 1),
                 "blocks": q.get_int("launch.blocks"), "refill_min": q.get_int("refill.min"),
                 "stack_entries": q.get_int("stack.entries"), "warmup": args.warmup, "reps": args.reps}
            if args.rebuild_leaf:
                r["rebuild_leaf"] = args.rebuild_leaf
            if extra:
                r.update(extra)
                r["sorted_over_unsorted"] = round(r["closest_sorted_ms"] / c_med, 3)
            if leg in legacy:
                r["legacy_closest_kernel_ms"] = round(legacy[leg], 4)
                r["legacy_over_closest"] = round(legacy[leg] / c_med, 3)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        doc = {"tool": "tools/bench_queries.py", "width": args.width, "height": args.height,
               "device": torch.cuda.get_device_name(0), "code_hash": _lib.lib().srt_code_hash().decode(),
               "timing": "torch.cuda.Event pairs around the enqueued call (memset of the claim counter + kernel); "
                         "legacy: closest_kernel dispatch durations of a rocprofv3 --kernel-trace run of --legacy",
               "legs": results}
        pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--legacy", action="store_true", help="run the rays through srt_trace_closest (for the profiler)")
    ap.add_argument("--legacy-trace", help="output directory of the profiler run of --legacy")
    ap.add_argument("--sorted", action="store_true", help="also time every leg through the sorted calls (srt_query_sort.h)")
    ap.add_argument("--legs", help="comma-separated legs to run (rubik/camera, rubik/surface, knot/camera, knot/surface)")
    ap.add_argument("--rebuild-leaf", type=int, default=0, help="measure on a device-rebuilt tree with this max_leaf")
    ap.add_argument("--out", help="write the legs to this JSON file")
    args = ap.parse_args()
    if args.warmup < 3 or args.reps < 10:
        ap.error("at least 3 warm-up launches and 10 measured ones")
    import torch  # noqa: F401  (before the library: one HIP runtime per process)

    legs = build_legs(args.width, args.height)
    if args.legacy:
        run_legacy(legs)
    else:
        run_new(legs, args)


if __name__ == "__main__":
    main()
