#!/usr/bin/env python3
"""Time of the device BVH refit (include/srt_refit.h) against what it replaces, and what the refit tree costs a query.

Two meshes: Rubik and the 262k-triangle torus knot (the surface mesh of bench.py --full), each displaced by
srt_amd.render.wave_vertices at --wave (default: the amplitude the tests use).  One JSON line per mesh:

  refit_ms      srt_query_refit, from a torch.cuda.Event pair around --batch back-to-back calls on the object's stream,
                divided by the batch (--warmup batches unmeasured, median of --reps);
  recreate_ms   the path without it, host wall clock: srt_bvh_refit on the host arrays, srt_query_destroy, and
                srt_query_create with the same arrays (which synchronises).  Existing code, unchanged by the refit;
  closest_*     Mrays/s of srt_query_closest (tools/bench_queries.py's measure, surface rays of the deformed mesh) on
                the refit tree and on a tree REBUILT from the deformed triangles: a refit keeps the old topology, so
                its boxes overlap more.

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


def time_refit(torch, q, verts_dev, n_verts, batch, warmup, reps):
    from srt_amd import _lib

    lib, h, vp = _lib.lib(), q.handle, C.c_void_p(verts_dev.data_ptr())
    ext = torch.cuda.ExternalStream(int(lib.srt_query_stream(h)))

    def run():
        for _ in range(batch):
            rc = lib.srt_query_refit(h, vp, n_verts)
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
    return statistics.median(ms), min(ms), max(ms)


def time_recreate(scene, verts, warmup, reps):
    """Host refit of the nodes, destroy, create: the per-frame path of a deforming mesh without srt_query_refit."""
    import srt_amd as S
    from srt_amd import _lib

    lib = _lib.lib()

    def create(nodes):
        h = C.c_void_p()
        rc = lib.srt_query_create(0, None, S._ptr(scene.bvhs), len(scene.bvhs), S._ptr(nodes), len(nodes), S._ptr(scene.tris),
                                  len(scene.tris), S._ptr(verts), len(verts), C.byref(h))
        assert rc == _lib.SRT_OK, _lib.last_error()
        return h

    h = create(scene.nodes)
    ms = []
    for k in range(warmup + reps):
        nodes = scene.nodes.copy()
        t0 = time.perf_counter()
        rc = lib.srt_bvh_refit(S._ptr(scene.bvhs), len(scene.bvhs), S._ptr(nodes), len(nodes), S._ptr(scene.tris),
                               len(scene.tris), S._ptr(verts), len(verts))
        assert rc == _lib.SRT_OK, _lib.last_error()
        lib.srt_query_destroy(h)
        h = create(nodes)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            ms.append(dt)
    lib.srt_query_destroy(h)
    return statistics.median(ms), min(ms), max(ms)


def closest_rate(torch, q, rays_dev, warmup, reps):
    from bench_queries import time_calls
    from srt_amd import _lib

    lib, h, n = _lib.lib(), q.handle, rays_dev.shape[0]
    hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    rp, hp = C.c_void_p(rays_dev.data_ptr()), C.c_void_p(hits.data_ptr())
    with torch.cuda.stream(torch.cuda.ExternalStream(int(lib.srt_query_stream(h)))):
        med, lo, hi = time_calls(torch, lambda: lib.srt_query_closest(h, rp, n, hp), warmup, reps)
    torch.cuda.synchronize()
    return med, lo, hi, hits


def run(args):
    import torch

    import srt_amd as S
    from bench_queries import surface_rays
    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.query import Query

    results = []
    for name in ("rubik", "knot"):
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else R.torus_knot_model()
        scene = S.Scene.from_models([model])
        verts = R.wave_vertices(scene.verts, args.wave)
        refit = S.refit_scene(scene, verts)
        rebuilt = S.Scene.from_models([S.model_from_triangles(verts["pos"][scene.tris["v"]].reshape(-1, 9))])
        rays = torch.from_numpy(surface_rays(refit, args.rays).view(np.float32).reshape(-1, 8).copy()).cuda()
        vdev = torch.from_numpy(verts.view(np.float32).reshape(-1, 8).copy()).cuda()
        torch.cuda.synchronize()
        with Query(scene, refit=True) as qd, Query(rebuilt) as qb:
            r_med, r_min, r_max = time_refit(torch, qd, vdev, len(verts), args.batch, args.warmup, args.reps)
            qd.set_bvh_count(1)
            qb.set_bvh_count(1)
            d_med, d_min, d_max, hits_d = closest_rate(torch, qd, rays, args.warmup, args.reps)
            b_med, b_min, b_max, hits_b = closest_rate(torch, qb, rays, args.warmup, args.reps)
            # both trees hold the same fp32 triangles, so the closest distances agree in their bits, up to the rays
            # whose box entry distance rounds past a triangle's own t in one tree and not in the other (reported)
            t_differ = int((hits_d[:, 1] != hits_b[:, 1]).sum())
            info = {k: qd.get_int("refit." + k) for k in ("heights", "launches", "bytes")}
            hit_fraction = float((hits_d[:, 0] != -1).float().mean())
        c_med, c_min, c_max = time_recreate(scene, verts, args.warmup, args.reps)
        r = {"mesh": name, "triangles": len(scene.tris), "vertices": len(verts), "wave": args.wave,
             "refit_ms": round(r_med, 5), "refit_ms_min_max": [round(r_min, 5), round(r_max, 5)], "refit_batch": args.batch,
             "refit_heights": info["heights"], "refit_launches": info["launches"], "refit_bytes": info["bytes"],
             "recreate_ms": round(c_med, 4), "recreate_ms_min_max": [round(c_min, 4), round(c_max, 4)],
             "recreate_over_refit": round(c_med / r_med, 1),
             "rays": args.rays, "hit_fraction": round(hit_fraction, 4), "rays_t_differs_from_rebuilt": t_differ,
             "closest_refit_ms": round(d_med, 4), "closest_refit_ms_min_max": [round(d_min, 4), round(d_max, 4)],
             "closest_refit_mrays_s": round(args.rays / d_med / 1e3, 1),
             "closest_rebuilt_ms": round(b_med, 4), "closest_rebuilt_ms_min_max": [round(b_min, 4), round(b_max, 4)],
             "closest_rebuilt_mrays_s": round(args.rays / b_med / 1e3, 1),
             "refit_over_rebuilt_rate": round(b_med / d_med, 3), "warmup": args.warmup, "reps": args.reps}
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        doc = {"tool": "tools/bench_refit.py", "device": torch.cuda.get_device_name(0),
               "code_hash": _lib.lib().srt_code_hash().decode(),
               "timing": "refit: torch.cuda.Event pair around a batch of enqueued srt_query_refit calls on the object's "
                         "stream, per call; recreate: host wall clock of srt_bvh_refit + srt_query_destroy + srt_query_create; "
                         "closest: event pair around one enqueued srt_query_closest",
               "meshes": results}
        pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wave", type=float, default=WAVE_AMPLITUDE)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=20, help="srt_query_refit calls between two events")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", help="write the results to this JSON file")
    args = ap.parse_args()
    if args.warmup < 3 or args.reps < 10 or args.batch < 1:
        ap.error("at least 3 warm-up rounds and 10 measured ones")
    import torch  # noqa: F401  (before the library: one HIP runtime per process)

    run(args)


if __name__ == "__main__":
    main()
