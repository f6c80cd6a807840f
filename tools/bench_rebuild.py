#!/usr/bin/env python3
"""Time of the device BVH rebuild (include/srt_rebuild.h) against the host path it replaces, and what each tree costs a
query.

Two meshes: Rubik and the 262k-triangle torus knot (the surface mesh of bench.py --full), displaced by
srt_amd.render.wave_vertices.  One JSON line per mesh:

  rebuild_ms        srt_query_rebuild, from a torch.cuda.Event pair around --batch back-to-back calls on the object's
                    stream, divided by the batch (each call synchronises once, so the pair spans that wait too), and the
                    host wall clock of the same calls; with the launches of one rebuild and the tree's depth;
  host_rebuild_ms   the path without it, host wall clock: the vertices read back, the midpoint tree built on the host,
                    srt_query_destroy and srt_query_create;
  closest, per amplitude: Mrays/s of srt_query_closest (tools/bench_queries.py's surface rays of the deformed mesh) on
                    three trees over the same vertices -- the refit rest-pose tree, the device LBVH, the midpoint tree
                    built on the host.  The amplitude doubles from --wave until the refit tree's rate falls under
                    --degraded of the midpoint tree's (or 4 doublings);
  remap_ms          the hit remap of a rebuilt object per --rays hits: srt_query_closest on the rebuilt object minus the
                    same call on an object created from the host-built LBVH arrays (the same tree, no remap).

With --leaf 1,2,4,8 (include/srt_rebuild_leaf.h) the tool measures the leaf collapse instead, one JSON line per mesh:
per max_leaf the rebuild time as above, --repeat times over (the spread of those medians is the run-to-run noise), with
the pairs, the depth and stack.in_hbm of the tree; and at the amplitudes of --waves the rate of srt_query_closest on the
refit tree, the midpoint tree and the device LBVH of every max_leaf.  max_leaf 1 never calls the setting, so that column
is the object a caller has without it.

With --models (include/srt_rebuild_models.h) the scene is Rubik beside the knot, two BVH records, and the tool prints one
JSON line: per max_leaf of --leaf (default 1,4) the time of srt_query_rebuild on the two-record object as above, --repeat
times over on fresh objects, beside the one-record rebuilds of Rubik and of the knot alone and their sum; the host path
(readback, a midpoint tree per record built on the host, destroy, create); and the rate of srt_query_closest on the refit
tree, the host midpoint trees and the device trees of every max_leaf.

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


def time_rebuild(torch, q, verts_dev, n_verts, batch, warmup, reps):
    from srt_amd import _lib

    lib, h, vp = _lib.lib(), q.handle, C.c_void_p(verts_dev.data_ptr())
    ext = torch.cuda.ExternalStream(int(lib.srt_query_stream(h)))

    def run():
        for _ in range(batch):
            rc = lib.srt_query_rebuild(h, vp, n_verts)
            assert rc == _lib.SRT_OK, _lib.last_error()

    ms, wall = [], []
    with torch.cuda.stream(ext):
        for _ in range(warmup):
            run()
        ext.synchronize()
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            run()
            wall.append((time.perf_counter() - t0) * 1e3 / batch)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / batch)
    return (statistics.median(ms), min(ms), max(ms)), statistics.median(wall)


def midpoint_scene(S, scene, pos):
    return S.Scene.from_models([S.model_from_triangles(pos[scene.tris["v"]].reshape(-1, 9))])


def time_host_rebuild(torch, S, scene, verts_dev, warmup, reps):
    from srt_amd import _lib

    lib = _lib.lib()

    def create(s):
        h = C.c_void_p()
        rc = lib.srt_query_create(0, None, S._ptr(s.bvhs), len(s.bvhs), S._ptr(s.nodes), len(s.nodes), S._ptr(s.tris), len(s.tris),
                                  S._ptr(s.verts), len(s.verts), C.byref(h))
        assert rc == _lib.SRT_OK, _lib.last_error()
        return h

    h = create(scene)
    ms, build = [], []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        pos = verts_dev.cpu().numpy()[:, :3]
        t1 = time.perf_counter()
        built = midpoint_scene(S, scene, pos)
        t2 = time.perf_counter()
        lib.srt_query_destroy(h)
        h = create(built)
        t3 = time.perf_counter()
        if k >= warmup:
            ms.append((t3 - t0) * 1e3)
            build.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    lib.srt_query_destroy(h)
    parts = [round(statistics.median(x), 4) for x in zip(*build)]
    return statistics.median(ms), min(ms), max(ms), parts


def run(args):
    import torch

    import srt_amd as S
    from bench_queries import surface_rays
    from bench_refit import closest_rate
    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.query import Query

    def dev(a):
        return torch.from_numpy(a.view(np.float32).reshape(-1, 8).copy()).cuda()

    results = []
    for name in ("rubik", "knot"):
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else R.torus_knot_model()
        scene = S.Scene.from_models([model])
        verts = R.wave_vertices(scene.verts, args.wave)
        vdev = dev(verts)
        torch.cuda.synchronize()
        with Query(scene, refit=True, rebuild=True) as q:
            (b_med, b_min, b_max), b_wall = time_rebuild(torch, q, vdev, len(verts), args.batch, args.warmup, args.reps)
            info = {k: q.get_int(k) for k in ("rebuild.launches", "rebuild.depth", "rebuild.bytes", "refit.launches", "stack.in_hbm")}
        h_med, h_min, h_max, parts = time_host_rebuild(torch, S, scene, vdev, args.warmup, args.reps)
        r = {"mesh": name, "triangles": len(scene.tris), "vertices": len(verts), "wave": args.wave,
             "rebuild_ms": round(b_med, 5), "rebuild_ms_min_max": [round(b_min, 5), round(b_max, 5)],
             "rebuild_wall_ms": round(b_wall, 5), "rebuild_batch": args.batch, **{k.replace(".", "_"): v for k, v in info.items()},
             "host_rebuild_ms": round(h_med, 4), "host_rebuild_ms_min_max": [round(h_min, 4), round(h_max, 4)],
             "host_readback_build_recreate_ms": parts, "host_over_device": round(h_med / b_med, 1),
             "rays": args.rays, "closest": [], "warmup": args.warmup, "reps": args.reps}
        amplitude = args.wave
        for _ in range(5):
            v = R.wave_vertices(scene.verts, amplitude)
            refit = S.refit_scene(scene, v)
            rays = dev(surface_rays(refit, args.rays))
            vd = dev(v)
            lbvh_host, _ = S.build_lbvh(scene, v)
            row = {"wave": amplitude}
            with Query(scene, refit=True) as qr, Query(scene, refit=True, rebuild=True) as ql, \
                    Query(midpoint_scene(S, scene, v["pos"])) as qm, Query(lbvh_host) as qh:
                qr.refit(vd)
                ql.rebuild(vd)
                for key, qq in (("refit", qr), ("lbvh", ql), ("midpoint", qm), ("lbvh_no_remap", qh)):
                    qq.set_bvh_count(1)
                    med, lo, hi, hits = closest_rate(torch, qq, rays, args.warmup, args.reps)
                    row[key + "_ms"] = round(med, 4)
                    row[key + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
                    row[key + "_mrays_s"] = round(args.rays / med / 1e3, 1)
                    row[key + "_stack_in_hbm"] = qq.get_int("stack.in_hbm")
                row["lbvh_depth"] = ql.get_int("rebuild.depth")
            row["remap_ms"] = round(row["lbvh_ms"] - row["lbvh_no_remap_ms"], 4)
            row["refit_over_midpoint_rate"] = round(row["midpoint_ms"] / row["refit_ms"], 3)
            row["lbvh_over_midpoint_rate"] = round(row["midpoint_ms"] / row["lbvh_ms"], 3)
            row["lbvh_over_refit_rate"] = round(row["refit_ms"] / row["lbvh_ms"], 3)
            r["closest"].append(row)
            if row["refit_over_midpoint_rate"] < args.degraded:
                break
            amplitude *= 2
        r["degraded_wave"] = r["closest"][-1]["wave"]
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        doc = {"tool": "tools/bench_rebuild.py", "device": torch.cuda.get_device_name(0),
               "code_hash": _lib.lib().srt_code_hash().decode(),
               "timing": "rebuild: torch.cuda.Event pair around a batch of srt_query_rebuild calls on the object's stream, per "
                         "call (each call synchronises once), and the host wall clock of the same calls; host rebuild: host wall "
                         "clock of the vertex readback + srt_model_from_triangles + srt_scene_build + srt_query_destroy + "
                         "srt_query_create; closest: event pair around one enqueued srt_query_closest",
               "meshes": results}
        pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def run_leaf(args):
    import torch

    import srt_amd as S
    from bench_queries import surface_rays
    from bench_refit import closest_rate
    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.query import Query

    def dev(a):
        return torch.from_numpy(a.view(np.float32).reshape(-1, 8).copy()).cuda()

    def tree(q):
        return {"pairs": q.get_int("layout.pairs") // 64, "depth": q.get_int("rebuild.depth"), "stack_in_hbm": q.get_int("stack.in_hbm"),
                "launches": q.get_int("rebuild.launches")}

    results = []
    for name in ("rubik", "knot"):
        model = R.rubik_model(ROOT / "tests" / "golden" / "objects") if name == "rubik" else R.torus_knot_model()
        scene = S.Scene.from_models([model])
        verts = R.wave_vertices(scene.verts, args.wave)
        vdev = dev(verts)
        torch.cuda.synchronize()
        r = {"mesh": name, "triangles": len(scene.tris), "vertices": len(verts), "wave": args.wave, "rebuild_batch": args.batch,
             "rebuild": [], "rays": args.rays, "closest": [], "warmup": args.warmup, "reps": args.reps, "repeat": args.repeat}
        for leaf in args.leaf:
            runs = []
            for _ in range(args.repeat):  # a fresh object each time: the spread of the medians is the noise
                with Query(scene, refit=True, rebuild=True) as q:
                    if leaf != 1:
                        q.set_rebuild_leaf(leaf)
                    (med, lo, hi), wall = time_rebuild(torch, q, vdev, len(verts), args.batch, args.warmup, args.reps)
                    runs.append({"ms": round(med, 5), "ms_min_max": [round(lo, 5), round(hi, 5)], "wall_ms": round(wall, 5)})
                    info = tree(q)
            meds = [x["ms"] for x in runs]
            r["rebuild"].append({"max_leaf": leaf, "rebuild_ms": round(statistics.median(meds), 5),
                                 "rebuild_ms_runs": meds, "runs": runs, **info})
        for amplitude in args.waves:
            v = R.wave_vertices(scene.verts, amplitude)
            refit = S.refit_scene(scene, v)
            rays = dev(surface_rays(refit, args.rays))
            vd = dev(v)
            row = {"wave": amplitude, "lbvh": []}
            with Query(scene, refit=True) as qr, Query(midpoint_scene(S, scene, v["pos"])) as qm:
                qr.refit(vd)
                for key, qq in (("refit", qr), ("midpoint", qm)):
                    qq.set_bvh_count(1)
                    med, lo, hi, _ = closest_rate(torch, qq, rays, args.warmup, args.reps)
                    row[key] = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                                "mrays_s": round(args.rays / med / 1e3, 1), "stack_in_hbm": qq.get_int("stack.in_hbm"),
                                "pairs": qq.get_int("layout.pairs") // 64, "depth": qq.get_int("stack.entries") - 1}
            for leaf in args.leaf:
                with Query(scene, refit=True, rebuild=True) as ql:
                    if leaf != 1:
                        ql.set_rebuild_leaf(leaf)
                    ql.rebuild(vd)
                    ql.set_bvh_count(1)
                    med, lo, hi, _ = closest_rate(torch, ql, rays, args.warmup, args.reps)
                    row["lbvh"].append({"max_leaf": leaf, "ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                                        "mrays_s": round(args.rays / med / 1e3, 1),
                                        "over_midpoint_rate": round(row["midpoint"]["ms"] / med, 3),
                                        "over_refit_rate": round(row["refit"]["ms"] / med, 3), **tree(ql)})
            r["closest"].append(row)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        doc = {"tool": "tools/bench_rebuild.py --leaf " + ",".join(str(x) for x in args.leaf), "device": torch.cuda.get_device_name(0),
               "code_hash": _lib.lib().srt_code_hash().decode(),
               "timing": "rebuild: torch.cuda.Event pair around a batch of srt_query_rebuild calls on the object's stream, per call "
                         "(each call synchronises once); the median of --reps such batches, --repeat times over on fresh objects; "
                         "closest: event pair around one enqueued srt_query_closest",
               "meshes": results}
        pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def run_models(args):
    import torch

    import srt_amd as S
    from bench_queries import surface_rays
    from bench_refit import closest_rate
    from srt_amd import _lib
    from srt_amd import render as R
    from srt_amd.query import Query

    def dev(a):
        return torch.from_numpy(a.view(np.float32).reshape(-1, 8).copy()).cuda()

    def timed(scene, vdev, leaf, models):
        runs, info = [], {}
        for _ in range(args.repeat):  # a fresh object each time: the spread of the medians is the noise
            with Query(scene, refit=True, rebuild=not models, rebuild_models=models) as q:
                if leaf != 1:
                    q.set_rebuild_leaf(leaf)
                (med, _, _), _ = time_rebuild(torch, q, vdev, vdev.shape[0], args.batch, args.warmup, args.reps)
                runs.append(round(med, 5))
                info = {"pairs": q.get_int("rebuild.pairs"), "depth": q.get_int("rebuild.depth"),
                        "launches": q.get_int("rebuild.launches"), "records": q.get_int("rebuild.records")}
        return {"rebuild_ms": round(statistics.median(runs), 5), "rebuild_ms_runs": runs, **info}

    models = [R.rubik_model(ROOT / "tests" / "golden" / "objects"), R.torus_knot_model()]
    scene = S.Scene.from_models(models)
    alone = [S.Scene.from_models([m]) for m in models]
    verts = R.wave_vertices(scene.verts, args.wave)
    vdev = dev(verts)
    leaves = args.leaf or [1, 4]
    r = {"scene": "rubik+knot", "records": len(scene.bvhs), "triangles": len(scene.tris), "vertices": len(verts), "wave": args.wave,
         "rebuild_batch": args.batch, "warmup": args.warmup, "reps": args.reps, "repeat": args.repeat, "rebuild": [], "rays": args.rays}
    for leaf in leaves:
        row = {"max_leaf": leaf, "models": timed(scene, vdev, leaf, True)}
        for name, one in zip(("rubik", "knot"), alone):
            row[name + "_alone"] = timed(one, dev(R.wave_vertices(one.verts, args.wave)), leaf, False)
        row["sum_alone_ms"] = round(row["rubik_alone"]["rebuild_ms"] + row["knot_alone"]["rebuild_ms"], 5)
        r["rebuild"].append(row)

    # the host path: readback, a midpoint tree per record, destroy, create
    own = np.zeros(len(scene.tris), np.int64)
    own[len(alone[0].tris):] = 1
    lib = _lib.lib()

    def host_scene(pos):
        return S.Scene.from_models([S.model_from_triangles(pos[scene.tris["v"][own == k]].reshape(-1, 9)) for k in (0, 1)])

    def create(s):
        h = C.c_void_p()
        rc = lib.srt_query_create(0, None, S._ptr(s.bvhs), len(s.bvhs), S._ptr(s.nodes), len(s.nodes), S._ptr(s.tris), len(s.tris),
                                  S._ptr(s.verts), len(s.verts), C.byref(h))
        assert rc == _lib.SRT_OK, _lib.last_error()
        return h

    h, ms = create(scene), []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        built = host_scene(vdev.cpu().numpy()[:, :3])
        lib.srt_query_destroy(h)
        h = create(built)
        if k >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    lib.srt_query_destroy(h)
    r["host_rebuild_ms"] = round(statistics.median(ms), 4)
    r["host_rebuild_ms_min_max"] = [round(min(ms), 4), round(max(ms), 4)]

    rays = dev(surface_rays(S.refit_scene(scene, verts), args.rays))
    r["closest"] = {}
    with Query(scene, refit=True) as qr, Query(host_scene(verts["pos"])) as qm:
        qr.refit(vdev)
        for key, qq in (("refit", qr), ("midpoint", qm)):
            med, lo, hi, _ = closest_rate(torch, qq, rays, args.warmup, args.reps)
            r["closest"][key] = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "mrays_s": round(args.rays / med / 1e3, 1)}
    for leaf in leaves:
        with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=leaf) as ql:
            ql.rebuild(vdev)
            med, lo, hi, _ = closest_rate(torch, ql, rays, args.warmup, args.reps)
            r["closest"][f"models_leaf_{leaf}"] = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                                                   "mrays_s": round(args.rays / med / 1e3, 1)}
    print(json.dumps(r), flush=True)
    if args.out:
        doc = {"tool": "tools/bench_rebuild.py --models", "device": torch.cuda.get_device_name(0),
               "code_hash": lib.srt_code_hash().decode(),
               "timing": "rebuild: torch.cuda.Event pair around a batch of srt_query_rebuild calls on the object's stream, per call "
                         "(each call synchronises once); the median of --reps such batches, --repeat times over on fresh objects; "
                         "host rebuild: host wall clock of readback + a host midpoint build per record + srt_query_destroy + "
                         "srt_query_create; closest: event pair around one enqueued srt_query_closest",
               "result": r}
        pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wave", type=float, default=WAVE_AMPLITUDE)
    ap.add_argument("--degraded", type=float, default=0.8, help="refit / midpoint rate under which the doubling stops")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=20, help="srt_query_rebuild calls between two events")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", help="write the results to this JSON file")
    ap.add_argument("--leaf", type=lambda t: [int(x) for x in t.split(",")], metavar="L,L,...",
                    help="measure the leaf collapse at these max_leaf values (srt_rebuild_leaf.h) instead")
    ap.add_argument("--models", action="store_true",
                    help="measure the two-record scene Rubik + knot (srt_rebuild_models.h) instead; --leaf defaults to 1,4")
    ap.add_argument("--waves", type=lambda t: [float(x) for x in t.split(",")], default=[0.25, 1.0, 4.0], metavar="A,A,...",
                    help="with --leaf: the amplitudes the query rate is measured at")
    ap.add_argument("--repeat", type=int, default=3, help="with --leaf: rebuild timings per max_leaf, each on a fresh object")
    args = ap.parse_args()
    if args.leaf and (not all(1 <= x <= 255 for x in args.leaf) or args.repeat < 1):
        ap.error("--leaf takes values in [1, 255], --repeat at least 1")
    if args.warmup < 3 or args.reps < 10 or args.batch < 1:
        ap.error("at least 3 warm-up rounds and 10 measured ones")
    import torch  # noqa: F401  (before the library: one HIP runtime per process)

    (run_models if args.models else run_leaf if args.leaf else run)(args)


if __name__ == "__main__":
    main()
