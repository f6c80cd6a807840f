#!/usr/bin/env python
"""bench.py -- Mrays/s of the MI355X path tracer on BASELINE.json's metric workload.

BASELINE metric: "Mrays/s + frame ms at 1920x1080, 256 spp, Airplane OBJ; 1/2/4/8 GPU".
The Airplane OBJ is absent from the reference checkout (.MISSING_LARGE_BLOBS), so
the default workload is the same frame shape and sampling on the reference's
shipped model scene (Rubik.obj, model camera, the 6 lights of src/main.cpp:584-589).

A step = one full progressive render of the workload: the reset frame + `spp`
sampled frames (one fused kernel launch per GPU) and, for N > 1, the gather of
every rank's sRGB8 row bands (4 B/px) to GPU 0 (RCCL over xGMI) plus GPU 0's
de-interleave of the frame.  Inputs (scene, noise buffers, lights) are resident
in HBM before timing.

N > 1 runs two ways, with the same kernels and the same exchange:
  python bench.py --gpus N     the in-process device group (srt_group_*: one context per GPU
                               in this process, ncclCommInitAll + ncclGather), what a C++ host
                               embedding the library does; --same-device puts every context on
                               GPU 0 (device copies instead of RCCL: the one-GPU test);
  torchrun --nproc-per-node N bench.py --gpus N
                               one process per GPU, torch.distributed over RCCL.

A plain run does only what the headline needs: set-up, the counting launch, warmup, the timed steps,
then the line.  --dump-outputs DIR also writes what the last timed step computed (the radiance
accumulation and the sRGB8 frame, as rank 0 reads them) to DIR/accum.npy and DIR/out.npy in float32;
the inputs are fixed by the arguments, so two builds can be compared array for array.

--full adds the rest: the CPU baseline (N = 1) and three more legs that time the real-mesh path
(scenes too large for the LDS scene copy, traversed from HBM/L2), each under "legs" with its own
roofline and ray mix; `value` is the main leg:
  global_scene        a synthetic 1 M-triangle soup (SURVEY.md 8d generator), 1920x1080 @16 spp;
  surface_mesh        a closed 262k-triangle surface (torus-knot tube wound outward, as an
                      exported mesh is, so paths bounce off it), 1920x1080 @64 spp;
  airplane_materials  C3's regime: the knot carrying the Airplane's six textured materials,
                      sampled at each hit's uv, at C3's 1920x1080 @256 spp.  The absent Airplane
                      OBJ would run in this mode (no real mesh fits the LDS copy), so the line
                      repeats this leg at top level as `c3_regime`, beside the Rubik `value`.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
       torchrun --nproc-per-node N bench.py --gpus N ...
       (tests: under torchrun, --backend gloo --same-device runs N ranks on one GPU, staging through the host)
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "simple-ray-tracer_amd"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters and LDS / wave sections)
CLOCK_HZ = 2.4e9
HBM_PEAK_GBS = 8000.0
SIMDS = 256 * 4
CUS = 256
VALU_ISSUE_CYCLES = 2  # one wave64 VALU instruction per 2 cycles per SIMD-32
VALU_PEAK_GIPS = SIMDS * CLOCK_HZ / VALU_ISSUE_CYCLES / 1e9  # 1228.8 G wave-instructions/s
LDS_PEAK_GCPS = CUS * CLOCK_HZ / 1e9  # 614.4 G LDS-array cycles/s (one per CU per clock)


def valu_issue_calibrated_gips(waves: int):
    """The VALU issue rate a SIMD reaches with `waves` waves of independent f32 arithmetic (tools/valu_issue_probe.hip,
    profiles/r05_calib/valu_issue_calibration.json): the fastest of the FMA / MUL / ADD forms at the nearest measured
    occupancy at or above `waves` (4 or 8 waves per SIMD), in G wave-instructions/s over 1024 SIMDs at 2.4 GHz.
    Two VALU instructions may issue per quad-cycle only from different waves, and on gfx950 even independent
    FMA streams reach 0.36-0.42 per cycle, not the nominal 0.5; min/max, compares and selects ~0.22."""
    p = ROOT / "profiles" / "r05_calib" / "valu_issue_calibration.json"
    try:
        rows = json.loads(p.read_text())["rows"]
        occ = min((r["waves_per_simd"] for r in rows if r["waves_per_simd"] >= waves), default=None)
        if occ is None:
            return None
        rate = max(r["wave_instr_per_simd_per_cycle"] for r in rows if r["waves_per_simd"] == occ and
                   r["form"].split()[0] in ("v_fmac_f32_e32", "v_fma_f32", "v_mul_f32_e32", "v_mul_f32_e64",
                                            "v_sub_f32_e32"))
        return {"peak": round(rate * SIMDS * CLOCK_HZ / 1e9, 1), "waves_per_simd_measured": occ,
                "rate_per_simd_cycle": rate}
    except Exception:
        return None


def kernel_waves(kernel_name: str) -> int:
    """Waves per SIMD of the timed instance (timed_kernel()'s description; the LDS kernel runs 4)."""
    import re

    m = re.search(r"(\d+) waves per SIMD", kernel_name)
    return int(m.group(1)) if m else 4


def l2_miss_peak_gbs() -> float:
    """The memory-side roof for the traversal's reads, measured (tools/gather_calib.hip,
    profiles/r03_gather_calibration.json): every L2 miss is one 128-B line request (FETCH_SIZE tallies
    it at 64 B), and random whole-record reads of a table the Infinity Cache holds move at most ~7.2 TB/s
    of lines; past the Infinity Cache, random lines move at 1.8-5.8 TB/s and a stream at 5.9 TB/s.  The
    counters cannot tell Infinity-Cache hits from HBM reads, so this roof is 'l2_miss', not 'hbm'."""
    p = ROOT / "profiles" / "r03_gather_calibration.json"
    try:
        cases = json.loads(p.read_text())["cases"]
        return max(c["dram_32B_bytes"] / (c["ms"] * 1e-3) / 1e9 for c in cases
                   if c["case"] != "stream" and c["table_MiB"] < 256)
    except Exception:
        return HBM_PEAK_GBS


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (10 timed steps: the first timed launch has no predecessor to overlap its drain, which 3 steps of a
    # 26-ms leg would still show; the metric's 10 steps take 1.5 s)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", default="rubik",
                    choices=("rubik", "spheres", "synthetic", "torusknot", "airplane_knot", "first_hit_knot"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--synthetic-tris", type=int, default=10_000_000)
    ap.add_argument("--band-rows", type=int, default=2)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target length of the CPU-baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-global-leg", action="store_true", help="skip the 1 M-triangle global-scene leg")
    ap.add_argument("--global-tris", type=int, default=1_000_000)
    ap.add_argument("--global-spp", type=int, default=16)
    ap.add_argument("--no-surface-leg", action="store_true", help="skip the 262k-triangle surface-mesh leg")
    ap.add_argument("--surface-spp", type=int, default=64)
    ap.add_argument("--no-airplane-leg", action="store_true",
                    help="skip the surface mesh carrying the Airplane's textured materials (C3's regime)")
    ap.add_argument("--airplane-spp", type=int, default=256, help="the Airplane-material leg's spp (C3's 256)")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"))
    ap.add_argument("--same-device", action="store_true", help="every rank on cuda:0 (multi-rank tests on one GPU)")
    ap.add_argument("--group", action="store_true",
                    help="run the in-process device group even at --gpus 1 (one RCCL rank: the N > 1 path's code)")
    ap.add_argument("--dump", default=None, help="rank 0 saves the assembled frame (npz) after the last step")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes the last timed step's arrays to DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--full", action="store_true",
                    help="also run the CPU baseline and the real-mesh legs (each still subject to its --no-* option)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def algorithmic_bytes(st: dict) -> int:
    """Bytes one sample_kernel launch must move (SURVEY.md 8d per-unit prices): 32 B per node box test,
    40 B per triangle test, 48 B per mesh-material fetch, 4 B per uniform-noise fetch, 8 B per jitter
    fetch, 32 B per light record, and the 16-B radiance store per sample (the sample buffer that
    accumulate_kernel sums; it replaces the reference's per-frame 32-B accumulation RMW)."""
    return (32 * st["nodes"] + 40 * st["tris"] + 48 * st["mat_reads"] + 4 * st["rng_u"] + 8 * st["rng_sq"]
            + 32 * st["light_reads"] + 16 * st["samples"])


def cpu_baseline(setup, spp_first: int, target_s: float) -> dict:
    """The oracle (scalar C restatement, OpenMP over row pieces) on this host, on a bounded sample of the workload:
    every 8th row of the frame, full width, consecutive frames of the same progressive sequence."""
    from oracle import pyoracle as O

    s = setup
    threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or min(16, os.cpu_count() or 1)
    orc = O.Oracle(s.scene, s.lights, s.noise, s.noise_u)
    cam = s.camera
    f = O.Oracle.frame(s.width, s.height, show_model=s.show_model, bvh_count=s.bvh_count, light_count=len(s.lights),
                       max_depth=s.max_depth, origin=cam.position, direction=cam.front, up=cam.up, right=cam.right)
    acc = np.zeros((s.height, s.width, 4), np.float32)
    out = np.zeros((s.height, s.width, 4), np.uint8)
    rows = np.arange(0, s.height, 8, dtype=np.int32)
    # calibrate on one frame, then size the sample to ~target_s
    t0 = time.perf_counter()
    st = orc.render_rows(f, spp_first, 1, acc, out, rows, threads)
    t1 = time.perf_counter()
    frames = max(1, int(target_s / max(t1 - t0, 1e-3)) - 1)
    frames = min(frames, 255)
    t2 = time.perf_counter()
    st2 = orc.render_rows(f, spp_first + 1, frames, acc, out, rows, threads)
    t3 = time.perf_counter()
    rays = st["rays"] + st2["rays"]
    secs = (t1 - t0) + (t3 - t2)
    return {"value": rays / secs / 1e6, "unit": "Mrays/s", "cores": threads, "kind": "port",
            "sample": f"oracle (gcc -O2 -mfma -ffp-contract=off: hardware FMA, OpenMP over 64-pixel row pieces) on {len(rows)} rows "
                      f"(every 8th) x {s.width} px x {frames + 1} frames of the same workload ({rays} rays, "
                      f"{secs:.1f} s)"}


def load_counters(workload: str):
    """Per-launch PMC counters of the workload's sample_kernel from the committed rocprofv3 passes
    (profiles/counters.json, written by tools/pmc_roofline.py), or None."""
    p = ROOT / "profiles" / "counters.json"
    if not p.exists():
        return None
    try:
        return json.loads(p.read_text()).get(workload)
    except Exception:
        return None


def code_hash() -> str:
    """srt_code_hash() of the loaded library: its kernel sources + hipcc flags."""
    from srt_amd import _lib

    return _lib.lib().srt_code_hash().decode()


def roofline(workload: str, k_ms: float, alg_bytes: int, kernel_name: str, global_mode: bool = False,
             scale: float = 1.0) -> dict:
    """Roofs of the dominant kernel, fractions of the live kernel time (each launch's span on the GPU clock, srt_kernel_time):
    VALU issue (SQ_INSTS_VALU x 2 cycles per SIMD-32 over 1024 SIMDs), LDS-array cycles
    (SQ_LDS_IDX_ACTIVE over 256 CUs), HBM (corrected FETCH_SIZE + WRITE_SIZE over 8 TB/s).  The counters
    are per launch of this workload, from profiles/counters.json, and count only when they were collected
    on the code that is timed (their code_hash equals the loaded library's); `bound` is the highest
    fraction."""
    k_s = k_ms * 1e-3
    alg_gbs = alg_bytes / k_s / 1e9
    here = code_hash()
    r = {"kernel": kernel_name, "kernel_ms": round(k_ms, 3), "algorithmic_bytes_per_launch": int(alg_bytes),
         "algorithmic_GBps": round(alg_gbs, 1), "code_hash": here}
    cnt = load_counters(workload)
    if cnt is not None and cnt.get("code_hash") != here:
        r.update({"bound": None, "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None,
                  "counters_source": cnt.get("source", ""), "counters_code_hash": cnt.get("code_hash"),
                  "note": "the committed PMC counters of this workload were collected on other code (their "
                          "code_hash differs from the loaded library's): roofs not reported until re-captured"})
        return r
    if cnt is None:
        # no roof can be claimed without counters: algorithmic bytes are mostly LDS / L2 reads, and
        # dividing them by the HBM peak gives fractions above 1 (round-1 VERDICT)
        r.update({"bound": None, "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None,
                  "note": "no committed PMC counters for this workload (profiles/counters.json): roofs unmeasured; "
                          "algorithmic_GBps = SURVEY 8d bytes per launch / kernel time"})
        return r
    if scale != 1.0:  # a rank's share of the 1-GPU launch (its share of the counted rays)
        cnt = {k: (v * scale if isinstance(v, (int, float)) else v) for k, v in cnt.items()}
        r["counters_scaled_by_ray_share"] = round(scale, 5)
    valu_gips = cnt["SQ_INSTS_VALU"] / k_s / 1e9
    lds_gcps = cnt["SQ_LDS_IDX_ACTIVE"] / k_s / 1e9
    hbm_bytes = cnt["hbm_bytes"]
    hbm_gbs = hbm_bytes / k_s / 1e9
    roofs = {
        "valu_issue": (valu_gips, VALU_PEAK_GIPS, "G VALU wave-instructions/s"),
        "lds": (lds_gcps, LDS_PEAK_GCPS, "G LDS-array cycles/s"),
        "l2_miss": (hbm_gbs, l2_miss_peak_gbs(), "GB/s of L2-miss lines (Infinity Cache or HBM)"),
    }
    fr = {k: a / p for k, (a, p, _) in roofs.items()}
    bound = max(fr, key=fr.get)
    a, p, u = roofs[bound]
    r.update({
        "bound": bound, "achieved": round(a, 2), "peak": p, "unit": u, "frac": round(a / p, 4),
        "traffic": int(hbm_bytes),
        "traffic_over_hbm_spec": round(hbm_gbs / HBM_PEAK_GBS, 4),
        "fractions": {k: round(v, 4) for k, v in fr.items()},
        "valu_lane_utilisation": round(cnt["SQ_THREAD_CYCLES_VALU"] / (64.0 * cnt["SQ_INSTS_VALU"]), 4),
        "useful_valu_frac": round(fr["valu_issue"] * cnt["SQ_THREAD_CYCLES_VALU"] / (64.0 * cnt["SQ_INSTS_VALU"]), 4),
        "lds_bank_conflict_frac": round(cnt["SQ_LDS_BANK_CONFLICT"] / max(cnt["SQ_LDS_IDX_ACTIVE"], 1.0), 4),
        **issue_split(cnt, k_s),
        **valu_calibrated(valu_gips, kernel_name),
        "counters_source": cnt.get("source", ""),
        "counters_code_hash": cnt.get("code_hash"),
        "note": "frac = the bound roof's fraction at the live kernel time; per-launch counters from the committed "
                "rocprofv3 passes of this workload (profiles/counters.json). The 2.4 GHz peak clock makes every "
                "fraction a lower bound. " + (
                    "l2_miss = the L2 misses' 128-B lines (2 x FETCH_SIZE + WRITE_SIZE, calibrated: "
                    "profiles/r03_gather_calibration.json), served by the Infinity Cache or HBM, over the measured "
                    "line-rate roof; traffic = those bytes per launch; "
                    "algorithmic_GBps = SURVEY 8d bytes per launch / kernel time (L2 hits included)." if global_mode
                    else "algorithmic_GBps = SURVEY 8d bytes per launch / kernel time: the scene is read from LDS "
                         "and the noise from L2, so it is not an HBM rate."),
    })
    return r


def valu_calibrated(valu_gips: float, kernel_name: str) -> dict:
    """The VALU issue fraction against the measured issue rate of independent f32 arithmetic at the instance's
    occupancy (valu_issue_calibrated_gips), beside the nominal one (`fractions.valu_issue`)."""
    cal = valu_issue_calibrated_gips(kernel_waves(kernel_name))
    if not cal:
        return {}
    return {"valu_issue_calibrated": {"achieved": round(valu_gips, 2), "peak": cal["peak"],
                                      "unit": "G VALU wave-instructions/s", "frac": round(valu_gips / cal["peak"], 4),
                                      "waves_per_simd": kernel_waves(kernel_name),
                                      "basis": f"independent f32 FMA/MUL streams at {cal['waves_per_simd_measured']} "
                                               f"waves per SIMD: {cal['rate_per_simd_cycle']} wave-instructions per "
                                               "SIMD per cycle (profiles/r05_calib/valu_issue_calibration.json)"}}


def issue_split(cnt: dict, k_s: float) -> dict:
    """Where a wave's cycles go, from the second SQ pass (tools/profile_round.sh): issuing an instruction
    (SQ_ACTIVE_INST_ANY: one quad-cycle per instruction), waiting on memory / LDS (SQ_WAIT_ANY) or stalled on
    issue (SQ_WAIT_INST_ANY), as fractions of SQ_WAVE_CYCLES (they sum to ~1); instructions issued per SIMD
    per quad-cycle (each wave issues at most one); the share of VALU quad-cycles that issued two VALU
    instructions (SQ_ACTIVE_INST_VALU2, from two waves)."""
    if "SQ_ACTIVE_INST_ANY" not in cnt or "SQ_WAVE_CYCLES" not in cnt:
        return {}
    w = cnt["SQ_WAVE_CYCLES"]
    out = {"wave_cycles": {"issuing": round(cnt["SQ_ACTIVE_INST_ANY"] / w, 4),
                           "waiting": round(cnt["SQ_WAIT_ANY"] / w, 4),
                           "issue_stalled": round(cnt.get("SQ_WAIT_INST_ANY", float("nan")) / w, 4)},
           "instructions_per_simd_quad_cycle": round(cnt["SQ_ACTIVE_INST_ANY"] / (SIMDS * k_s * CLOCK_HZ / 4), 4)}
    if "SQ_ACTIVE_INST_VALU2" in cnt and "SQ_ACTIVE_INST_VALU" in cnt:
        v, v2 = cnt["SQ_ACTIVE_INST_VALU"], cnt["SQ_ACTIVE_INST_VALU2"]
        out["valu_dual_issue_share"] = round(v2 / max(v - v2, 1.0), 4)
    return out


def build_setup(scene: str, W: int, H: int, spp: int, max_depth: int, synthetic_tris: int):
    from srt_amd import render as R

    if scene == "rubik":
        models = [R.rubik_model(ROOT / "tests" / "golden" / "objects")]
        show_model, wl = True, f"rubik_{W}x{H}_{spp}spp"
    elif scene == "synthetic":
        models = [R.synthetic_model(synthetic_tris)]
        show_model, wl = True, f"synthetic{synthetic_tris}_{W}x{H}_{spp}spp"
    elif scene == "torusknot":  # outward faces, framed at render.SURFACE_KNOT_SCALE
        models = [R.torus_knot_model()]
        show_model, wl = True, f"torusknot262144out_{W}x{H}_{spp}spp"
    elif scene == "first_hit_knot":  # rounds 2-5's surface leg: inward faces, no path bounces
        models = [R.first_hit_only_knot_model()]
        show_model, wl = True, f"torusknot262144in_{W}x{H}_{spp}spp"
    elif scene == "airplane_knot":
        models = [airplane_knot_model()]
        show_model, wl = True, f"torusknot262144_airplane_materials_{W}x{H}_{spp}spp"
    else:
        models, show_model, wl = None, False, f"spheres_{W}x{H}_{spp}spp"
    if max_depth != 5:
        wl += f"_depth{max_depth}"
    return R.make_setup(W, H, show_model=show_model, models=models, max_depth=max_depth), wl


AIRPLANE_MATERIALS = ("11803_Airplane_body", "11803_Airplane_wing_R", "11803_Airplane_wing_details_R",
                      "11803_Airplane_tail", "11803_Airplane_wing_details_L", "11803_Airplane_wing_L")


def airplane_knot_model():
    """C3's material path on the surface mesh: the torus-knot tube (outward faces) carrying the Airplane's six
    .mtl materials and 1024x1024 diffuse PNGs (the reference's assets, tests/golden/objects), one segment each,
    with real per-vertex uvs loaded (has_texcoords set): every hit samples its texture at its uv
    (srt_amd.render.write_textured_torus_knot_obj; tests/test_gpu_configs.py renders it at 1080p @256 spp)."""
    import shutil
    import tempfile

    import srt_amd as S
    from srt_amd import render as R

    src = ROOT / "tests" / "golden" / "objects" / "11803_Airplane_v1_l1"
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        for f in src.iterdir():
            shutil.copy(f, d / f.name)
        obj = R.write_textured_torus_knot_obj(d / "knot_airplane.obj", "11803_Airplane_v1_l1.mtl", AIRPLANE_MATERIALS)
        return S.load_obj(obj, texcoords=True)


class RankRun:
    """One rank's share of a workload under torch.distributed (one process per GPU): its row bands
    (srt_set_tiling), its images in torch tensors, and bench's step (clear + one fused launch of `spp`
    frames that also encodes the rank's own sRGB8 rows, then on N > 1 the per-frame exchange: one gather
    of every rank's sRGB8 rows, 4 B/px, into rank 0's preallocated receive buffer, and rank 0's
    de-interleave).  The radiance stays on its rank; frame() gathers it for a dump."""

    def __init__(self, setup, spp, *, rank, world, device, band_rows, stream):
        import torch

        from srt_amd import parallel as PAR
        from srt_amd import render as R

        self.setup, self.spp, self.rank, self.world, self.band = setup, spp, rank, world, band_rows
        self.dev = torch.device("cuda", device)
        self.rdr = R.Renderer(setup, device=device, stream=stream.cuda_stream, rank=rank, nranks=world,
                              band_rows=band_rows)
        self.c = self.rdr.compute
        W, H = setup.width, setup.height
        self.rows_pad = PAR.rows_pad(H, band_rows, world)
        self.accum_local = torch.zeros((self.rows_pad, W, 4), dtype=torch.float32, device=self.dev)
        self.out_local = torch.zeros((self.rows_pad, W), dtype=torch.int32, device=self.dev)
        self.c.set_image_buffers(self.accum_local.data_ptr(), self.out_local.data_ptr())
        self.recv_out = self.full_out = None
        self.ex_events = []
        if rank == 0 and world > 1:
            self.recv_out = torch.empty((world, self.rows_pad, W), dtype=torch.int32, device=self.dev)
            self.full_out = torch.zeros((H, W), dtype=torch.int32, device=self.dev)

    def count(self) -> dict:
        """Deterministic counting run (untimed): the work every step repeats."""
        import torch

        self.rdr.render(self.spp, count=True, write_output=True)
        torch.cuda.synchronize(self.dev)
        return self.c.stats()

    def step(self):
        import torch

        from srt_amd import parallel as PAR

        self.rdr.clear()
        self.c.render_frames(2, self.spp, write_output=True, count=False)
        self.rdr.accum_frames = self.spp + 1
        if self.world > 1:  # the one exchange: every rank's sRGB8 rows to rank 0 (RCCL over xGMI)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()  # (the shared stream: after this rank's accumulation, i.e. its rows rendered)
            PAR.gather_bands(self.out_local, dst=0, out=self.recv_out)
            if self.rank == 0:
                self.c.assemble_output_bands(self.recv_out.data_ptr(), self.world, self.rows_pad, self.band,
                                             self.full_out.data_ptr())
            ev[1].record()
            self.ex_events.append(ev)

    def exchange_time(self) -> list:
        """[(ms, frames)] of this rank's part of the per-frame exchange since the last call (events on the
        shared stream around the gather and, on rank 0, the assembly)."""
        import torch

        torch.cuda.synchronize(self.dev)
        ms = sum(a.elapsed_time(b) for a, b in self.ex_events)
        n = len(self.ex_events)
        self.ex_events = []
        return [(ms, n)]

    def chunks(self) -> list:
        return [self.c.GetInt("launch.chunks")]  # sample launches of the last render

    def overlaps(self) -> list:
        return [self.c.GetInt("launch.overlap")]  # the last render's launches overlapped their predecessors

    def sync(self):
        import torch

        torch.cuda.synchronize(self.dev)

    def kernel_time(self) -> list:
        return [self.c.kernel_time()]  # [(throughput ms, launches)] since the previous call

    def frame(self):
        """Rank 0's frame after a step: (accum (H, W, 4) float32, sRGB8 (H, W, 4) uint8) on the host; None
        on other ranks.  Collective for N > 1 (every rank calls it): the radiance rows are gathered here."""
        import torch

        from srt_amd import parallel as PAR

        torch.cuda.synchronize(self.dev)
        H, W = self.setup.height, self.setup.width
        if self.world > 1:
            stacked = PAR.gather_bands(self.accum_local, dst=0)
            if self.rank != 0:
                return None
            acc = torch.empty((H, W, 4), dtype=torch.float32, device=self.dev)
            self.c.assemble_bands(stacked.data_ptr(), self.world, self.rows_pad, self.band, self.spp + 1,
                                  acc.data_ptr(), None)
            out = self.full_out
        else:
            acc, out = self.accum_local, self.out_local
        torch.cuda.synchronize(self.dev)
        return (acc[:H].cpu().numpy(), out[:H].cpu().numpy().view(np.uint8).reshape(H, W, 4))

    def close(self):
        self.rdr.close()


class GroupRun:
    """The whole workload tiled over N devices of this one process through the C ABI's device group
    (srt_group_*, the C++ host's multi-GPU path): one context and stream per device, each rendering its
    row bands and encoding its own sRGB8 rows; per frame one gather of those rows (ncclGather over xGMI,
    communicators from ncclCommInitAll; device copies when a device repeats, as under --same-device) to
    device 0, which de-interleaves them.  No torch.distributed and no rank processes: this is what
    `python bench.py --gpus N` runs when it is not launched under torch.distributed.run."""

    def __init__(self, setup, spp, *, devices, band_rows):
        from srt_amd import render as R

        self.setup, self.spp = setup, spp
        self.devices = list(devices)
        self.grp = R.GroupRenderer(setup, self.devices, band_rows=band_rows)
        self.enqueue_s = []
        if self.grp.transport == "rccl" and self.grp.get_int("ranks") != len(self.devices):  # (the library checks too)
            raise SystemExit(f"RCCL sees {self.grp.get_int('ranks')} ranks, not {len(self.devices)}")

    def count(self) -> dict:
        return self.grp.count(self.spp)

    def step(self):
        t0 = time.perf_counter()
        self.grp.render(self.spp)
        self.enqueue_s.append(time.perf_counter() - t0)  # host time to enqueue every device's step

    def sync(self):
        self.grp.finish()

    def kernel_time(self) -> list:
        return self.grp.kernel_time()  # per context: (throughput ms, launches) since the previous call

    def exchange_time(self) -> list:
        return self.grp.exchange_time()  # per context: (ms of its part of the exchange, frames)

    def chunks(self) -> list:
        return [p.compute.GetInt("launch.chunks") for p in self.grp.parts]

    def overlaps(self) -> list:
        return [p.compute.GetInt("launch.overlap") for p in self.grp.parts]

    def rank_stats(self) -> list:
        return self.grp.part_stats

    def frame(self):
        return self.grp.accum(), self.grp.output()

    def info(self) -> dict:
        g = self.grp
        return {"mode": "in-process device group (srt_group_*)", "transport": g.transport,
                "rccl_ranks": g.get_int("ranks"), "contexts": g.get_int("contexts"), "devices": self.devices,
                "gather_bytes_per_frame": g.get_int("bytes.output") * 1024,
                "radiance_gathers_in_timed_steps": g.get_int("gathers.accum"),
                "host_enqueue_ms_per_step": round(1e3 * float(np.median(self.enqueue_s)), 3) if self.enqueue_s else None}

    def close(self):
        self.grp.close()


def run_leg(setup, spp, args, *, mode, rank, world, device, stream):
    """Counting run, warmup, then exactly `steps` timed steps enqueued back to back and bracketed by
    barrier + synchronize; every context's kernel time (its launches' throughput time, srt_kernel_time)
    and part of the per-frame exchange are read once, after the region.  Returns (elapsed max over ranks,
    total rays over ranks, this process's stats, per-context timing dicts, run)."""
    import torch
    import torch.distributed as dist

    if mode == "group":
        run = GroupRun(setup, spp, devices=[0] * args.gpus if args.same_device else range(args.gpus),
                       band_rows=args.band_rows)
    else:
        run = RankRun(setup, spp, rank=rank, world=world, device=device, band_rows=args.band_rows, stream=stream)
    st = run.count()
    counts = torch.tensor([float(st["rays"])], dtype=torch.float64)
    if mode == "dist" and world > 1:
        counts = counts.to(run.dev) if args.backend == "nccl" else counts
        dist.all_reduce(counts)
    total_rays = float(counts[0].item())
    for _ in range(args.warmup):
        run.step()
    run.sync()
    if mode == "dist" and world > 1:
        dist.barrier()
    run.sync()
    run.kernel_time()    # drops the counting and warmup launches
    run.exchange_time()  # (and the warmup's exchanges)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run.step()
    run.sync()
    if mode == "dist" and world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    kt, ex, chunks, ovl = run.kernel_time(), run.exchange_time(), run.chunks(), run.overlaps()
    per_ctx = []
    for i, ((ms, launches), (ex_ms, ex_n), ch, ov) in enumerate(zip(kt, ex, chunks, ovl)):
        # every timed launch is counted (a chunked render makes several per step), or the total is short
        if launches != args.steps * ch:
            raise SystemExit(f"context {i}: {launches} sample launches timed, expected {args.steps} steps x {ch}")
        per_ctx.append({"kernel_ms": ms / args.steps, "launches_per_step": ch, "overlap": bool(ov),
                        "exchange_ms": (ex_ms / ex_n) if ex_n else None})
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64)
    if mode == "dist" and world > 1:
        elapsed = elapsed.to(run.dev) if args.backend == "nccl" else elapsed
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    return float(elapsed.item()), total_rays, st, per_ctx, run


def rank_table(per_ctx, stats, args, mode, world, dev) -> list:
    """Every rank's (context's) timing and counted share, rank order: under torch.distributed one
    all_gather_object; the in-process group holds every context's already."""
    import torch.distributed as dist

    mine = [dict(t, rays=int(s["rays"]), algorithmic_bytes=int(algorithmic_bytes(s))) for t, s in zip(per_ctx, stats)]
    if mode != "dist" or world == 1:
        return mine
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    return [r for p in parts for r in p]


def per_rank_lines(table, workload, kname, global_mode) -> list:
    """Per rank: its render (sample-kernel throughput ms per step), its part of the per-frame exchange,
    and its roofline from the 1-GPU counters of the workload scaled by the rank's share of the counted
    rays (a rank's launch does that share of the 1-GPU launch's work: its row bands of every frame)."""
    total = sum(r["rays"] for r in table) or 1
    out = []
    for i, r in enumerate(table):
        share = r["rays"] / total
        rf = roofline(workload, r["kernel_ms"], r["algorithmic_bytes"], kname, global_mode=global_mode, scale=share)
        out.append({"rank": i, "kernel_ms": round(r["kernel_ms"], 3), "launches_per_step": r["launches_per_step"],
                    "exchange_ms": None if r["exchange_ms"] is None else round(r["exchange_ms"], 3),
                    "rays_share": round(share, 5), "roofline": rf})
    return out


KERNEL_LDS = "srt::sample_kernel<false, true, true, 1024, false, false, 4> (LDS-resident scene)"


def timed_kernel(c, scene: str) -> str:
    """The sample_kernel instance the run's timed launches took.  Global-scene mode: fused sub-steps for
    trees under 600 MB (the legs), the IL pattern past it (C5); the fused instance at 5 waves per SIMD
    for trees under 48 MB (the surface-mesh legs), else 4 (srt_get_int's scene.* names); the texture
    instance when materials sample their textures (the Airplane-material leg)."""
    if scene == "rubik":
        return KERNEL_LDS
    if scene == "spheres":
        return "srt::sphere_kernel<false> (spheres: no BVH, 5 waves per SIMD)"
    fused = c.GetInt("scene.fused") == 1
    gw = c.GetInt("scene.global_waves") if fused else 4
    tex = scene == "airplane_knot"
    return (f"srt::sample_kernel<false, false, true, 256, {'true' if tex else 'false'}, {'true' if fused else 'false'}, "
            f"{gw}> (global-scene mode, {'fused' if fused else 'IL'} sub-steps, {gw} waves per SIMD"
            f"{', textures sampled per hit' if tex else ''})")


def ray_kinds(st: dict) -> dict:
    """The counted rays by kind (srt_ray_kinds): camera (one per sample), shadow, bounce, and the bounce share."""
    cam, sh = int(st["samples"]), int(st.get("shadow_rays", 0))
    b = int(st["rays"]) - cam - sh
    return {"camera": cam, "shadow": sh, "bounce": b, "bounce_share": round(b / max(int(st["rays"]), 1), 4)}


DUMP_BUDGET_BYTES = 60_000_000  # the dump may take 64 MB in all; the rest is room for the file headers


def dump_outputs(dirname, arrays: dict) -> None:
    """The arrays as DIR/<name>.npy in float32.  When they exceed the budget together, every array above its equal
    share is cut to a fixed, seeded sample of its pixels (rows of the last axis), in raster order: the same
    pixels in every run and every build, so the files of two runs compare element for element."""
    d = pathlib.Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    arrays = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in arrays.items()}
    over = sum(a.nbytes for a in arrays.values()) > DUMP_BUDGET_BYTES
    share = DUMP_BUDGET_BYTES // len(arrays)
    for name, a in arrays.items():
        if over and a.nbytes > share:
            px = a.reshape(-1, a.shape[-1])
            keep = share // (4 * px.shape[1])
            a = px[np.sort(np.random.default_rng(0).choice(px.shape[0], keep, replace=False))]
        np.save(d / f"{name}.npy", a)


def run_compute(run):
    return run.grp.parts[0].compute if isinstance(run, GroupRun) else run.c


def parallelism(args, mode, world, run) -> str:
    if world == 1 and mode != "group":
        return "single GPU"
    if mode == "group":
        return (f"row-band tiling x{world} ({args.band_rows}-row bands) over the devices of one process + per-frame "
                f"sRGB8 gather to device 0 ({'RCCL ncclGather' if run.grp.transport == 'rccl' else 'device copies'})")
    return (f"row-band tiling x{world} ({args.band_rows}-row bands), one process per GPU + per-frame sRGB8 gather "
            f"to rank 0 ({'RCCL' if args.backend == 'nccl' else 'gloo'})")


def main(argv=None):
    args = parse(argv)
    # (the box's default of 4 hardware queues per process, which the two pipeline slots are sized for: torch's
    # stream, the context's and the two slots' each get one; profiles/r05_experiments/pipeline_slots_queues.txt)
    import torch
    import torch.distributed as dist

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world_env > 1:
        if world_env != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} differs from WORLD_SIZE {world_env}")
        mode, world = "dist", world_env  # torch.distributed.run: one rank per GPU
    elif args.gpus > 1 or args.group:
        mode, world = "group", args.gpus  # plain `python bench.py --gpus N`: the in-process device group
        if not args.same_device and torch.cuda.device_count() < args.gpus:
            raise SystemExit(f"--gpus {args.gpus}: only {torch.cuda.device_count()} devices visible")
    else:
        mode, world = "single", 1
    device = 0 if args.same_device else local_rank
    torch.cuda.set_device(device)
    if mode == "dist":
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")
    dev = torch.device("cuda", device)

    W, H, spp = args.width, args.height, args.spp
    setup, wl_name = build_setup(args.scene, W, H, spp, args.max_depth, args.synthetic_tris)
    stream = torch.cuda.Stream(device=dev)   # a real (non-null) stream shared by torch and the library
    torch.cuda.set_stream(stream)

    elapsed_s, total_rays, st, per_ctx, run = run_leg(setup, spp, args, mode=mode, rank=rank, world=world,
                                                      device=device, stream=stream)
    group_info = run.info() if mode == "group" else None  # (before a dump's radiance gather)
    if args.dump:
        fr = run.frame()
        if rank == 0:
            np.savez(args.dump, accum=fr[0], out=fr[1])
    if args.dump_outputs:
        fr = run.frame()  # (collective for N > 1: every rank calls it)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"accum": fr[0], "out": fr[1]})
    kname = timed_kernel(run_compute(run), args.scene)
    par = parallelism(args, mode, world, run)
    table = rank_table(per_ctx, run.rank_stats() if mode == "group" else [st], args, mode, world, dev)
    run.close()
    global_main = args.scene in ("synthetic", "torusknot", "airplane_knot", "first_hit_knot")

    legs = []
    for leg, enabled, scene, lw, lh, lspp, ntri in (
            ("global_scene", not args.no_global_leg, "synthetic", 1920, 1080, args.global_spp, args.global_tris),
            ("surface_mesh", not args.no_surface_leg, "torusknot", 1920, 1080, args.surface_spp, 0),
            ("airplane_materials", not args.no_airplane_leg, "airplane_knot", 1920, 1080, args.airplane_spp, 0)):
        if not (args.full and enabled):
            continue
        lsetup, lname = build_setup(scene, lw, lh, lspp, 5, ntri)
        l_el, l_rays, l_st, l_ctx, l_run = run_leg(lsetup, lspp, args, mode=mode, rank=rank, world=world,
                                                   device=device, stream=stream)
        l_kname = timed_kernel(run_compute(l_run), scene)
        l_table = rank_table(l_ctx, l_run.rank_stats() if mode == "group" else [l_st], args, mode, world, dev)
        l_run.close()
        if rank == 0:
            desc = (f"synthetic {ntri} triangles (SURVEY 8d generator)" if scene == "synthetic" else
                    "torus-knot tube, 262144 triangles wound outward so paths bounce (closed surface mesh; "
                    "srt_amd.render.torus_knot_triangles at SURFACE_KNOT_SCALE), model camera and lights"
                    if scene == "torusknot" else
                    "the torus-knot tube with outward faces carrying the Airplane's six .mtl materials and diffuse "
                    "PNGs, textures sampled at each hit's uv (C3's material path; bench.airplane_knot_model)")
            l_ranks = per_rank_lines(l_table, lname, l_kname, True)
            legs.append({
                "leg": leg, "workload": lname, "value": round(l_rays * args.steps / l_el / 1e6, 3),
                "unit": "Mrays/s", "ms_per_step": round(l_el * 1e3 / args.steps, 3),
                "config": {"scene": desc, "width": lw, "height": lh, "spp": lspp, "max_depth": 5},
                "rays_per_step": int(l_rays), "ray_kinds": ray_kinds(l_st),
                "kernel_ms_per_rank": [r["kernel_ms"] for r in l_ranks],
                "exchange_ms_per_rank": [r["exchange_ms"] for r in l_ranks],
                "roofline": max(l_ranks, key=lambda r: r["kernel_ms"])["roofline"],
                "per_rank": l_ranks if world > 1 else None,
            })

    if rank == 0:
        ms_per_step = elapsed_s * 1e3 / args.steps
        value = total_rays * args.steps / elapsed_s / 1e6
        ranks = per_rank_lines(table, wl_name, kname, global_main)
        slowest = max(ranks, key=lambda r: r["kernel_ms"])
        line = {
            "metric": "Mrays/s (CheckHit queries: camera + bounce + shadow rays) at the BASELINE frame/spp",
            "value": round(value, 3),
            "unit": "Mrays/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic inputs: glibc-rand noise buffers as the reference generates them; "
                    + ("Rubik.obj (the reference's shipped model scene; the Airplane OBJ is absent from its checkout)"
                       if args.scene == "rubik" else f"{args.scene} scene"),
            "config": {
                "workload": wl_name, "width": W, "height": H, "spp": spp, "max_depth": args.max_depth,
                "scene": args.scene, "lights": int(len(setup.lights)), "parallelism": par,
            },
            "frame_ms": round(ms_per_step / spp, 4),
            "msamples_per_s": round(W * H * spp * args.steps / elapsed_s / 1e6, 3),
            "rays_per_step": int(total_rays),
            "ray_kinds": ray_kinds(st),
            "code_hash": code_hash(),
            # sample-kernel throughput time per step of every rank (launches overlap their predecessor's
            # drain: each counts from its start or the previous launch's end to its end, srt_kernel_time),
            # and each rank's part of the per-frame sRGB8 exchange (N > 1)
            "kernel_ms_per_rank": [r["kernel_ms"] for r in ranks],
            "exchange_ms_per_rank": [r["exchange_ms"] for r in ranks],
            "launch_overlap": all(r["overlap"] for r in table),
            # the step's bound: the slowest rank's launch, its counters the 1-GPU launch's scaled by its share
            "roofline": slowest["roofline"],
            "per_rank": ranks if world > 1 else None,
            "legs": legs,
        }
        # C3's regime (BASELINE metric: the Airplane OBJ at 1920x1080 @256 spp): the absent mesh would run in
        # global-scene mode, measured here on the surface carrying the Airplane's textured materials at C3's spp
        c3 = next((l for l in legs if l["leg"] == "airplane_materials"), None)
        line["c3_regime"] = None if c3 is None else {
            "workload": c3["workload"], "value": c3["value"], "unit": "Mrays/s", "ms_per_step": c3["ms_per_step"],
            "spp": c3["config"]["spp"], "ray_kinds": c3["ray_kinds"], "roofline": c3["roofline"],
            "note": "the Airplane OBJ is absent (.MISSING_LARGE_BLOBS); any real mesh exceeds the LDS scene copy "
                    "and runs this global-scene instance, so this is C3's regime; `value` stays the Rubik stand-in"}
        if group_info is not None:
            line["group"] = group_info
        elif mode == "dist":
            line["group"] = {"mode": "torch.distributed, one process per GPU", "backend": args.backend,
                             "world_size": world,
                             "gather_bytes_per_frame": world * PAR_rows_pad(H, args.band_rows, world) * W * 4}
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(setup, 2, args.cpu_seconds)
        else:
            line["cpu_baseline"] = None
        print(json.dumps(line), flush=True)
    if mode == "dist":
        dist.destroy_process_group()


def PAR_rows_pad(height, band_rows, world):
    from srt_amd import parallel as PAR

    return PAR.rows_pad(height, band_rows, world)


if __name__ == "__main__":
    main()
