#!/usr/bin/env python3
"""Choose the denoiser's default sigmas on the CPU: the oracle's Rubik frame at WIDTH x HEIGHT and --spp,
filtered by the numpy restatement of the filter (tests/denoise_ref.py) over a grid of (sigma_color, sigma_depth),
against the oracle's --ref-spp frame.  Prints the MSE over hit pixels per pair, the raw mean's MSE and the best
pair; no GPU and no library call is involved.  DESIGN.md section 5 ("Denoiser") quotes its output.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--sigma-color", type=float, nargs="+", default=[0.1, 0.3, 1.0, 3.0])
    ap.add_argument("--sigma-depth", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    a = ap.parse_args()

    import denoise_ref as D
    import srt_amd as S
    from conftest import OBJECTS, oracle_render
    from oracle import pyoracle as O
    from srt_amd import render as R

    setup = R.make_setup(a.width, a.height, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    cam = setup.camera
    o, d = D.camera_rays(cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector(), a.width, a.height)
    rays = np.zeros(a.width * a.height, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    tri, t, nrm, _ = O.Oracle(setup.scene).trace_closest(setup.bvh_count, rays)
    sh = (a.height, a.width)
    guide = D.make_guide(tri.reshape(sh), t.reshape(sh), nrm.reshape(sh + (3,)))
    hit = guide["tri"] != D.MISS
    acc, _, _ = oracle_render(setup, a.spp)
    ref_acc, _, _ = oracle_render(setup, a.ref_spp)
    noisy, ref = D.mean_colour(acc, a.spp + 1), D.mean_colour(ref_acc, a.ref_spp + 1)

    def mse(img):
        return float(np.mean((img[hit].astype(np.float64) - ref[hit].astype(np.float64)) ** 2))

    out = {"width": a.width, "height": a.height, "spp": a.spp, "ref_spp": a.ref_spp,
           "hit_fraction": round(float(hit.mean()), 4), "mse_raw_mean": mse(noisy), "grid": []}
    for sc in a.sigma_color:
        for sd in a.sigma_depth:
            m = mse(D.atrous(noisy, guide, 5, 5, sc, sd))
            out["grid"].append({"sigma_color": sc, "sigma_depth": sd, "mse": m})
            print(f"sigma_color {sc:<5} sigma_depth {sd:<5} mse {m:.6f}", flush=True)
    best = min(out["grid"], key=lambda r: r["mse"])
    out["best"] = best
    print(f"raw mean mse {out['mse_raw_mean']:.6f}; best {best}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
