#!/usr/bin/env python3
"""Choose the variance-guided filter's default sigma_lum on the CPU and record the quality comparison DESIGN.md
section 5 ("Variance-guided filter") quotes: Rubik 64 x 48, the 8-frame orbit and the 8-frame spin, every frame the
oracle's reset + 1 spp, through the numpy restatements (tests/variance_ref.py, tests/denoise_ref.py) against the
oracle's 256-spp frame of the last camera or pose.  Over the hit pixels it prints, for the raw 1-spp mean, the
temporal output, temporal + the existing filter at its defaults and temporal + the variance-guided filter per
sigma_lum: the MSE of linear radiance and the MSE after x / (1 + x) per channel.  No GPU and no library call that
touches a device is involved.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (str(ROOT / "simple-ray-tracer_amd"), str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sigma-lum", type=float, nargs="+", default=[0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    ap.add_argument("--min-history", type=int, nargs="+", default=[4])
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 2, 3, 5],
                    help="at 64 x 48 the fifth pass's step of 16 pixels spans a third of the image")
    a = ap.parse_args()

    import variance_ref as V
    import variance_scenes as VS

    out = {"width": VS.RUBIK_W, "height": VS.RUBIK_H, "frames": VS.FRAMES, "ref_spp": VS.REF_SPP, "sequences": {}}
    total = {}
    for name, seq in (("orbit", VS.orbit()), ("spin", VS.spin())):
        res, mom = VS.temporal_pass(seq)[-1]
        base = VS.metrics(seq, {k: v for k, v in VS.four_images(seq, res, mom, seq["accs"][-1]).items() if k != "variance"})
        rec = {"hit_pixels": int((seq["guides"][-1]["tri"] != V.MISS).sum()), "young": float((mom[..., 3] < 4).mean()),
               **{k: {"mse": m, "mse_tm": t} for k, (m, t) in base.items()}, "grid": []}
        for k, (m, t) in base.items():
            print(f"{name:5} {k:9} mse {m:.6f}  tone-mapped {t:.6f}", flush=True)
        for mh in a.min_history:
            for ps in a.passes:
                for sl in a.sigma_lum:
                    img = V.run_variance(res, 1, seq["guides"][-1], mom, sigma_lum=sl, min_history=mh, passes=ps)[0]
                    m, t = VS.metrics(seq, {"v": img})["v"]
                    rec["grid"].append({"sigma_lum": sl, "min_history": mh, "passes": ps, "mse": m, "mse_tm": t})
                    total[(sl, mh, ps)] = total.get((sl, mh, ps), 0.0) + t
                    print(f"{name:5} variance  passes {ps} sigma_lum {sl:<6} min_history {mh:<3} mse {m:.6f}  tone-mapped {t:.6f}",
                          flush=True)
        out["sequences"][name] = rec
    best = min(total, key=total.get)
    out["best"] = {"sigma_lum": best[0], "min_history": best[1], "passes": best[2], "sum_mse_tm": total[best]}
    for ps in a.passes:
        row = {k[0]: v for k, v in total.items() if k[1] == best[1] and k[2] == ps}
        print(f"passes {ps}: summed tone-mapped MSE per sigma_lum " + "  ".join(f"{k:g}: {v:.6f}" for k, v in sorted(row.items())))
    print(f"lowest tone-mapped MSE summed over both sequences: {out['best']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
