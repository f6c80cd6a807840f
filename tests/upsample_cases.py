"""Shared synthetic inputs of the guided-upsampling tests (tests/test_upsample_ref.py on the CPU,
tests/test_gpu_upsample.py on the GPU), numpy only, in the style of test_gpu_denoise.py::synthetic.

A low accumulation image (a sum over `frames`) and two hand-built guides, the full one drawn independently of the low
one: misses in blocks and scattered, two BVH ids, unit normals with runs of one shared normal and of its opposite
between random ones, t from {3, 3.02, 3.3, 250}.  From 10 x 10 low pixels on, two placed blocks make the rarer paths
certain: low pixels [0, 6) x [0, 6) are all hits while the full pixels over low [1, 4) x [1, 4) are all misses (no tap
of the bilinear four or of the ring has their id: the nearest path), and a low block of misses lies under a full block
of misses (a miss pixel averaging miss taps).
"""
from __future__ import annotations

import functools

import numpy as np

import denoise_ref as D

# (low_w, low_h, factor): 1x1 (every tap but one outside the image), 3x1, partial tiles in both axes (38 x 24),
# several tiles with the inexact thirds (69 x 42), factor 4 (72 x 44), and factor 1 (the second tap's weight is 0)
CASES = [(1, 1, 2), (3, 1, 4), (19, 12, 2), (23, 14, 3), (18, 11, 4), (5, 4, 1)]
BIG = [c for c in CASES if c[0] >= 10 and c[1] >= 10]
T_VALUES = np.asarray([3.0, 3.0, 3.0, 3.02, 3.3, 250.0], np.float32)


FACTOR, LOW_SPP, FULL_SPP = 2, 4, 1


@functools.lru_cache(maxsize=None)
def scene_case(name):
    """name: "rubik" or "textured" (tests/surface_scenes.py), oracle and numpy only, computed once per process.  The
    64 x 48 case of surface_scenes.case(name) (its guide, its 256-spp reference) beside the same camera's 32 x 24
    frame: {"full": that case, "low_setup", "low_hits", "low_guide", "low_acc" (the oracle's accumulation of reset +
    LOW_SPP frames at 32 x 24), "low_frames", "full_acc" / "full_frames" (reset + FULL_SPP frames at 64 x 48)}."""
    import surface_scenes as SS
    from conftest import oracle_render

    full = SS.case(name)
    w, h = SS.W // FACTOR, SS.H // FACTOR
    low_setup = SS.textured_setup(w, h) if name == "textured" else SS.rubik_setup(w, h)
    cl, cf = low_setup.camera, full["setup"].camera
    for a, b in ((cl.getOrigin(), cf.getOrigin()), (cl.getForward(), cf.getForward()),
                 (cl.getRightVector(), cf.getRightVector()), (cl.getUpVector(), cf.getUpVector())):
        assert (np.asarray(a, np.float32) == np.asarray(b, np.float32)).all()  # one camera, two sizes
    low_hits = SS.oracle_hits(low_setup.scene, low_setup.bvh_count, SS.pixel_rays(low_setup))
    low_acc, _, _ = oracle_render(low_setup, LOW_SPP)
    full_acc, _, _ = oracle_render(full["setup"], FULL_SPP)
    return {"full": full, "low_setup": low_setup, "low_hits": low_hits, "low_guide": D.guide_from_hits(low_hits, w, h),
            "low_acc": low_acc, "low_frames": LOW_SPP + 1, "full_acc": full_acc, "full_frames": FULL_SPP + 1}


def _guide(rng, w, h, n0):
    tri = rng.integers(0, 500, (h, w)).astype(np.uint32)
    tri[rng.uniform(size=(h, w)) < 0.15] = D.MISS
    n = rng.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    n[(np.arange(h) % 3) != 0] = n0            # two rows in three share one normal
    n[:, (np.arange(w) % 7) == 3] = -n0        # columns of the opposed normal
    t = rng.choice(T_VALUES, (h, w))
    bvh = (rng.uniform(size=(h, w)) < 0.25).astype(np.uint32)
    bvh[:, w // 2:] |= (rng.uniform(size=(h, w - w // 2)) < 0.5).astype(np.uint32)
    return tri, t, n, bvh


def hit_records(tri, t, n, bvh, rng):
    from srt_amd.query import HIT_DTYPE

    hits = np.zeros(tri.size, HIT_DTYPE)
    hits["triangle"], hits["t"], hits["normal"], hits["bvh"] = tri.reshape(-1), t.reshape(-1), n.reshape(-1, 3), bvh.reshape(-1)
    hits["material"] = rng.integers(0, 9, tri.size)  # never read by the stage
    return hits


def synthetic(w, h, f, seed=11, nonfinite=False, frames=3):
    """{"accum" (h, w, 4), "frames", "low" / "full": guides (denoise_ref.make_guide), "low_parts" / "full_parts":
    (tri, t, n, bvh) for hit_records, "rng"}."""
    rng = np.random.default_rng(seed + 1000 * w + 10 * h + f)
    W, H = f * w, f * h
    accum = np.ones((h, w, 4), np.float32)
    accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
    n0 = rng.normal(size=3)
    n0 = (n0 / np.linalg.norm(n0)).astype(np.float32)
    low = list(_guide(rng, w, h, n0))
    full = list(_guide(rng, W, H, n0))
    if w == 1 and h == 1:
        low[0][0, 0], low[3][0, 0] = 7, 1
        full[0][0, 0], full[3][0, 0] = 9, 1     # one full pixel of the low pixel's id; the others as drawn
        full[2][0, 0] = low[2][0, 0]
    if w >= 10 and h >= 10:
        blk = low[0][:6, :6]
        blk[blk == D.MISS] = 17                 # all hits ...
        full[0][f:4 * f, f:4 * f] = D.MISS      # ... under full misses: the nearest path
        low[0][h // 2:h // 2 + 3, w // 3:w // 3 + 4] = D.MISS
        full[0][f * (h // 2):f * (h // 2 + 2), f * (w // 3):f * (w // 3 + 3)] = D.MISS
    if nonfinite:
        assert w >= 10 and h >= 10
        accum[2, 2, :3] = (np.nan, 1.0, 2.0)    # the nearest pixel of the full pixels over it
        accum[3, 1, 1] = np.inf
        accum[7, 8, 0] = np.nan
        accum[h - 1, w - 1, 2] = -np.inf
        accum[h // 2 + 1, w // 3 + 1, :3] = np.inf   # inside the block of misses
        accum[8, 3, :3] = np.nan
    return {"accum": accum, "frames": frames, "low": D.make_guide(*low), "full": D.make_guide(*full),
            "low_parts": low, "full_parts": full, "rng": rng}
