"""Shared inputs of the variance tests and of tools/variance_sigma_grid.py, CPU only (the oracle and the numpy
restatements; no library call that touches a device): Rubik at 64 x 48 along the 8-frame orbit of
tests/test_gpu_temporal.py and under the 8-frame spin of tests/test_gpu_temporal_motion.py, each frame the oracle's
reset + 1 spp, with the oracle's 256-spp frame of the last camera or pose; and the four images of the quality
comparison.  Everything is computed once per process and left unchanged.
"""
from __future__ import annotations

import copy
import functools

import numpy as np

import denoise_ref as D
import temporal_motion_ref as M
import temporal_ref as T
import variance_ref as V

RUBIK_W, RUBIK_H = 64, 48
ORBIT_PATH = [(0.5, -1.0)] * 7   # MoveRight(delta), Rotate(yaw, 0) after the first frame
SPIN_DEGREES, FRAMES = 2.0, 8
REF_SPP = 256
EXISTING = dict(passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2)  # srt_denoise.h's defaults


def rubik_setup(w=RUBIK_W, h=RUBIK_H):
    import srt_amd as S
    from conftest import OBJECTS
    from srt_amd import render as R

    return R.make_setup(w, h, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])


def orbit_cameras(setup):
    """Moves setup.camera along ORBIT_PATH, yielding after each position (8 in all)."""
    yield setup.camera
    for delta, yaw in ORBIT_PATH:
        setup.camera.MoveRight(delta)
        setup.camera.Rotate(yaw, 0.0)
        yield setup.camera


def spin_poses(scene):
    """Per frame k the pose of record 0 with the cube turned by (k + 1) * SPIN_DEGREES about the vertical axis
    through the centre of its bounds."""
    v = scene.verts["pos"].astype(np.float64)
    centre = (v.min(0) + v.max(0)) / 2
    poses = []
    for k in range(FRAMES):
        rot = M.rotation("y", (k + 1) * SPIN_DEGREES)
        poses.append(M.pose_from_model(M.column_major(rot, centre - rot @ centre)))
    return poses


def posed_setup(setup, pose):
    s = copy.copy(setup)
    s.scene = copy.copy(setup.scene)
    s.scene.bvhs = setup.scene.bvhs.copy()
    s.scene.bvhs[0]["frame"] = pose[0]
    return s


def oracle_guide(setup):
    import srt_amd as S
    from oracle import pyoracle as O

    w, h = setup.width, setup.height
    o, d = D.camera_rays(*T.as_camera(setup.camera), w, h)
    rays = np.zeros(w * h, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    tri, t, nrm, _ = O.Oracle(setup.scene).trace_closest(setup.bvh_count, rays)
    return D.make_guide(tri.reshape(h, w), t.reshape(h, w), nrm.reshape(h, w, 3))


@functools.lru_cache(maxsize=None)
def orbit(with_accum=True):
    """{"cams", "guides", "accs" (the oracle's accumulation of reset + 1 spp: a sum over 2), "poses" (None), "ref"}."""
    from conftest import oracle_render

    setup = rubik_setup()
    cams, guides, accs = [], [], []
    for cam in orbit_cameras(setup):
        cams.append(T.as_camera(cam))
        guides.append(oracle_guide(setup))
        accs.append(oracle_render(setup, 1)[0] if with_accum else None)
    ref = D.mean_colour(oracle_render(setup, REF_SPP)[0], REF_SPP + 1)
    return {"cams": cams, "guides": guides, "accs": accs, "poses": [None] * len(cams), "ref": ref}


@functools.lru_cache(maxsize=None)
def spin(with_accum=True):
    from conftest import oracle_render

    setup = rubik_setup()
    cam = T.as_camera(setup.camera)
    poses = spin_poses(setup.scene)
    posed = [posed_setup(setup, p) for p in poses]
    guides = [oracle_guide(s) for s in posed]
    accs = [oracle_render(s, 1)[0] if with_accum else None for s in posed]
    ref = D.mean_colour(oracle_render(posed[-1], REF_SPP)[0], REF_SPP + 1)
    return {"cams": [cam] * FRAMES, "guides": guides, "accs": accs, "poses": poses, "ref": ref}


def temporal_pass(seq, accs=None):
    """The restatement over a sequence: per frame (out, moments); accs default to the oracle's."""
    ref = V.VarianceTemporalRef(RUBIK_W, RUBIK_H)
    res = []
    for k, (cam, g, pose) in enumerate(zip(seq["cams"], seq["guides"], seq["poses"])):
        if pose is not None:
            ref.set_models([pose])
        res.append(ref.accumulate_moments((accs or seq["accs"])[k], 2, g, cam))
    return res


def four_images(seq, out, mom, acc, sigma_lum=None, min_history=4):
    """raw 1-spp mean, temporal output, temporal + the existing filter at its defaults, temporal + the variance-guided
    filter, of the last frame."""
    g = seq["guides"][-1]
    kw = {} if sigma_lum is None else {"sigma_lum": sigma_lum}
    return {"raw": D.mean_colour(acc, 2), "temporal": out[..., :3],
            "existing": D.atrous(out[..., :3], g, **EXISTING),
            "variance": V.run_variance(out, 1, g, mom, min_history=min_history, **kw)[0]}


def metrics(seq, images):
    hit = seq["guides"][-1]["tri"] != D.MISS
    return {k: (V.mse(v, seq["ref"], hit), V.mse_tm(v, seq["ref"], hit)) for k, v in images.items()}
