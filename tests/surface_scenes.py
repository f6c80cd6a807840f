"""Shared inputs of the surface-attribute and albedo-demodulation tests and of tools/albedo_floor_grid.py, CPU only
(the oracle and the numpy restatements; no library call that touches a device).

The textured scene is built from arrays: a quad of two triangles that faces the model camera and fills about half of a
64 x 48 frame, its material sampling texture 0 with uvs from (-0.5, -0.5) to (1.5, 1.5) (GL_REPEAT and negative
coordinates occur), an untextured quad with a plain diffuse material beside it, and one light.  Texture 0 is an
8 x 8 RGBA8 checker of two colours in cells of 2 x 2 texels; the quad shows 16 texels across about 36 x 40 pixels,
so a texel covers 5 to 6 pixels.  Texture 1 is 1 x 1 and texture 2 is 5 x 3 with distinct bytes everywhere.
Everything is computed once per process and left unchanged.
"""
from __future__ import annotations

import functools

import numpy as np

import denoise_ref as D
import surface_ref as SR

W, H = 64, 48
SPP, REF_SPP = 4, 256
TEX_ALBEDO = np.asarray([[0.6, 0.5, 0.4], [0.0, 0.0, 0.0]], np.float32)  # the constant-albedo variant
CHECKER = (np.asarray([230, 40, 40, 255], np.uint8), np.asarray([30, 60, 220, 255], np.uint8))


def textures():
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    cell = ((xx // 2) + (yy // 2)) & 1
    t0 = np.where(cell[..., None] == 0, CHECKER[0], CHECKER[1]).astype(np.uint8)
    t1 = np.asarray([[[17, 130, 250, 255]]], np.uint8)
    t2 = (np.arange(60, dtype=np.uint8) * 4 + 3).reshape(3, 5, 4)
    return [t0, t1, t2]


def textured_scene(sample_textures=True, handle=0):
    """The srt_amd.Scene of the two quads (one BVH record: a root over two leaves of two triangles each)."""
    import srt_amd as S

    verts = np.zeros(8, S.VERT_DTYPE)
    # the textured quad: x -18 .. 4.8, y -7.8 .. 25.8 at z = 0; the camera is at (0, 9, 40) looking down -z
    verts["pos"][:4] = [(-18.0, -7.8, 0.0), (4.8, -7.8, 0.0), (4.8, 25.8, 0.0), (-18.0, 25.8, 0.0)]
    verts["uv"][:4] = [(-0.5, -0.5), (1.5, -0.5), (1.5, 1.5), (-0.5, 1.5)]
    verts["pos"][4:] = [(6.4, -3.0, 0.0), (18.0, -3.0, 0.0), (18.0, 21.0, 0.0), (6.4, 21.0, 0.0)]
    tris = np.zeros(4, S.TRI_DTYPE)
    tris["v"] = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]   # wound so that cross(e1, e2) points at the camera
    tris["mat"] = [0, 0, 1, 1]
    mats = np.zeros(2, S.MAT_DTYPE)
    mats["diffuse"] = [(1.0, 1.0, 1.0), (0.7, 0.3, 0.2)]
    mats["Ks"], mats["Ns"] = (0.2, 0.2, 0.2), 10.0
    mats["use_texture"] = [1, 0]
    mats["handle"][0] = (handle & 0xFFFFFFFF, handle >> 32)
    nodes = np.zeros(3, S.NODE_DTYPE)
    nodes["min"] = [(-18.0, -7.8, -0.5), (-18.0, -7.8, -0.5), (6.4, -3.0, -0.5)]
    nodes["max"] = [(18.0, 25.8, 0.5), (4.8, 25.8, 0.5), (18.0, 21.0, 0.5)]
    nodes["first"] = [1, 0, 2]
    nodes["count"] = [0, 2, 2]
    bvhs = np.zeros(1, S.BVH_DTYPE)
    bvhs["count"] = 3
    bvhs["frame"][0] = np.eye(4, dtype=np.float32).reshape(16)
    e1 = verts["pos"][1] - verts["pos"][0]
    e2 = verts["pos"][2] - verts["pos"][0]
    assert np.cross(e1, e2)[2] > 0
    return S.Scene(bvhs, nodes, mats, TEX_ALBEDO.copy(), tris, verts, textures=textures(),
                   sample_textures=sample_textures, tri_input=np.arange(4, dtype=np.uint32))


def textured_setup(w=W, h=H, sample_textures=True):
    import srt_amd as S
    from srt_amd import render as R

    lights = S.lights_array([S.PointLight((0.0, 12.0, 30.0), (1.0, 1.0, 1.0), 400.0)])
    noise = S.generate_noise(w, h, True)
    return R.FrameSetup(w, h, True, textured_scene(sample_textures), lights, noise[0], noise[1], S.Camera(True), 5, 1)


def rubik_setup(w=W, h=H):
    import srt_amd as S
    from conftest import OBJECTS
    from srt_amd import render as R

    return R.make_setup(w, h, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])


def pixel_rays(setup):
    """The pixel-centre rays of setup.camera as RAY_DTYPE records (denoise_ref.camera_rays)."""
    import srt_amd as S

    cam = setup.camera
    o, d = D.camera_rays(cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector(), setup.width,
                         setup.height)
    rays = np.zeros(setup.width * setup.height, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    return rays


def oracle_hits(scene, bvh_count, rays, frame=None):
    """The oracle's closest hits as HIT_DTYPE records (one BVH record can hit: bvh == 0)."""
    import copy

    from oracle import pyoracle as O
    from srt_amd.query import HIT_DTYPE

    if frame is not None:
        scene = copy.copy(scene)
        scene.bvhs = scene.bvhs.copy()
        scene.bvhs["frame"][0] = frame
    tri, t, nrm, _ = O.Oracle(scene).trace_closest(bvh_count, rays)
    hits = np.zeros(len(rays), HIT_DTYPE)
    hit = tri != D.MISS
    hits["triangle"], hits["t"], hits["normal"] = tri, t, nrm
    hits["material"][hit] = scene.tris["mat"][tri[hit]]
    return hits


def scene_albedo(setup, rays, hits):
    """The restated attrs of a setup's scene as the renderer shades it (sampled textures or tex_albedo)."""
    s = setup.scene
    if s.sample_textures:
        return SR.shade(s, rays, hits, textures=s.textures, bvh_count=setup.bvh_count)
    return SR.shade(s, rays, hits, tex_albedo=s.tex_albedo, bvh_count=setup.bvh_count)


@functools.lru_cache(maxsize=None)
def case(name):
    """name: "textured" or "rubik".  {"setup", "rays", "hits", "guide", "attrs", "albedo" (H, W, 3), "acc" (the oracle's
    accumulation of reset + SPP frames), "frames" (SPP + 1), "ref" (the mean of the oracle's REF_SPP frames)}."""
    from conftest import oracle_render

    setup = textured_setup() if name == "textured" else rubik_setup()
    rays = pixel_rays(setup)
    hits = oracle_hits(setup.scene, setup.bvh_count, rays)
    attrs = scene_albedo(setup, rays, hits)
    acc, _, _ = oracle_render(setup, SPP)
    ref_acc, _, _ = oracle_render(setup, REF_SPP)
    return {"setup": setup, "rays": rays, "hits": hits, "guide": D.guide_from_hits(hits, setup.width, setup.height),
            "attrs": attrs, "albedo": attrs["albedo"].reshape(setup.height, setup.width, 3), "acc": acc,
            "frames": SPP + 1, "ref": D.mean_colour(ref_acc, REF_SPP + 1)}


def mse(img, ref, mask):
    return float(np.mean((img[mask].astype(np.float64) - ref[mask].astype(np.float64)) ** 2))


def mse_tm(img, ref, mask):
    """The MSE after x / (1 + x)."""
    a, b = img[mask].astype(np.float64), ref[mask].astype(np.float64)
    return float(np.mean((a / (1 + a) - b / (1 + b)) ** 2))
