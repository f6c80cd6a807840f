"""The references of the deforming-mesh extension alone (tests/temporal_deform_ref.py), CPU only, with the guide from
the oracle: the shared sequence is not vacuous, following the deformation matters, and the deform reference differs
from temporal_motion_ref where it should and nowhere else.

The sequence (temporal_deform_ref): refit_ref.grid_triangles(4) -- 32 triangles -- as record 0, waved with amplitude
0.25 and a phase that advances by 0.6 per frame, and a static quad as record 1; 37 x 23 (no multiple of the kernel's
64 x 4 tile), 4 frames under temporal_motion_ref's CAMERAS[1:5].  Each frame's accumulation is a noise-free pattern
fixed to the material: a function of the triangle index and the hit's barycentrics.

Recorded at these settings, last frame: 423 hit pixels, 334 DEFORMING with N' > 1 (0.790), 80 RIGID (0.189), 9
DEFORMING rejected; over the 256 DEFORMING interior pixels mean |out - C| is 0.1194 with the mesh attached and 0.2551
through TemporalMotionRef, which ignores the deformation.
"""
import functools

import numpy as np

import denoise_ref as D
import temporal_deform_ref as DR
import temporal_motion_ref as M
from conftest import bits_equal


@functools.lru_cache(maxsize=None)
def sequence():
    """Per frame (cam, verts, guide, accum); the oracle traces each frame's host-refit scene once."""
    scene, ids = DR.grid_scene()
    frames = []
    for k, cam in enumerate(DR.sequence_cameras()):
        verts = DR.waved(scene, ids, k)
        g = DR.oracle_guide(scene, verts, cam)
        bv, bw = DR.hit_barycentrics(g, verts, scene.tris, cam)
        acc = np.ones((DR.H, DR.W, 4), np.float32)
        acc[..., :3] = DR.material_pattern(g["tri"], bv, bw)
        frames.append((cam, verts, g, acc))
    return scene, frames


@functools.lru_cache(maxsize=None)
def run():
    """The sequence through the deform reference and through TemporalMotionRef: the last frame's results."""
    scene, frames = sequence()
    ref, plain = DR.TemporalDeformRef(DR.W, DR.H), M.TemporalMotionRef(DR.W, DR.H)
    ref.set_mesh(scene.tris, len(scene.verts))
    classes = []
    for cam, verts, g, acc in frames:
        ref.set_vertices(verts)
        out, out_plain = ref.accumulate(acc, 1, g, cam), plain.accumulate(acc, 1, g, cam)
        classes.append(ref.deforming.copy())
    return out, out_plain, classes, g, acc


def test_the_sequence_is_not_vacuous():
    out, _, classes, g, _ = run()
    hit, deforming, n = g["tri"] != D.MISS, classes[-1], out[..., 3]
    assert not classes[0].any()  # the first frame has neither a history nor V'
    assert (deforming <= (hit & (g["bvh"] == 0))).all() and not deforming[g["bvh"] == 1].any()
    kept, rigid, rejected = (deforming & (n > 1)).sum(), (hit & ~deforming).sum(), (deforming & (n == 1)).sum()
    print(f"{hit.sum()} hit pixels: {kept} DEFORMING with N' > 1 ({kept / hit.sum():.3f}), {rigid} RIGID "
          f"({rigid / hit.sum():.3f}), {rejected} DEFORMING rejected")
    assert kept >= 0.25 * hit.sum()
    assert rigid >= 0.05 * hit.sum()
    assert rejected >= 1


def test_following_the_deformation_matters():
    out, out_plain, classes, _, acc = run()
    inner = M.interior(classes[-1])
    C = acc[..., :3]
    with_mesh, without = np.abs(out[..., :3] - C)[inner].mean(), np.abs(out_plain[..., :3] - C)[inner].mean()
    print(f"{inner.sum()} DEFORMING interior pixels: mean |out - C| {with_mesh:.4f} with the mesh, {without:.4f} without")
    assert inner.sum() > 100
    assert with_mesh < without


def test_the_references_differ_where_the_surface_deforms():
    out, out_plain, classes, g, _ = run()
    deforming = classes[-1]
    differ = ~bits_equal(out, out_plain).all(-1)
    kept = deforming & (out[..., 3] > 1)
    print(f"{differ.sum()} pixels differ; {kept.sum()} DEFORMING with N' > 1, of which {(differ & kept).sum()} differ")
    assert differ[kept].mean() >= 0.9 and differ.sum() >= 0.25 * (g["tri"] != D.MISS).sum()
    # the quad (record 1, RIGID) keeps TemporalMotionRef's result where its taps never met the grid's history
    quad = M.interior((g["bvh"] == 1) & (g["tri"] != D.MISS))
    assert quad.sum() > 10 and not differ[quad].any()


def test_unchanged_vertices_and_no_mesh_are_temporal_motion_ref():
    """A mesh whose vertices never change, and an object without V, are bit-identical to TemporalMotionRef; the moments
    variant agrees with variance_ref's in the same way."""
    import variance_ref as VR

    scene, frames = sequence()
    still, bare, plain = (DR.TemporalDeformRef(DR.W, DR.H) for _ in range(3))
    moments = VR.VarianceTemporalRef(DR.W, DR.H)
    still.set_mesh(scene.tris, len(scene.verts))
    bare.set_mesh(scene.tris, len(scene.verts))
    for cam, _, g, acc in frames:
        still.set_vertices(scene.verts)
        a, ma = still.accumulate_moments(acc, 1, g, cam)
        b, c = bare.accumulate(acc, 1, g, cam), plain.accumulate(acc, 1, g, cam)
        d, md = moments.accumulate_moments(acc, 1, g, cam)
        assert not still.deforming.any()
        assert bits_equal(a, b).all() and bits_equal(a, c).all() and bits_equal(a, d).all() and bits_equal(ma, md).all()
    assert (a[..., 3] > 1).mean() > 0.2
