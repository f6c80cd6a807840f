"""The numpy restatement of srt_surface_refit (include/srt_surface_refit.h), for the tests: a surface object refit to
new vertices answers as surface_ref.shade does over a scene that holds those vertices -- the positions change, the
uvs, the triangles, the materials and the frames stay.  It never calls into the library's device code.
"""
from __future__ import annotations

import copy

import numpy as np

import surface_ref as SR


def scene_at(scene, verts):
    """A shallow copy of `scene` whose vertex POSITIONS are `verts`' (a VERT_DTYPE array); its uvs stay the scene's."""
    assert len(verts) == len(scene.verts)
    s = copy.copy(scene)
    s.verts = scene.verts.copy()
    s.verts["pos"] = np.asarray(verts["pos"], np.float32)
    return s


def shade_refit(scene, verts, rays, hits, **kw):
    """surface_ref.shade of `hits` (a query refit to `verts`) after srt_surface_refit(verts)."""
    return SR.shade(scene_at(scene, verts), rays, hits, **kw)


def triangle_words(scene, verts):
    """The three words srt_surface_refit rewrites per triangle, (n_tris, 9) float32: v0, v1 - v0, v2 - v0."""
    p = np.asarray(verts["pos"], np.float32)[scene.tris["v"]]
    return np.concatenate([p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], axis=1).astype(np.float32)
