"""GPU: temporal reprojection that follows a deforming mesh (include/srt_temporal_deform.h, Temporal.set_mesh /
set_vertices) against the independent numpy float32 restatement (tests/temporal_deform_ref.py): `out` bit for bit
after every frame (bits_equal treats any NaN as equal to any NaN), so frame k + 1 pins the history frame k left.

The sequence is temporal_deform_ref's (the waved 32-triangle grid and a static quad, 37 x 23, 4 frames, CAMERAS[1:5])
with random accumulations; the guide is the GPU's own Query(refit=True) after refit, computed once per module and
checked against the oracle's triangles there.
"""
import numpy as np
import pytest

import denoise_ref as D
import temporal_deform_ref as DR
import temporal_motion_ref as M
from conftest import bits_equal

pytestmark = pytest.mark.gpu

W, H = DR.W, DR.H


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def verts_dev(torch, verts):
    return torch.from_numpy(verts.view(np.float32).reshape(-1, 8).copy()).cuda()


def spin_pose(k):
    """Record 0 turned by 1.5 degrees per frame about z through the grid's middle."""
    rot = M.rotation("z", 1.5 * k)
    centre = np.array([-0.7, 0.0, 0.0])
    return M.pose_from_model(M.column_major(rot, centre - rot @ centre))


@pytest.fixture(scope="module")
def frames(torch):
    """Per variant ("wave": identity frames; "spin": record 0 posed by spin_pose(k)) and frame: (cam, verts, hits on
    the host, accum).  The guide is the refit query's, with the oracle's triangles."""
    from srt_amd.query import Query

    scene, ids = DR.grid_scene()
    rng = np.random.default_rng(77)
    out = {"scene": scene, "wave": [], "spin": []}
    with Query(scene, refit=True) as q:
        for variant in ("wave", "spin"):
            for k, cam in enumerate(DR.sequence_cameras()):
                verts = DR.waved(scene, ids, k)
                if variant == "spin":
                    q.update_model_matrix(0, spin_pose(k)[0])
                q.refit(verts_dev(torch, verts))
                rays = DR.pixel_rays(cam)  # denoise_ref.camera_rays: the pixel-centre rays, as the oracle is given them
                hits = q.closest(torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()).numpy()
                if variant == "wave":
                    want = DR.oracle_guide(scene, verts, cam)
                    assert (hits["triangle"].reshape(H, W) == want["tri"]).all() and (hits["bvh"].reshape(H, W) == want["bvh"]).all()
                    assert bits_equal(hits["t"].reshape(H, W), want["t"]).all()
                acc = np.ones((H, W, 4), np.float32)
                acc[..., :3] = rng.uniform(0, 6, (H, W, 3)).astype(np.float32)
                out[variant].append((cam, verts, hits, acc))
    return out


def hits_dev(torch, hits):
    return torch.from_numpy(hits.view(np.int32).reshape(-1, 8).copy()).cuda()


def step(torch, tp, ref, cam, hits, acc, moments=False):
    """One frame through the GPU object and the restatement; asserts they agree bit for bit; returns the restatement's."""
    g = D.guide_from_hits(hits, W, H)
    if moments:
        got, gm = tp.accumulate_moments(to_dev(torch, acc), 3, hits_dev(torch, hits), cam)
        want, wm = ref.accumulate_moments(acc, 3, g, cam)
    else:
        got = tp.accumulate(to_dev(torch, acc), 3, hits_dev(torch, hits), cam)
        want = ref.accumulate(acc, 3, g, cam)
    tp.synchronize()
    bad = int((~bits_equal(got.cpu().numpy(), want)).sum())
    if moments:
        bad += int((~bits_equal(gm.cpu().numpy(), wm)).sum())
    print(f"frame {ref.frames - 1}: {bad} words differ; {int(ref.deforming.sum())} DEFORMING pixels")
    assert bad == 0
    return want


def attach(tp, ref, scene, tris=None):
    tris = scene.tris if tris is None else tris
    tp.set_mesh(tris, len(scene.verts))
    ref.set_mesh(tris, len(scene.verts))


def set_verts(torch, tp, ref, verts):
    tp.set_vertices(None if verts is None else verts_dev(torch, verts))
    ref.set_vertices(verts)


def test_wave_only(torch, frames):
    """(i) No poses: launches are the kernel and the copy; the result differs from a history that ignores the wave."""
    from srt_amd.temporal import Temporal

    scene = frames["scene"]
    ref, plain = DR.TemporalDeformRef(W, H), M.TemporalMotionRef(W, H)
    with Temporal(W, H) as tp:
        attach(tp, ref, scene)
        assert tp.get_int("mesh.tris") == len(scene.tris) and tp.get_int("mesh.verts") == len(scene.verts)
        assert tp.get_int("mesh.bytes") == 16 * (len(scene.tris) + len(scene.verts)) and tp.get_int("scratch.bytes") == 72 * W * H
        for k, (cam, verts, hits, acc) in enumerate(frames["wave"]):
            set_verts(torch, tp, ref, verts)
            want = step(torch, tp, ref, cam, hits, acc)
            want_plain = plain.accumulate(acc, 3, D.guide_from_hits(hits, W, H), cam)
            assert tp.get_int("launches") == 2 and tp.get_int("deform") == 1
            assert ref.deforming.any() == (k > 0)
    kept = ref.deforming & (want[..., 3] > 1)
    assert kept.sum() >= 0.25 * (hits["triangle"] != D.MISS).sum()
    assert (~bits_equal(want, want_plain).all(-1))[kept].mean() >= 0.9  # a device that ignored the wave would fail above


def test_wave_and_a_spinning_pose(torch, frames):
    """(ii) Record 0 also turns (n_Q = 1), so record 1 takes the r >= n_Q branch; first stated after frame 0, so frame 1
    has n_P = 0 < r + 1 = n_Q and A is Q's; launches are 1 + 1 + 1 + 1."""
    from srt_amd.temporal import Temporal

    scene = frames["scene"]
    ref = DR.TemporalDeformRef(W, H)
    with Temporal(W, H) as tp:
        attach(tp, ref, scene)
        for k, (cam, verts, hits, acc) in enumerate(frames["spin"]):
            if k:
                pose = spin_pose(k)
                tp.set_models([pose[0]], [pose[1]])
                ref.set_models([pose])
            set_verts(torch, tp, ref, verts)
            want = step(torch, tp, ref, cam, hits, acc)
            assert tp.get_int("launches") == (4 if k else 2) and tp.get_int("deform") == 1
        assert tp.get_int("mesh.bytes") == 16 * (len(scene.tris) + len(scene.verts)) + 96 and tp.get_int("models.bytes") == 64
    g = D.guide_from_hits(hits, W, H)
    assert (ref.deforming & (want[..., 3] > 1)).sum() >= 0.25 * (g["tri"] != D.MISS).sum()
    assert ((g["bvh"] == 1) & (g["tri"] != D.MISS) & (want[..., 3] > 1)).sum() > 10  # record 1, past the poses, keeps its history


def test_moments_instance(torch, frames):
    """(iii) accumulate_moments under the wave and the pose: out and (m1, m2, v, N) bit for bit."""
    from srt_amd.temporal import Temporal

    scene = frames["scene"]
    ref = DR.TemporalDeformRef(W, H)
    with Temporal(W, H) as tp:
        tp.enable_moments()
        attach(tp, ref, scene)
        for k, (cam, verts, hits, acc) in enumerate(frames["spin"]):
            pose = spin_pose(k)
            tp.set_models([pose[0]], [pose[1]])
            ref.set_models([pose])
            set_verts(torch, tp, ref, verts)
            step(torch, tp, ref, cam, hits, acc, moments=True)
            assert tp.get_int("launches") == 4 and tp.get_int("deform") == 1
    assert ref.deforming.sum() > 100


def test_indices_past_the_arrays(torch, frames):
    """(iv) Triangle 3 names a vertex >= n_verts (it reads zeros in V and V'), and the guide names triangles >= n_tris
    in a block of pixels (RIGID): the restatement's values, and nothing read past an array."""
    from srt_amd.temporal import Temporal

    scene = frames["scene"]
    tris = scene.tris.copy()
    tris["v"][3, 1] = len(scene.verts)
    tris["v"][5, 2] = 0xFFFFFFF0
    ref = DR.TemporalDeformRef(W, H)
    seen = 0
    with Temporal(W, H) as tp:
        attach(tp, ref, scene, tris)
        for cam, verts, hits, acc in frames["wave"]:
            hits = hits.copy()
            block = hits["triangle"].reshape(H, W)[8:14, 4:12]
            seen += int(np.isin(hits["triangle"], (3, 5)).sum())
            block[block != D.MISS] = np.array([len(tris), len(tris) + 7, 0x7FFFFFFF, 0xFFFFFFFE], np.uint32)[np.arange((block != D.MISS).sum()) % 4]
            set_verts(torch, tp, ref, verts)
            step(torch, tp, ref, cam, hits, acc)
            past = (hits["triangle"].reshape(H, W) >= len(tris)) & (hits["triangle"].reshape(H, W) != D.MISS)
            assert past.sum() > 20 and not ref.deforming[past].any()
    assert seen > 20


def test_unchanged_vertices_equal_no_mesh(torch, frames):
    """(v) The same vertices every frame: bit-identical to an object without a mesh, while a deform instance runs and
    one more launch is enqueued; (vi) the object never given a mesh matches TemporalMotionRef with today's launches."""
    from srt_amd.temporal import Temporal

    scene = frames["scene"]
    ref = M.TemporalMotionRef(W, H)
    with Temporal(W, H) as meshed, Temporal(W, H) as bare:
        meshed.set_mesh(scene)
        v = verts_dev(torch, frames["wave"][0][1])
        for cam, _, hits, acc in frames["wave"]:
            meshed.set_vertices(v)
            a = meshed.accumulate(to_dev(torch, acc), 3, hits_dev(torch, hits), cam)
            b = bare.accumulate(to_dev(torch, acc), 3, hits_dev(torch, hits), cam)
            meshed.synchronize()
            bare.synchronize()
            want = ref.accumulate(acc, 3, D.guide_from_hits(hits, W, H), cam)
            assert bits_equal(a.cpu().numpy(), want).all() and bits_equal(b.cpu().numpy(), want).all()
            assert meshed.get_int("deform") == 1 and meshed.get_int("launches") == 2
            assert bare.get_int("deform") == 0 and bare.get_int("launches") == 1
        for name in ("mesh.tris", "mesh.verts", "mesh.bytes", "deform"):
            assert bare.get_int(name) == 0
    assert (want[..., 3] > 1).mean() > 0.1


def test_fallbacks(torch, frames):
    """(vii) reset, set_vertices(None) and set_mesh(n_tris = 0) each give the stated behaviour on the next frame; the
    argument errors leave the state as it was."""
    from srt_amd import SrtError, _lib
    from srt_amd.temporal import Temporal

    scene = frames["scene"]
    seq = frames["wave"]
    ref = DR.TemporalDeformRef(W, H)

    def frame(tp, k, verts="own"):
        cam, own, hits, acc = seq[k % len(seq)]
        if verts == "own":
            set_verts(torch, tp, ref, own)
        return step(torch, tp, ref, cam, hits, acc)

    with Temporal(W, H) as tp:
        with pytest.raises(SrtError) as e:  # no mesh yet
            tp.set_vertices(verts_dev(torch, seq[0][1]))
        assert e.value.code == _lib.SRT_ERR_INVALID and "no mesh" in str(e.value)
        attach(tp, ref, scene)
        good = verts_dev(torch, seq[0][1])
        for bad in (torch.cat([good, good[:1]]), good[:-1].contiguous()):
            with pytest.raises(SrtError) as e:
                tp.set_vertices(bad)
            assert e.value.code == _lib.SRT_ERR_INVALID and "n_verts" in str(e.value)
        flat = torch.zeros(8 * len(good) + 1, dtype=torch.float32, device="cuda")
        with pytest.raises(SrtError) as e:
            tp.set_vertices(flat[1:].view(len(good), 8))
        assert e.value.code == _lib.SRT_ERR_INVALID and "aligned" in str(e.value)
        with pytest.raises(ValueError):
            tp.set_vertices(good.cpu())
        del e, bad
        frame(tp, 0, verts=None)  # a mesh without V: today's kernels
        assert tp.get_int("deform") == 0 and tp.get_int("launches") == 1
        frame(tp, 0)
        frame(tp, 1)
        assert ref.deforming.any() and tp.get_int("launches") == 2
        tp.reset()
        ref.reset()
        out = frame(tp, 2)  # no history: (C, 1) everywhere, and V' is made again
        assert (out[..., 3] == 1).all() and not ref.deforming.any() and tp.get_int("deform") == 1
        frame(tp, 3)
        assert ref.deforming.any()
        set_verts(torch, tp, ref, None)  # every pixel RIGID, today's kernels, V' dropped
        frame(tp, 0, verts=None)
        assert tp.get_int("deform") == 0 and tp.get_int("launches") == 1 and not ref.deforming.any()
        frame(tp, 1)  # V again, V' absent: RIGID for one frame
        assert tp.get_int("deform") == 1 and not ref.deforming.any()
        frame(tp, 2)
        assert ref.deforming.any()
        tp.set_mesh(None)
        ref.set_mesh(np.zeros((0, 3), np.int64), 0)
        frame(tp, 3, verts=None)
        assert tp.get_int("deform") == 0 and tp.get_int("launches") == 1 and tp.get_int("mesh.bytes") == 0
        assert tp.get_int("frames") == 6  # since the reset
