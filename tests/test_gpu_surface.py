"""GPU: the surface-attribute stage (include/srt_surface.h, srt_amd.surface.Surface) against the independent numpy
float32 restatement (tests/surface_ref.py, which never calls into the library): every field of every record, bit for
bit.  The hits come from the GPU's own Query over the same rays and are first checked against the oracle's.
"""
import numpy as np
import pytest

import surface_ref as SR
import surface_scenes as SS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def rays_dev(torch, rays):
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def hits_dev(torch, hits):
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.int32).reshape(-1, 8).copy()).cuda()


def gpu_attrs(torch, surf, rays, hits):
    from srt_amd.surface import ATTR_DTYPE

    out = surf.shade(rays_dev(torch, rays), hits_dev(torch, hits))
    surf.synchronize()
    assert tuple(out.shape) == (len(rays), 8) and out.dtype == torch.float32
    return out.cpu().numpy().view(ATTR_DTYPE).reshape(-1)


def assert_same(got, want):
    for f in ("albedo", "bary_v", "bary_w", "uv", "hit"):
        bad = got[f].view(np.uint32) != want[f].view(np.uint32)
        print(f"{f}: {int(bad.sum())} of {bad.size} words differ")
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def gpu_hits(torch, scene, bvh_count, rays, frame=None):
    """The library's closest hits of `rays`, checked against the oracle's triangles and distances."""
    from srt_amd.query import Query

    with Query(scene) as q:
        q.set_bvh_count(bvh_count)
        if frame is not None:
            q.update_model_matrix(0, frame)
        hits = q.closest(rays_dev(torch, rays)).numpy()
    want = SS.oracle_hits(scene, bvh_count, rays, frame)
    assert (hits["triangle"] == want["triangle"]).all() and (hits["t"].view(np.uint32) == want["t"].view(np.uint32)).all()
    assert (hits["material"] == want["material"]).all() and (hits["bvh"] == 0).all()
    return hits


@pytest.fixture(scope="module")
def textured():
    setup = SS.textured_setup()
    return setup, SS.pixel_rays(setup)


def test_rubik_constant_albedo(torch):
    """Rubik at 64 x 48: tex_albedo / diffuse materials, hits and misses mixed."""
    from srt_amd.surface import Surface

    setup = SS.rubik_setup()
    rays = SS.pixel_rays(setup)
    hits = gpu_hits(torch, setup.scene, setup.bvh_count, rays)
    hit = hits["triangle"] != SR.MISS
    assert 0.1 < hit.mean() < 0.9
    with Surface(setup.scene) as surf:
        assert surf.get_int("textures") == 0 and surf.get_int("bvh_count") == 1 and surf.get_int("launch.block") == 256
        got = gpu_attrs(torch, surf, rays, hits)
        assert surf.get_int("launch.blocks") == (64 * 48 + 255) // 256
    want = SS.scene_albedo(setup, rays, hits)
    assert_same(got, want)
    assert (got["hit"] == hit).all() and len(np.unique(got["albedo"][hit], axis=0)) > 2


def test_textured_scene_sampled_and_constant(torch, textured):
    """tex_albedo = NULL: texture 0 is sampled at the hit's uv (GL_REPEAT, negative coordinates); tex_albedo given:
    the constant.  Barycentrics and uv are the same in both and are written for the plain quad too."""
    from srt_amd.surface import Surface

    setup, rays = textured
    scene = setup.scene
    hits = gpu_hits(torch, scene, 1, rays)
    with Surface(scene) as surf:
        assert surf.get_int("textures") == 3
        sampled = gpu_attrs(torch, surf, rays, hits)
    assert_same(sampled, SR.shade(scene, rays, hits, textures=scene.textures))
    quad = hits["triangle"] < 2
    assert len(np.unique(sampled["albedo"][quad], axis=0)) > 20              # the checker and its blends
    const_scene = SS.textured_scene(sample_textures=False)
    with Surface(const_scene) as surf:
        assert surf.get_int("textures") == 0
        const = gpu_attrs(torch, surf, rays, hits)
    assert_same(const, SR.shade(scene, rays, hits, tex_albedo=SS.TEX_ALBEDO))
    plain = (hits["triangle"] != SR.MISS) & ~quad
    assert (const["uv"][plain] == 0).all() and (const["bary_v"][plain] != 0).any()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_partial_waves_and_blocks(torch, textured, n):
    """A window of n rays of row 20 from pixel 10 on: it starts on the textured quad and, from 63 rays on, crosses the
    gap between the quads (misses and hits in one wave)."""
    from srt_amd.surface import Surface

    setup, rays = textured
    first = 20 * SS.W + 10
    hits = SS.oracle_hits(setup.scene, 1, rays)
    r, h = rays[first:first + n], hits[first:first + n]
    assert h["triangle"][0] != SR.MISS and (n == 1 or (h["triangle"] == SR.MISS).any())
    with Surface(setup.scene) as surf:
        got = gpu_attrs(torch, surf, r, h)
        assert surf.get_int("launch.blocks") == (n + 255) // 256
    assert_same(got, SR.shade(setup.scene, r, h, textures=setup.scene.textures))


def test_zero_rays_launch_nothing(torch, textured):
    from srt_amd.surface import Surface

    setup, rays = textured
    hits = SS.oracle_hits(setup.scene, 1, rays)
    with Surface(setup.scene) as surf:
        gpu_attrs(torch, surf, rays[:300], hits[:300])
        assert surf.get_int("launch.blocks") == 2
        out = surf.shade(rays_dev(torch, rays[:0]), hits_dev(torch, hits[:0]))
        surf.synchronize()
        assert tuple(out.shape) == (0, 8) and surf.get_int("launch.blocks") == 2


def test_unknown_handle_one_texel_texture_and_replaced_set(torch, textured):
    """Handle 7 with three textures uploaded, and a handle past 2^32: zero albedo with hit = 1 and the usual uv;
    handle 1 samples the 1 x 1 texture (its one colour everywhere); upload_textures replaces the set."""
    from srt_amd.surface import Surface

    setup, rays = textured
    hits = SS.oracle_hits(setup.scene, 1, rays)
    quad = hits["triangle"] < 2
    for handle in (7, 1 << 32):
        scene = SS.textured_scene(handle=handle)
        with Surface(scene) as surf:
            got = gpu_attrs(torch, surf, rays, hits)
        assert_same(got, SR.shade(scene, rays, hits, textures=scene.textures))
        assert (got["albedo"][quad] == 0).all() and (got["hit"][quad] == 1).all() and (got["uv"][quad] != 0).any()
    scene = SS.textured_scene(handle=1)
    with Surface(scene) as surf:
        got = gpu_attrs(torch, surf, rays, hits)
        assert_same(got, SR.shade(scene, rays, hits, textures=scene.textures))
        one = scene.textures[1][0, 0, :3].astype(np.float32) / np.float32(255)
        assert (np.abs(got["albedo"][quad] - one) <= 1e-6).all()          # four equal texels, weights summing to 1 within a few ulp
        # a new set: handle 1 is now the 5 x 3 texture, and two textures are known
        surf.upload_textures([scene.textures[0], scene.textures[2]])
        assert surf.get_int("textures") == 2
        got = gpu_attrs(torch, surf, rays, hits)
        assert_same(got, SR.shade(scene, rays, hits, textures=[scene.textures[0], scene.textures[2]]))
        assert len(np.unique(got["albedo"][quad], axis=0)) > 20


def test_update_model_matrix(torch, textured):
    """A rotated and translated frame on both the query and the surface object."""
    from srt_amd.surface import Surface

    setup, rays = textured
    ang = np.deg2rad(20.0)
    rot = np.asarray([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, (1.5, -2.0, 3.0)
    frame = np.ascontiguousarray(m.T, np.float32).reshape(16)                # column-major
    hits = gpu_hits(torch, setup.scene, 1, rays, frame)
    hit = hits["triangle"] != SR.MISS
    assert 0.2 < hit.mean() < 0.9
    with Surface(setup.scene) as surf:
        before = gpu_attrs(torch, surf, rays, hits)
        surf.update_model_matrix(0, frame)
        got = gpu_attrs(torch, surf, rays, hits)
    want = SR.shade(setup.scene, rays, hits, textures=setup.scene.textures, frames=frame[None])
    assert_same(got, want)
    assert (before["bary_v"][hit] != got["bary_v"][hit]).mean() > 0.9
    v, w = got["bary_v"][hit], got["bary_w"][hit]
    assert (v > -1e-3).all() and (w > -1e-3).all() and (v + w < 1 + 1e-3).all()  # the hit lies in its triangle


def test_bvh_count_below_n_bvhs(torch, textured):
    """bvh_count = 0 with one record: every hit reads the zero frame (mp = 0), still a hit record."""
    from srt_amd.surface import Surface

    setup, rays = textured
    hits = SS.oracle_hits(setup.scene, 1, rays)
    with Surface(setup.scene) as surf:
        surf.set_bvh_count(0)
        assert surf.get_int("bvh_count") == 0
        got = gpu_attrs(torch, surf, rays, hits)
    want = SR.shade(setup.scene, rays, hits, textures=setup.scene.textures, bvh_count=0)
    assert_same(got, want)
    hit = hits["triangle"] != SR.MISS
    assert (got["hit"] == hit).all() and len(np.unique(got["bary_v"][hits["triangle"] == 0])) == 1


def test_all_misses(torch, textured):
    from srt_amd.surface import Surface

    setup, rays = textured
    hits = SS.oracle_hits(setup.scene, 1, rays)[:700].copy()
    hits["triangle"] = SR.MISS
    with Surface(setup.scene) as surf:
        got = gpu_attrs(torch, surf, rays[:700], hits)
    assert (got.view(np.uint32) == 0).all()
