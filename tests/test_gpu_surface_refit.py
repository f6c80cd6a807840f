"""GPU: the device refit of a surface object (include/srt_surface_refit.h, Surface(scene, refit=True).refit) on
surface_scenes.textured_scene and Rubik at 32 x 24: the srt_surface_attr records of a refit query's hits against the
numpy restatement on the deformed vertices (tests/surface_refit_ref.py) and against a surface object freshly created
from them, bit for bit; and tools/render.py's deforming frame loop end to end, as a child process.
"""
import subprocess
import sys

import numpy as np
import pytest

import refit_ref as RR
import surface_ref as SR
import surface_refit_ref as SRR
import surface_scenes as SS
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = 32, 24


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev(torch, records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.float32).reshape(-1, 8).copy()).cuda()


def attrs_of(surf, rays, hits):
    from srt_amd.surface import ATTR_DTYPE

    out = surf.shade(rays, hits)
    surf.synchronize()
    return out.cpu().numpy().view(ATTR_DTYPE).reshape(-1)


def same(got, want):
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{bad} of {got.view(np.uint32).size} words differ")
    return bad == 0


def shade_kw(setup):
    s = setup.scene
    kw = {"textures": s.textures} if s.sample_textures else {"tex_albedo": s.tex_albedo}
    return dict(kw, bvh_count=setup.bvh_count)


@pytest.mark.parametrize("name", ["textured", "rubik"])
def test_refit_matches_the_restatement_and_a_fresh_object(torch, name):
    from srt_amd.query import Query
    from srt_amd.surface import Surface

    setup = SS.textured_setup(W, H) if name == "textured" else SS.rubik_setup(W, H)
    scene, kw = setup.scene, shade_kw(setup)
    verts = RR.wave(scene.verts, 0.5 if name == "textured" else RR.WAVE_AMPLITUDE, 0.3)
    rays_host = SS.pixel_rays(setup)
    rays = dev(torch, rays_host)
    with Query(scene, refit=True) as q, Surface(scene, refit=True) as surf, Surface(SRR.scene_at(scene, verts)) as fresh:
        q.set_bvh_count(setup.bvh_count)
        assert surf.get_int("refit") == 1 and surf.get_int("refit.bytes") == 16 * len(scene.tris) and surf.get_int("refit.count") == 0
        assert fresh.get_int("refit") == 0 and fresh.get_int("refit.bytes") == 0
        hits0 = q.closest(rays)
        before = attrs_of(surf, rays, hits0)
        assert same(before, SR.shade(scene, rays_host, hits0.numpy(), **kw))
        v = dev(torch, verts)
        q.refit(v)
        surf.refit(v)
        assert surf.get_int("refit.count") == 1
        hits1 = q.closest(rays)
        h1 = hits1.numpy()
        got = attrs_of(surf, rays, hits1)
        want = SRR.shade_refit(scene, verts, rays_host, h1, **kw)
        hit = h1["triangle"] != SR.MISS
        assert hit.sum() > 50 and same(got, want)
        assert same(got, attrs_of(fresh, rays, hits1))
        # the refit is no no-op: on the pixels both meshes hit, the barycentrics moved
        both = hit & (hits0.numpy()["triangle"] == h1["triangle"])
        assert both.sum() > 20 and (before["bary_v"][both].view(np.uint32) != got["bary_v"][both].view(np.uint32)).mean() > 0.5
        # the numpy path, and back to the original vertices: the original records
        surf.refit(scene.verts)
        q.refit(scene.verts)
        assert surf.get_int("refit.count") == 2
        assert same(attrs_of(surf, rays, q.closest(rays)), before)


def test_an_object_without_the_flag_refuses_and_shades_as_before(torch):
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query
    from srt_amd.surface import Surface

    setup = SS.textured_setup(W, H)
    scene = setup.scene
    rays_host = SS.pixel_rays(setup)
    rays = dev(torch, rays_host)
    good = dev(torch, RR.wave(scene.verts, 0.5, 0.3))
    with Query(scene) as q, Surface(scene) as plain, Surface(scene, refit=True) as flagged:
        hits = q.closest(rays)
        before = attrs_of(plain, rays, hits)
        assert same(before, attrs_of(flagged, rays, hits))
        with pytest.raises(SrtError) as e:
            plain.refit(good)
        assert e.value.code == _lib.SRT_ERR_INVALID and "without SRT_SURFACE_REFIT" in str(e.value)
        assert plain.get_int("refit.count") == 0 and same(attrs_of(plain, rays, hits), before)
        # the flagged object's argument errors enqueue nothing
        for bad in (torch.cat([good, good[:1]]), good[:-1].contiguous()):
            with pytest.raises(SrtError) as e:
                flagged.refit(bad)
            assert e.value.code == _lib.SRT_ERR_INVALID and "n_verts" in str(e.value)
        flat = torch.zeros(8 * len(good) + 1, dtype=torch.float32, device="cuda")
        with pytest.raises(SrtError) as e:
            flagged.refit(flat[1:].view(len(good), 8))
        assert e.value.code == _lib.SRT_ERR_INVALID and "aligned" in str(e.value)
        with pytest.raises(ValueError):
            flagged.refit(good.cpu())
        del e, bad
        assert flagged.get_int("refit.count") == 0 and same(attrs_of(flagged, rays, hits), before)
        assert same(before, SR.shade(scene, rays_host, hits.numpy(), **shade_kw(setup)))


def test_render_tool_deforming_frame_loop(tmp_path):
    """tools/render.py --wave 0.25 --orbit 3 --denoise --albedo on Rubik at 64 x 48, 1 spp, in a fresh child process:
    it exits 0 and writes its three images, every pixel finite."""
    import srt_amd as S  # noqa: F401  (the package's image reader below)
    from PIL import Image

    out = tmp_path / "frame.png"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "render.py"), "--scene", "rubik", "--width", "64", "--height", "48",
                        "--spp", "1", "--wave", "0.25", "--orbit", "3", "--denoise", "--albedo", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for suffix in ("", "_denoised", "_temporal"):
        p = tmp_path / f"frame{suffix}.png"
        assert p.exists(), (p, r.stdout)
        img = np.asarray(Image.open(p), np.float32)
        assert img.shape[:2] == (48, 64) and np.isfinite(img).all() and img[..., :3].max() > 0
