"""GPU: albedo-demodulated denoising (srt_denoise_run_albedo, Denoiser.run_albedo) against the numpy float32
restatement (tests/denoise_albedo_ref.py over tests/denoise_ref.py, which never call into the library), bit for bit on
the float output and on sRGB8.

The inputs are the oracle's 4-spp accumulation, the oracle's hits and the restated albedo of tests/surface_scenes.py
(computed once per process), so a difference can only come from the filter.  bits_equal treats any NaN as any NaN.
"""
import numpy as np
import pytest

import denoise_albedo_ref as DA
import denoise_ref as D
import surface_scenes as SS
from conftest import bits_equal
from test_gpu_denoise import srgb8

pytestmark = pytest.mark.gpu

DEFAULTS = dict(passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).reshape(-1, 8).copy()).cuda()


def gpu_run_albedo(torch, dn, acc, frames, hits, attrs, floor=None, srgb=False):
    kw = {} if floor is None else {"albedo_floor": floor}
    res = dn.run_albedo(torch.from_numpy(np.ascontiguousarray(acc)).cuda(), frames, dev(torch, hits, np.int32),
                        dev(torch, attrs, np.float32), srgb=srgb, **kw)
    dn.synchronize()
    return tuple(r.cpu().numpy() for r in res) if srgb else res.cpu().numpy()


def check(got, want, what):
    bad = ~bits_equal(got[..., :3], want)
    print(f"{what}: {int(bad.sum())} of {bad.size} components differ")
    assert not bad.any()
    assert (got[..., 3] == 1.0).all()


@pytest.mark.parametrize("name", ["textured", "rubik"])
def test_bit_exact_over_pass_counts(torch, name):
    """64 x 48 at 4 spp, the default floor: passes 1 (first = last), 2 (tiled + direct), 3 and 5 (steps past
    tile.max_step); the sRGB8 image is the float image's encoding."""
    from srt_amd.denoise import ALBEDO_FLOOR, Denoiser

    c = SS.case(name)
    assert ALBEDO_FLOOR == 0.1
    with Denoiser(SS.W, SS.H) as dn:
        assert dn.get_int("tile.max_step") == 1
        for passes in (1, 2, 3, 5):
            dn.set_params(passes=passes)
            f32, u8 = gpu_run_albedo(torch, dn, c["acc"], c["frames"], c["hits"], c["attrs"], srgb=True)
            assert dn.get_int("launches") == passes
            want = DA.run_albedo(c["acc"], c["frames"], c["guide"], c["albedo"], ALBEDO_FLOOR, **dict(DEFAULTS, passes=passes))
            check(f32, want, f"{name} passes {passes}")
            if passes in (1, 5):
                want8 = np.full((SS.H, SS.W, 4), 255, np.uint8)
                want8[..., :3] = np.reshape([srgb8(v) for v in f32[..., :3].reshape(-1)], (SS.H, SS.W, 3))
                assert (u8 == want8).all()
    hit = c["guide"]["tri"] != D.MISS
    plain = D.atrous(D.mean_colour(c["acc"], c["frames"]), c["guide"], **DEFAULTS)
    assert (~bits_equal(want[hit], plain[hit])).mean() > 0.5   # the restatement itself differs from the plain filter


def crop(c, w, h, x0=0, y0=14):
    """A w x h window of a case: accumulation, hit records, attrs, guide and albedo."""
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    hits = c["hits"].reshape(SS.H, SS.W)[sl].reshape(-1).copy()
    attrs = c["attrs"].reshape(SS.H, SS.W)[sl].reshape(-1).copy()
    return (np.ascontiguousarray(c["acc"][sl]), hits, attrs, D.guide_from_hits(hits, w, h),
            attrs["albedo"].reshape(h, w, 3))


@pytest.mark.parametrize("frames", [1, 4])
def test_partial_tiles_frames_floor_and_nan(torch, frames):
    """A 37 x 19 window of the textured frame (no multiple of the 32 x 8 tile or the 64 x 4 direct block) that spans
    misses and the textured quad's edge; the same sum read as 1 and as 4 frames; one hit pixel's albedo set to exactly
    0 and another's to (0.05, 0.2, 0), so the floor is taken per channel; a NaN written into the accumulation at a hit
    pixel is repaired as in the plain filter."""
    from srt_amd.denoise import Denoiser

    w, h = 37, 19
    acc, hits, attrs, guide, albedo = crop(SS.case("textured"), w, h)
    hit = guide["tri"] != D.MISS
    assert hit[9, 20] and hit[10, 25] and hit[4, 30] and (~hit).sum() > 20
    attrs["albedo"][9 * w + 20] = 0.0
    attrs["albedo"][10 * w + 25] = (0.05, 0.2, 0.0)
    acc[4, 30, 1] = np.nan
    albedo = attrs["albedo"].reshape(h, w, 3)
    with Denoiser(w, h) as dn:
        for passes in (1, 5):
            dn.set_params(passes=passes)
            for floor in (0.1, 0.01):
                got = gpu_run_albedo(torch, dn, acc, frames, hits, attrs, floor)
                want = DA.run_albedo(acc, frames, guide, albedo, floor, **dict(DEFAULTS, passes=passes))
                check(got, want, f"frames {frames} passes {passes} floor {floor}")
                assert np.isfinite(want[9, 20]).all() and np.isfinite(want[10, 25]).all()
        # 5 passes: the NaN pixel has finite neighbours of its record, so it is repaired
        assert np.isfinite(want[4, 30]).all() and np.isfinite(got[4, 30, :3]).all()
    C0, a = DA.demodulate(acc, frames, guide, albedo, 0.01)
    assert bits_equal(a[9, 20], np.float32([0.01] * 3)).all() and bits_equal(a[10, 25], np.float32([0.05, 0.2, 0.01])).all()


def test_passes_zero_and_no_state_leak(torch):
    """passes == 0: attrs are ignored (None too) and both outputs equal run's, which test_gpu_denoise.py holds equal to
    image0.  After run_albedo calls on the object, run itself still equals the plain restatement."""
    from srt_amd import _lib
    from srt_amd.denoise import Denoiser

    c = SS.case("rubik")
    acc = torch.from_numpy(np.ascontiguousarray(c["acc"])).cuda()
    hd, ad = dev(torch, c["hits"], np.int32), dev(torch, c["attrs"], np.float32)
    with Denoiser(SS.W, SS.H) as dn:
        dn.set_params(passes=0)
        r32, r8 = dn.run(acc, c["frames"], None, srgb=True)
        for attrs in (ad, None):
            a32, a8 = dn.run_albedo(acc, c["frames"], None, attrs, srgb=True)
            dn.synchronize()
            assert dn.get_int("launches") == 1
            assert (a32.cpu().numpy().view(np.uint32) == r32.cpu().numpy().view(np.uint32)).all()
            assert (a8.cpu().numpy() == r8.cpu().numpy()).all()
        check(r32.cpu().numpy(), D.mean_colour(c["acc"], c["frames"]), "passes 0")
        dn.set_params(passes=5)
        # rejected calls on a live object leave it as it was
        import ctypes as C
        run = _lib.lib().srt_denoise_run_albedo
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        o = torch.empty((SS.H, SS.W, 4), dtype=torch.float32, device="cuda")
        bad = _lib.SRT_ERR_INVALID
        assert run(dn.handle, P(acc), c["frames"], P(hd), None, C.c_float(0.1), P(o), None) == bad        # no attrs, passes > 0
        assert run(dn.handle, P(acc), c["frames"], P(hd), C.c_void_p(ad.data_ptr() + 4), C.c_float(0.1), P(o), None) == bad
        assert run(dn.handle, P(acc), c["frames"], P(hd), P(ad), C.c_float(0.0), P(o), None) == bad
        assert run(dn.handle, P(acc), c["frames"], P(hd), P(ad), C.c_float(float("nan")), P(o), None) == bad
        assert run(dn.handle, P(acc), 0, P(hd), P(ad), C.c_float(0.1), P(o), None) == bad                 # run's own cases
        assert run(dn.handle, P(acc), c["frames"], None, P(ad), C.c_float(0.1), P(o), None) == bad
        assert run(dn.handle, P(acc), c["frames"], P(hd), P(ad), C.c_float(0.1), None, None) == bad
        assert dn.params == pytest.approx(DEFAULTS)
        got = gpu_run_albedo(torch, dn, c["acc"], c["frames"], c["hits"], c["attrs"])
        check(got, DA.run_albedo(c["acc"], c["frames"], c["guide"], c["albedo"], 0.1, **DEFAULTS), "run_albedo")
        plain = dn.run(acc, c["frames"], hd)
        dn.synchronize()
        check(plain.cpu().numpy(), D.atrous(D.mean_colour(c["acc"], c["frames"]), c["guide"], **DEFAULTS), "run after run_albedo")


def test_end_to_end_quality_on_the_textured_quad(torch):
    """Render 4 spp of the textured scene on the GPU, trace the guide and shade the attrs on the GPU, filter with the
    default parameters (5 passes) and the default floor: run_albedo equals the restatement on the read-back inputs,
    and over the textured quad's pixels its x / (1 + x) MSE against the oracle's 256-spp frame is lower than run's
    (on the CPU, tools/albedo_floor_grid.py: 0.000552 against 0.000856 at 5 passes)."""
    from srt_amd import render as R
    from srt_amd.denoise import ALBEDO_FLOOR, Denoiser
    from srt_amd.query import Query
    from srt_amd.surface import ATTR_DTYPE, Surface

    c = SS.case("textured")
    setup = c["setup"]
    rdr = R.Renderer(setup, device=0)
    try:
        rdr.render(SS.SPP)
        rdr.finish()
        frames = rdr.accum_frames
        acc = rdr.accum()
        acc_ptr, _ = rdr.compute.image_pointers()
        with Denoiser(SS.W, SS.H) as dn, Query(setup.scene) as q, Surface(setup.scene) as surf:
            assert dn.params == pytest.approx(DEFAULTS)
            rays = dn.primary_rays(setup.camera)
            hits = q.closest(rays)
            attrs = surf.shade(rays, hits)
            demod = dn.run_albedo(acc_ptr, frames, hits, attrs)
            plain = dn.run(acc_ptr, frames, hits)
            dn.synchronize()
            demod, plain = demod.cpu().numpy(), plain.cpu().numpy()
            attrs = attrs.cpu().numpy().view(ATTR_DTYPE).reshape(-1)
            hits = hits.numpy()
    finally:
        rdr.close()
    assert frames == c["frames"] and bits_equal(acc, c["acc"]).all()         # the GPU's frame is the oracle's
    assert (hits["triangle"] == c["hits"]["triangle"]).all()
    assert (attrs.view(np.uint32) == c["attrs"].view(np.uint32)).all()
    check(demod, DA.run_albedo(acc, frames, c["guide"], c["albedo"], ALBEDO_FLOOR, **DEFAULTS), "run_albedo")
    check(plain, D.atrous(D.mean_colour(acc, frames), c["guide"], **DEFAULTS), "run")
    quad = c["guide"]["tri"] < 2
    m_demod, m_plain = SS.mse_tm(demod[..., :3], c["ref"], quad), SS.mse_tm(plain[..., :3], c["ref"], quad)
    print(f"x/(1+x) MSE over {int(quad.sum())} pixels of the textured quad: run_albedo {m_demod:.6f}, run {m_plain:.6f}")
    assert m_demod < m_plain
