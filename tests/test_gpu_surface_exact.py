"""GPU: the two device samplers and the barycentrics above them at exact coordinates (tests/surface_exact.py).

surface.hpp's sample_bilinear receives chosen (s, t) bit patterns -- texel centres, seams and their float32
neighbours, the wrap seam from both sides, coordinates with no fraction left, NaNs -- through t = 0 hits on v0 of one
small triangle per pair, and is compared with the float32 restatement (tests/surface_ref.py) and the host sampler
bit for bit, and with the float64 GL sampler within the derived bound.  A second scene puts degenerate, sliver and
overflowing triangles under the barycentric division.  shading.hpp's texture_sample renders a quad whose uvs put
seams on its vertices, against the oracle.

NaNs are compared as words, like every other value: the restatement on the host and the kernel produce the same NaN
words in every case here but one, a frame scaled by 3e38, which this file adds to the frames asked for.  There
Inf - Inf and NaN + NaN meet, IEEE 754 leaves the sign and payload of the result open, and x86 and gfx950 differ
(conftest.bits_equal); that case alone asks for a NaN where the restatement has a NaN.
"""
import numpy as np
import pytest

import srt_amd as S
import surface_exact as X
import surface_ref as SR
from test_gpu_surface import gpu_attrs

pytestmark = pytest.mark.gpu

F = np.float32
TEXTURES = range(len(X.SHAPES))
FIELDS = ("albedo", "bary_v", "bary_w", "uv", "hit")
K8 = X.SHAPES.index((8, 8, 3))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, nan_words=True):
    """Every field, every dword, NaNs compared as words; with nan_words=False a NaN where `want` has a NaN will do."""
    ok = True
    for f in FIELDS:
        strict = words(got[f]) != words(want[f])
        bad = strict.copy()
        if f != "hit":
            bad &= ~(np.isnan(got[f]) & np.isnan(want[f]))
        print(f"{f}: {int(strict.sum())} of {strict.size} words differ ({int(bad.sum())} but for the words of NaNs)")
        ok &= not (strict if nan_words else bad).any()
    assert ok


@pytest.fixture(scope="module")
def device(torch):
    """One Surface.shade per texture over records(scene): the attrs of every coordinate, computed once."""
    from srt_amd.surface import Surface

    out = []
    for k in TEXTURES:
        c = X.case(k)
        with Surface(c["scene"]) as surf:
            assert surf.get_int("textures") == len(X.SHAPES)
            got = gpu_attrs(torch, surf, c["rays"], c["hits"])
            assert surf.get_int("launch.blocks") == (len(c["rays"]) + 255) // 256
        got.setflags(write=False)
        out.append(got)
    return out


@pytest.mark.parametrize("k", TEXTURES)
def test_every_coordinate_bit_exact(device, k):
    """Every field against the restatement; uv is the injected pair where it is finite, so the sampler did receive
    the chosen bits; the albedo is srt_texture_sample's at that pair, pair by pair."""
    c, got = X.case(k), device[k]
    coords = c["coords"]
    assert len(got) == len(coords) < 4096
    assert_same(got, c["want"])
    finite = np.isfinite(coords)
    assert (words(got["uv"])[finite] == words(coords)[finite]).all()
    assert np.isnan(got["uv"][~finite]).all() and (got["hit"] == 1).all()
    assert (words(got["bary_v"]) == 0).all() and (words(got["bary_w"]) == 0).all()
    host = np.stack([S.texture_sample(c["tex"], float(a), float(b)) for a, b in coords])
    bad = (words(got["albedo"]) != words(host)).any(1)
    print(f"{X.SHAPES[k]}: {int(bad.sum())} of {len(bad)} albedos differ from srt_texture_sample")
    assert not bad.any()


@pytest.mark.parametrize("k", TEXTURES)
def test_against_the_float64_sampler(device, k):
    """The device's albedo against the float64 sampler written from the GL definition, within surface_exact.bound."""
    c, got = X.case(k), device[k]
    w, h, _ = X.SHAPES[k]
    err = np.abs(got["albedo"].astype(np.float64) - X.sample64(c["tex"], c["coords"][:, 0], c["coords"][:, 1]))
    worst = np.unravel_index(np.argmax(err), err.shape)
    print(f"{X.SHAPES[k]}: largest error {err.max() / X.E24:.3f} * 2^-24 at {c['coords'][worst[0]]}, "
          f"bound {X.bound(w, h) / X.E24:.0f} * 2^-24")
    assert err.max() <= X.bound(w, h)


@pytest.mark.parametrize("shape", [(5, 3, 1), (3, 5, 2)])
def test_one_and_two_channel_textures_on_the_device(device, shape):
    """The host packs r | g << 8 | b << 16 words from 1 and 2 bytes a texel: the channels the file does not have
    are exactly 0 everywhere, and red varies."""
    k = X.SHAPES.index(shape)
    alb = device[k]["albedo"]
    assert_same(device[k], X.case(k)["want"])
    assert (words(alb[:, shape[2]:]) == 0).all()
    assert len(np.unique(alb[:, 0])) > 20 and (alb[:, :shape[2]] > 0).any(0).all()
    if shape[2] == 2:
        assert len(np.unique(alb[:, 1])) > 20 and (alb[:, 0] != alb[:, 1]).any()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_partial_blocks_of_specials(torch, n):
    """The first n records of a shuffled 8 x 8 case: NaN, huge and seam lanes beside ordinary ones in one wave."""
    from srt_amd.surface import Surface

    c = X.case(K8)
    order = np.random.default_rng(8).permutation(len(c["coords"]))[:n]
    coords = c["coords"][order]
    if n >= 63:
        tm = SR.sample_terms(c["tex"], coords[:, 0], coords[:, 1])
        first = slice(0, 63)                                     # all of these within the first wave
        assert (tm["nonfinite"][0] | tm["nonfinite"][1])[first].any()
        assert (np.isfinite(coords) & (np.abs(coords) >= 2.0 ** 24))[first].any()
        assert ((tm["a"][0] == F(0.5)) | (tm["a"][1] == F(0.5)))[first].any()
        assert np.isfinite(coords).all(1)[first].sum() > 20
    rays, hits = np.ascontiguousarray(c["rays"][order]), np.ascontiguousarray(c["hits"][order])
    with Surface(c["scene"]) as surf:
        got = gpu_attrs(torch, surf, rays, hits)
        assert surf.get_int("launch.blocks") == (n + 255) // 256
    assert_same(got, c["want"][order])
    assert_same(got, SR.shade(c["scene"], rays, hits, textures=c["scene"].textures))


def test_degenerate_and_sliver_triangles(torch):
    """Zero-area triangles (collinear, two coincident vertices, a point), slivers whose determinant underflows or
    cancels to 0, and edges of 1e19 and 2e19 whose dots overflow, each hit on v0 at t = 0 and at the mean of its
    vertices: denom = 1 / 0, NaN barycentrics and NaN uvs, which the sampler reads as 0."""
    from srt_amd.surface import Surface

    sc, rays, hits = X.degenerate_scene(X.textures(), K8)
    terms = {}
    want = SR.shade(sc, rays, hits, textures=sc.textures, terms=terms)
    assert np.isposinf(terms["denom"]).any() and np.isnan(terms["v"]).any()
    finite = np.isfinite(want["uv"]).all(1) & np.isfinite(want["bary_v"]) & np.isfinite(want["bary_w"])
    assert finite.any() and (~finite).sum() >= 8
    with Surface(sc) as surf:
        got = gpu_attrs(torch, surf, rays, hits)
    assert_same(got, want)
    assert (got["hit"] == 1).all()
    assert (np.isnan(got["uv"]) == np.isnan(want["uv"])).all() and not np.isinf(want["uv"]).any()
    tex = sc.textures[K8]
    uv = np.where(np.isfinite(got["uv"]), got["uv"], F(0))      # a non-finite coordinate samples at 0
    at0 = np.stack([S.texture_sample(tex, float(a), float(b)) for a, b in uv])
    assert (words(got["albedo"]) == words(at0)).all()
    both = ~np.isfinite(got["uv"]).any(1)
    assert both.any() and (words(got["albedo"][both]) == words(S.texture_sample(tex, 0.0, 0.0))).all()


def test_frames_that_overflow(torch):
    """The 8 x 8 case under frames scaled by 1e30, by 3e38 and by 0: mp is huge, Inf or NaN, or 0, and so are the
    barycentrics and the uv that reach the sampler.  (3e38 is this file's addition: see the module's note on NaNs.)"""
    from srt_amd.surface import Surface

    c = X.case(K8)
    sc = c["scene"]
    seen = {}
    with Surface(sc) as surf:
        for scale in (1e30, 3e38, 0.0):
            frame = (np.eye(4, dtype=np.float32) * F(scale)).reshape(16)
            surf.update_model_matrix(0, frame)
            got = gpu_attrs(torch, surf, c["rays"], c["hits"])
            terms = {}
            want = SR.shade(sc, c["rays"], c["hits"], textures=sc.textures, frames=frame[None], terms=terms)
            print(f"frame scaled by {scale}:")
            assert_same(got, want, nan_words=scale != 3e38)
            assert (got["hit"] == 1).all() and np.isfinite(got["albedo"]).all()
            seen[scale] = terms["mp"]
    assert np.isfinite(seen[1e30]).all() and (np.abs(seen[1e30][:, :2]) >= 1e30).all()
    assert np.isinf(seen[3e38]).any() and (seen[0.0] == 0).all()


@pytest.mark.parametrize("k", range(len(X.SEAM_UVS)))
def test_path_tracer_samples_the_same_seams(k):
    """shading.hpp's texture_sample against the oracle: the textured quad with the 8 x 8 random texture and uvs that
    put seams on its vertices, the wrap seam 2^-24 below them, or no fraction at all, at 32 x 24, 2 spp, depth 2,
    through the counting and the timed instance, bit for bit over the whole frame."""
    from conftest import bits_equal
    from test_gpu_parity import gpu_render

    setup = X.seam_setup(k)
    acc, out, st = X.seam_oracle(k)
    for other in range(len(X.SEAM_UVS)):                         # from the oracle alone: the three frames differ
        if other != k:
            assert not bits_equal(acc, X.seam_oracle(other)[0]).all()
    gacc, gout, gst = gpu_render(setup, X.SEAM_SPP)
    eq = bits_equal(gacc, acc)
    assert eq.all(), f"{(~eq).sum()} accumulation values differ"
    assert (gout == out).all()
    assert gst["rays"] == st["rays"] and gst["samples"] == st["samples"] and gst["shadow_rays"] == st["shadow_rays"]
