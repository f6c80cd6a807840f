"""Surface attributes and albedo-demodulated denoising (include/srt_surface.h), CPU only: the exported symbols, the
record layout, every SRT_ERR_INVALID path that is decided before a device is touched, the restated sampler against
srt_texture_sample, and the restatement's own sanity on the textured scene."""
import ctypes as C
import re

import numpy as np

import srt_amd as S
import surface_ref as SR
import surface_scenes as SS
from conftest import ROOT, bits_equal
from srt_amd import _lib

NAMES = ("srt_surface_abi_version", "srt_surface_create", "srt_surface_create_obj", "srt_surface_upload_textures",
         "srt_surface_update_model_matrix", "srt_surface_set_bvh_count", "srt_surface_destroy", "srt_surface_stream",
         "srt_surface_get_int", "srt_surface_shade", "srt_denoise_run_albedo")
INVALID = _lib.SRT_ERR_INVALID


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srt_surface.h").read_text(), flags=re.S)
    return re.findall(r"\b(srt_\w+)\s*\(", text)


def test_header_symbols_and_version():
    lib = _lib.lib()
    assert set(declared_functions()) == set(NAMES) == set(_lib.SURFACE_SYMBOLS)
    for other in (_lib.EXPORTED_SYMBOLS, _lib.QUERY_SYMBOLS, _lib.DENOISE_SYMBOLS, _lib.VARIANCE_SYMBOLS):
        assert not set(_lib.SURFACE_SYMBOLS) & set(other)
    assert lib.srt_surface_abi_version() == 1
    header = (ROOT / "include" / "srt_surface.h").read_text()
    assert "#define SRT_SURFACE_ABI_VERSION 1" in header
    # the other headers' versions are untouched
    assert lib.srt_abi_version() == 2 and lib.srt_query_abi_version() == 1 and lib.srt_denoise_abi_version() == 1
    assert lib.srt_variance_abi_version() == 1


def test_record_layout():
    from srt_amd.surface import ATTR_DTYPE

    A = _lib.SurfaceAttr
    assert C.sizeof(A) == 32 == ATTR_DTYPE.itemsize == SR.ATTR_DTYPE.itemsize
    want = {"albedo": 0, "bary_v": 12, "bary_w": 16, "uv": 20, "hit": 28}
    assert {n: getattr(A, n).offset for n in want} == want
    assert {n: ATTR_DTYPE.fields[n][1] for n in want} == want == {n: SR.ATTR_DTYPE.fields[n][1] for n in want}


def _create(scene, out, *, bvhs=True, n_bvhs=None, mats=True, tris=None, verts=True, tex=None):
    s = scene
    tris = s.tris if tris is None else tris
    P = S._ptr
    return _lib.lib().srt_surface_create(0, None, P(s.bvhs) if bvhs else None, len(s.bvhs) if n_bvhs is None else n_bvhs,
                                         P(s.mats) if mats else None, P(tex), len(s.mats), P(tris), len(tris),
                                         P(s.verts) if verts else None, len(s.verts), out)


def test_create_rejects_bad_scenes_on_the_host():
    """None of these reaches a device: this test runs where there is none."""
    scene = SS.textured_scene()
    h = C.c_void_p(0xDEAD)
    assert _create(scene, None) == INVALID                                 # no `out`
    for kw in (dict(bvhs=False), dict(mats=False), dict(verts=False), dict(n_bvhs=0)):
        h.value = 0xDEAD
        assert _create(scene, C.byref(h), **kw) == INVALID and not h.value  # *out is cleared
    for col, bad in ((0, 8), (1, 8), (2, 0xFFFFFFFF)):                      # each vertex index out of range
        tris = scene.tris.copy()
        tris["v"][3, col] = bad
        assert _create(scene, C.byref(h), tris=tris) == INVALID
        assert "vertex index" in _lib.last_error()
    tris = scene.tris.copy()
    tris["mat"][0] = 2                                                     # a material index out of range
    assert _create(scene, C.byref(h), tris=tris, tex=SS.TEX_ALBEDO) == INVALID
    assert "material index" in _lib.last_error()
    lib = _lib.lib()
    assert lib.srt_surface_create_obj(0, None, None, C.byref(h)) == INVALID
    # NULL objects
    assert lib.srt_surface_destroy(None) == INVALID and lib.srt_surface_set_bvh_count(None, 1) == INVALID
    assert lib.srt_surface_shade(None, None, None, 0, None) == INVALID
    assert lib.srt_surface_update_model_matrix(None, 0, None) == INVALID
    assert lib.srt_surface_get_int(None, b"textures", None) == INVALID and not lib.srt_surface_stream(None)


def test_upload_textures_validates_before_the_object():
    lib = _lib.lib()
    texel = np.zeros(4, np.uint8)
    for w, h, c, ptr in ((0, 1, 4, texel.ctypes.data), (1, -1, 4, texel.ctypes.data), (1, 1, 0, texel.ctypes.data),
                         (1, 1, 5, texel.ctypes.data), (1, 1, 4, None)):
        d = (_lib.Texture * 1)(_lib.Texture(ptr, w, h, c))
        assert lib.srt_surface_upload_textures(None, d, 1) == INVALID
        assert "texture 0" in _lib.last_error()
    assert lib.srt_surface_upload_textures(None, None, 1) == INVALID
    big = (_lib.Texture * 2)(_lib.Texture(texel.ctypes.data, 65536, 32768, 1), _lib.Texture(texel.ctypes.data, 65536, 32768, 1))
    assert lib.srt_surface_upload_textures(None, big, 2) == _lib.SRT_ERR_LIMIT
    good = (_lib.Texture * 1)(_lib.Texture(texel.ctypes.data, 1, 1, 4))
    assert lib.srt_surface_upload_textures(None, good, 1) == INVALID        # valid textures, no object


def test_run_albedo_rejects_bad_floors_before_the_object():
    run = _lib.lib().srt_denoise_run_albedo
    for floor in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert run(None, None, 1, None, None, C.c_float(floor), None, None) == INVALID
        assert "albedo_floor" in _lib.last_error()
    assert run(None, None, 1, None, None, C.c_float(0.1), None, None) == INVALID  # a NULL object


COORDS = np.asarray([-1.25, -0.5, -1e-9, 0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.999999, 1.0, 1.5, 7.5, 1e20, np.inf, -np.inf,
                     np.nan] + [(i + 0.5) / 5 for i in range(5)] + [(j + 0.5) / 3 for j in range(3)], np.float32)


def test_restated_sampler_equals_srt_texture_sample():
    """Texture 2 (5 x 3, distinct bytes) over the full grid of COORDS x COORDS, the 1 x 1 texture, the checker, and
    1- to 3-channel cuts of texture 2, bit for bit."""
    tex = SS.textures()
    s, t = (g.reshape(-1) for g in np.meshgrid(COORDS, COORDS, indexing="ij"))
    for texels in (tex[2], tex[1], tex[0], tex[2][..., :1], tex[2][..., :2], tex[2][..., :3]):
        got = SR.sample(texels, s, t)
        want = np.stack([S.texture_sample(texels, float(a), float(b)) for a, b in zip(s, t)])
        bad = ~bits_equal(got, want)
        print(f"{texels.shape}: {int(bad.sum())} of {bad.size} components differ")
        assert not bad.any()
    # exact texel centres return the texel itself
    c = SR.sample(tex[2], np.float32([0.5 / 5, 4.5 / 5]), np.float32([0.5 / 3, 2.5 / 3]))
    assert bits_equal(c, tex[2][[0, 2], [0, 4], :3].astype(np.float32) / np.float32(255)).all()


def test_fma32_is_the_single_rounding():
    from oracle.scene_ref import fma_f32

    rng = np.random.default_rng(5)
    a, b = rng.normal(size=400).astype(np.float32), rng.normal(size=400).astype(np.float32)
    c = (-(a.astype(np.float64) * b).astype(np.float32) * np.float32(1 + 2.0 ** -12)).astype(np.float32)  # cancellation
    c[::3] = rng.normal(size=len(c[::3])).astype(np.float32)
    # halfway cases of the float64 sum: a * b = 1 + 2^-24 exactly (a tie in float32), nudged by c
    a[:3], b[:3] = np.float32(1 + 2.0 ** -12), np.float32(1 - 2.0 ** -12 + 2.0 ** -23)
    c[:3] = np.float32([2.0 ** -60, -2.0 ** -60, 0.0])
    got = SR.fma32(a, b, c)
    want = np.asarray([fma_f32(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_restated_attributes_on_the_textured_scene():
    """Oracle hits of the pixel-centre rays: the barycentrics sum to 1 within the expression's own rounding, the uv
    of the textured quad spans (-0.5, 1.5) with GL_REPEAT at work, both checker colours show, the plain quad reads its
    diffuse colour, and misses are all-zero records."""
    setup = SS.textured_setup()
    rays = SS.pixel_rays(setup)
    hits = SS.oracle_hits(setup.scene, 1, rays)
    a = SS.scene_albedo(setup, rays, hits)
    hit = hits["triangle"] != SR.MISS
    assert 0.55 < hit.mean() < 0.75 and (a["hit"] == hit).all()
    assert (a[~hit].view(np.uint32) == 0).all()
    quad = hits["triangle"] < 2
    assert 0.40 < quad.mean() < 0.55                                         # about half of the frame
    v, w = a["bary_v"][hit], a["bary_w"][hit]
    u = np.float32(1) - v - w
    # u = (1 - v) - w: two roundings of values in [0, 1], so u + v + w is within 2 ulp(1) of 1, plus the sum's own
    assert np.abs((u.astype(np.float64) + v + w) - 1).max() <= 4 * 2.0 ** -24
    assert (v > -1e-4).all() and (w > -1e-4).all() and (u > -1e-4).all()
    uv = a["uv"][quad]
    assert uv.min() < -0.4 and uv.max() > 1.4 and (uv >= -0.5 - 1e-4).all() and (uv <= 1.5 + 1e-4).all()
    alb = a["albedo"][quad]
    c0, c1 = (c[:3].astype(np.float32) / np.float32(255) for c in SS.CHECKER)
    near = lambda c: (np.abs(alb - c).max(-1) < 1e-6).mean()  # noqa: E731
    # a cell is 2 texels wide and GL_LINEAR blends between texel centres: a sample is unblended over half of each
    # axis, a quarter of the area, an eighth per colour
    assert near(c0) > 0.08 and near(c1) > 0.08
    plain = hit & ~quad
    assert plain.sum() > 200 and bits_equal(a["albedo"][plain], np.broadcast_to(setup.scene.mats["diffuse"][1], (plain.sum(), 3))).all()
    # tex_albedo given: constant albedo over the textured quad, the same barycentrics and uv
    b = SR.shade(setup.scene, rays, hits, tex_albedo=SS.TEX_ALBEDO)
    assert bits_equal(b["albedo"][quad], np.broadcast_to(SS.TEX_ALBEDO[0], (quad.sum(), 3))).all()
    assert (b["uv"].view(np.uint32) == a["uv"].view(np.uint32)).all()
