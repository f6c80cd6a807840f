"""The numpy restatement of the guided upsampling (tests/upsample_ref.py), CPU only: the contract's axis tables, the
properties the contract implies, the gathered-array form against its per-pixel form, and the conditions the GPU test
places on its synthetic inputs (every path occurs)."""
import numpy as np
import pytest

import denoise_ref as D
import upsample_cases as UC
import upsample_ref as U
from conftest import bits_equal


def test_axis_tables():
    """f = 1: i0 = X and r = 0.  f = 2: quarters.  f = 3: the inexact thirds.  f = 4: eighths.  X = 0 reaches i0 = -1
    for every f > 1 (n = 1 - f is negative: floor division)."""
    i0, a0, a1 = U.axis_terms(6, 1)
    assert i0.tolist() == [0, 1, 2, 3, 4, 5] and (a1 == 0).all() and (a0 == 1).all()
    i0, a0, a1 = U.axis_terms(6, 2)
    assert i0.tolist() == [-1, 0, 0, 1, 1, 2]
    assert a1.tolist() == [0.75, 0.25, 0.75, 0.25, 0.75, 0.25] and a0.tolist() == [0.25, 0.75, 0.25, 0.75, 0.25, 0.75]
    i0, a0, a1 = U.axis_terms(7, 3)
    assert i0.tolist() == [-1, 0, 0, 0, 1, 1, 1]
    third, two = np.float32(2) / np.float32(6), np.float32(4) / np.float32(6)
    assert bits_equal(a1, np.asarray([two, 0, third, two, 0, third, two], np.float32)).all()
    assert bits_equal(a0, np.float32(1) - a1).all()
    assert set(a1.tolist()) == {0.0, float(third), float(two)}
    assert float(third) * 3 != 1.0 and a0[2] + a1[2] == np.float32(1)  # inexact, yet a0 + a1 rounds to 1
    i0, a0, a1 = U.axis_terms(9, 4)
    assert i0.tolist() == [-1, -1, 0, 0, 0, 0, 1, 1, 1]
    assert a1.tolist() == [0.625, 0.875, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375, 0.625]
    for f in (1, 2, 3, 4):
        i0, a0, a1 = U.axis_terms(40 * f, f)
        X = np.arange(40 * f)
        assert (i0 <= X // f).all() and (X // f <= i0 + 1).all()     # the nearest pixel is one of the bilinear taps
        centre = (i0 + 0.5) * f + a1.astype(np.float64) * f            # where the weights place X + 1/2
        assert np.allclose(centre, X + 0.5, atol=1e-5)
        assert i0.min() == (-1 if f > 1 else 0) and i0.max() == 39


def test_factor_one_is_the_guided_copy():
    """f = 1: the second tap of each axis has weight 0 and is skipped, so a pixel whose guides agree comes back as its
    own mean bit for bit (w * C / w), on the bilinear path."""
    c = UC.synthetic(5, 4, 1)
    out, path = U.upsample(c["accum"], c["frames"], c["low"], c["low"], 1)
    C = D.mean_colour(c["accum"], c["frames"])
    assert (path == U.BILINEAR).all()
    assert np.abs(out - C).max() <= np.spacing(C.max())


def _constant(c, f, low, full):
    w, h = low["tri"].shape[1], low["tri"].shape[0]
    accum = np.ones((h, w, 4), np.float32)
    accum[..., :3] = np.asarray([0.3, 1.7, 4.1], np.float32) * np.float32(c["frames"])
    out, path, detail = U.upsample(accum, c["frames"], low, full, f, detail=True)
    C = D.mean_colour(accum, c["frames"])[0, 0]
    return out, path, C, np.abs(out - C) / np.spacing(C), detail


@pytest.mark.parametrize("w,h,f", UC.CASES)
def test_constant_colour_comes_back(w, h, f):
    """A constant finite colour C comes back exactly on the nearest path, within 1 ulp where one tap is accepted and
    within 2n ulp where n taps are, as long as no accepted weight is so small that w * C is subnormal.

    The proof, with u = 2^-24 and every term positive (no cancellation): sum is n products, each within a factor
    (1 + u), added by n - 1 roundings, so it is C * (w_1 + ... + w_n) within (1 + u)^n; sw is the same weights added by
    n - 1 roundings, within (1 + u)^(n - 1); the division adds one more.  sum / sw is then C within (1 + u)^(2n), a
    relative error of 2n * u to first order, and an ulp of C is more than u * C (C is no power of two here): fewer
    than 2n ulp.  For n = 1 sw = w exactly and two roundings remain: 1 ulp.  A weight below 4 * FLT_MIN is left out of
    the bound, not out of the operation: 0.3 * w is then subnormal and keeps few bits (or none: it can round to 0),
    and with the random normals' max(dot, 0)^32 the error printed below reaches 1e7 ulp.  So the bound is asserted (a)
    over every pixel of the general synthetic guides whose accepted weights are all at least 4 * FLT_MIN, and (b) as
    1 ulp on guides that let exactly one tap decide a pixel (a BVH id of its own per low pixel, the full guide
    repeating the id of its nearest low pixel; normals the shared one or its opposite, so the weight is normal)."""
    c = UC.synthetic(w, h, f)
    out, path, C, ulps, detail = _constant(c, f, c["low"], c["full"])
    normal = (path != U.NEAREST) & (detail["min_weight"] >= 4 * np.finfo(np.float32).tiny)
    n = detail["taps"]
    print(f"{w}x{h} f={f} general guides: largest error {ulps.max()} ulp over all pixels, {ulps[normal].max(initial=0)} ulp "
          f"over the {int(normal.sum())} with normal weights (up to {int(n[normal].max(initial=0))} taps)")
    assert (n[path != U.NEAREST] >= 1).all() and (n[path == U.NEAREST] == 0).all()
    assert (ulps[normal] < 2 * n[normal][..., None]).all()
    assert (ulps[normal & (n == 1)] <= 1.0).all()
    assert normal.sum() > 0
    assert bits_equal(out[path == U.NEAREST], np.broadcast_to(C, out[path == U.NEAREST].shape)).all()
    # one tap: each low pixel's id is unique among its neighbours' (ids 0, 1 and miss cannot do that, so the guide
    # carries a BVH id per low pixel), and the full guide repeats the id of its nearest low pixel
    ids_low = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    n0 = c["low"]["normal"][1 % h, 0]                    # the shared normal (row 0 is random)

    def signed(n):
        return np.where((n @ n0 >= 0)[..., None], n0, -n0).astype(np.float32)

    low = D.make_guide(np.zeros((h, w), np.uint32), c["low"]["t"], signed(c["low"]["normal"]), ids_low)
    full = D.make_guide(np.zeros((f * h, f * w), np.uint32), c["full"]["t"], signed(c["full"]["normal"]), U.replicate(ids_low, f))
    out, path, C, ulps, detail = _constant(c, f, low, full)
    accepted = path != U.NEAREST
    assert (detail["taps"][accepted] == 1).all()
    print(f"{w}x{h} f={f} one tap a pixel: largest error {ulps.max()} ulp over {int(accepted.sum())} accepted pixels")
    assert accepted.sum() > 0 or w * h == 1
    assert (ulps[accepted] <= 1.0).all()
    assert bits_equal(out[~accepted], np.broadcast_to(C, out[~accepted].shape)).all()


def test_all_misses_over_all_hits_takes_the_nearest_path():
    w, h, f = 7, 5, 3
    c = UC.synthetic(w, h, f)
    low = D.make_guide(np.full((h, w), 4, np.uint32), c["low"]["t"], c["low"]["normal"], c["low"]["bvh"])
    full = D.make_guide(np.full((f * h, f * w), D.MISS, np.uint32), c["full"]["t"], c["full"]["normal"], c["full"]["bvh"])
    out, path = U.upsample(c["accum"], c["frames"], low, full, f)
    assert (path == U.NEAREST).all()
    assert bits_equal(out, U.replicate(D.mean_colour(c["accum"], c["frames"]), f)).all()


@pytest.mark.parametrize("w,h,f", UC.BIG)
@pytest.mark.parametrize("nonfinite", [False, True])
def test_synthetic_inputs_take_every_path(w, h, f, nonfinite):
    """A condition on the GPU test's inputs: bilinear, ring and nearest pixels all occur, among hit pixels and among
    miss pixels the bilinear path occurs, and the non-finite variant has a nearest pixel whose low pixel is NaN."""
    c = UC.synthetic(w, h, f, nonfinite=nonfinite)
    out, path = U.upsample(c["accum"], c["frames"], c["low"], c["full"], f)
    counts = {p: int((path == p).sum()) for p in (U.BILINEAR, U.RING, U.NEAREST)}
    print(f"{w}x{h} f={f} nonfinite={nonfinite}: bilinear {counts[0]}, ring {counts[1]}, nearest {counts[2]}")
    assert all(v > 0 for v in counts.values())
    hit = U.ids(c["full"]) != D.MISS
    assert (path[hit] == U.BILINEAR).sum() > 0 and (path[~hit] == U.BILINEAR).sum() > 0
    assert (path[hit] == U.RING).sum() > 0
    if nonfinite:
        assert path[2 * f, 2 * f] == U.NEAREST and np.isnan(out[2 * f, 2 * f, 0]) and out[2 * f, 2 * f, 1] == np.float32(1.0) / 3
        ok = path != U.NEAREST
        assert np.isfinite(out[ok]).all()    # a non-finite low pixel never enters an average


@pytest.mark.parametrize("w,h,f", [(1, 1, 2), (3, 1, 4), (11, 10, 2), (10, 10, 3), (5, 4, 1)])
def test_restatement_matches_its_per_pixel_form(w, h, f):
    c = UC.synthetic(w, h, f, nonfinite=w >= 10)
    for nsq, sd in ((5, 0.2), (0, 0.01)):
        a, pa = U.upsample(c["accum"], c["frames"], c["low"], c["full"], f, nsq, sd)
        b, pb = U.upsample_naive(c["accum"], c["frames"], c["low"], c["full"], f, nsq, sd)
        assert a.dtype == np.float32 and bits_equal(a, b).all() and (pa == pb).all()
