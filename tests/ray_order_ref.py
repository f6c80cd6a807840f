"""A numpy restatement, in float32, of the ordering rule of include/srt_query_sort.h (csrc/ray_order_rule.hpp), for
tests/test_ray_order_api.py: the bounds of the finite origins, the key of every ray, the stable order.  Written from the
header's text and independent of the library; the two bit counts are arguments.
"""
import numpy as np

F = np.float32
U = np.uint32
FLT_MAX = np.finfo(np.float32).max


def _ordered(x):
    """The order-preserving word of a float32: a < b (with -0 < +0) iff ordered(a) < ordered(b)."""
    u = np.asarray(x, F).view(U)
    return np.where(u & U(0x80000000), ~u, u | U(0x80000000)).astype(U)


def bounds(rays):
    """lo xyz, hi xyz over the finite origins, in the total order of the words; zeros on an axis without one."""
    out = np.zeros(6, F)
    o = rays["o"].astype(F).reshape(-1, 3)
    for k in range(3):
        x = o[:, k]
        with np.errstate(invalid="ignore"):
            x = x[np.abs(x) <= FLT_MAX]
        if len(x):
            w = _ordered(x)
            out[k], out[3 + k] = x[np.argmin(w)], x[np.argmax(w)]
    return out


def _quantize(u, bits):
    """0 unless u > 0, 2^bits - 1 from there up, else u truncated; NaN gives 0."""
    top = (1 << bits) - 1
    with np.errstate(invalid="ignore"):
        pos, high = u > F(0), u >= F(top)
        inner = pos & ~high
        cell = np.zeros(u.shape, U)
        cell[high & pos] = top
        cell[inner] = u[inner].astype(U)
    return cell


def _spread3(x):
    x = x.astype(np.uint64)
    out = np.zeros(x.shape, np.uint64)
    for b in range(10):
        out |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def _morton(c):
    return (_spread3(c[:, 0]) << np.uint64(2)) | (_spread3(c[:, 1]) << np.uint64(1)) | _spread3(c[:, 2])


def keys(rays, origin_bits, dir_bits, box=None):
    box = bounds(rays) if box is None else box
    n = len(rays)
    o, d = rays["o"].astype(F).reshape(n, 3), rays["d"].astype(F).reshape(n, 3)
    oc, dc = np.zeros((n, 3), U), np.zeros((n, 3), U)
    with np.errstate(all="ignore"):
        for k in range(3):
            lo, hi = box[k], box[3 + k]
            ext = F(hi - lo)
            if ext > 0:
                r = ((o[:, k] - lo) / ext).astype(F)
                u = (r * F(2.0 ** origin_bits)).astype(F)
            else:
                u = np.zeros(n, F)
            oc[:, k] = _quantize(u, origin_bits)
        a = np.abs(d)
        m = a[:, 0].copy()
        m = np.where(a[:, 1] > m, a[:, 1], m)
        m = np.where(a[:, 2] > m, a[:, 2], m)
        ok = (m > 0) & (m <= FLT_MAX)
        for k in range(3):
            r = (d[:, k] / m).astype(F)
            u = ((r + F(1.0)).astype(F) * F(2.0 ** (dir_bits - 1))).astype(F)
            dc[:, k] = _quantize(np.where(ok, u, F(0.0)).astype(F), dir_bits)
    key = (_morton(oc) << np.uint64(3 * dir_bits)) | _morton(dc)
    assert (key < (1 << 3 * (origin_bits + dir_bits))).all()
    return key.astype(U)


def order(key):
    return np.argsort(key, kind="stable").astype(U)


def ray_order(rays, origin_bits, dir_bits):
    """(order, sorted keys, bounds), as srt_ray_order returns them."""
    box = bounds(rays)
    k = keys(rays, origin_bits, dir_bits, box)
    p = order(k)
    return p, k[p], box
