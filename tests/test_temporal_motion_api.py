"""The moving-model extension of the temporal reprojection (include/srt_temporal_motion.h), CPU only: exported
symbols, version and struct size, argument checks that return before any device is touched, the affine inverse
against numpy's, the C++ mirror, the pose bookkeeping under ASan/UBSan as a stand-alone program, and properties of
the numpy restatement alone (tests/temporal_motion_ref.py): its per-pixel form, equal poses, a rigid move of
everything, and a square that is followed across the image where the static history ghosts."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import temporal_motion_ref as M
import temporal_ref as T
from conftest import PKG, ROOT, bits_equal

NAMES = ("srt_temporal_motion_abi_version", "srt_temporal_set_models", "srt_temporal_model_from_frame")


def declared_functions():
    text = (ROOT / "include" / "srt_temporal_motion.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_temporal_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_motion_symbol():
    assert declared_functions() == sorted(NAMES)
    for so in ("libsrt_amd.so", "libsrt_amd_F.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / so)], capture_output=True, text=True,
                             check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [n for n in NAMES if n not in exported], so


def test_python_binding_version_and_size():
    from srt_amd import _lib

    assert set(_lib.TEMPORAL_MOTION_SYMBOLS) == set(NAMES)
    assert not set(_lib.TEMPORAL_MOTION_SYMBOLS) & set(_lib.TEMPORAL_SYMBOLS)
    lib = _lib.lib()
    assert lib.srt_temporal_motion_abi_version() == 1
    assert lib.srt_temporal_abi_version() == 1  # the older header's version stays
    assert C.sizeof(_lib.TemporalModel) == 128
    header = (ROOT / "include" / "srt_temporal_motion.h").read_text()
    assert re.search(r"#define\s+SRT_TEMPORAL_MOTION_ABI_VERSION\s+1\b", header)
    assert '#include "srt_temporal.h"' in header
    low = header.lower()
    assert "light" in low and "shading" in low and "bitwise" in low  # what is not modelled; the static rule
    assert "srt_temporal_motion.h" in (ROOT / "include" / "srt_temporal.h").read_text()
    from srt_amd.temporal import Temporal

    assert callable(Temporal.set_models)


def models(n):
    from srt_amd import _lib

    arr = (_lib.TemporalModel * n)()
    for m in arr:
        m.world_to_model[:] = M.IDENTITY.tolist()
        m.model_to_world[:] = M.IDENTITY.tolist()
    return arr


def test_null_range_and_validation_without_a_device():
    """srt_temporal_set_models checks the array before it looks at the object, so each of these returns before a
    device call (with none here, one that reached a device would give SRT_ERR_HIP): the message tells which check
    answered."""
    from srt_amd import _lib

    lib = _lib.lib()
    inv, lim = _lib.SRT_ERR_INVALID, _lib.SRT_ERR_LIMIT
    good = models(3)
    assert lib.srt_temporal_set_models(None, good, 3) == inv and "NULL object" in _lib.last_error()
    assert lib.srt_temporal_set_models(None, None, 0) == inv and "NULL object" in _lib.last_error()
    assert lib.srt_temporal_set_models(None, None, 2) == inv and "finite" in _lib.last_error()
    for field in ("world_to_model", "model_to_world"):
        for k, bad in ((0, float("nan")), (13, float("inf")), (6, float("-inf")),       # a non-finite entry
                       (3, 1e-30), (7, -1.0), (11, 0.5), (15, 0.99999994), (15, 0.0)):  # the bottom row
            arr = models(3)
            getattr(arr[2], field)[k] = bad
            assert lib.srt_temporal_set_models(None, arr, 3) == inv and "finite" in _lib.last_error(), (field, k)
            assert lib.srt_temporal_set_models(None, arr, 2) == inv and "NULL object" in _lib.last_error()
    for n in (65536, 1 << 20, 0xFFFFFFFF):  # the cap, checked before the array is read
        assert lib.srt_temporal_set_models(None, good, n) == lim and "65535" in _lib.last_error()
    m = _lib.TemporalModel()
    assert lib.srt_temporal_model_from_frame(None, C.byref(m)) == inv
    assert lib.srt_temporal_model_from_frame(M.IDENTITY.ctypes.data_as(C.c_void_p), None) == inv


FRAMES = {
    "rotation": M.column_major(M.rotation("y", 33.0) @ M.rotation("x", -71.0) @ M.rotation("z", 12.5)),
    "scale": M.column_major(np.diag([1.7, 0.6, 1.2])),
    "translation": M.column_major(translation=(0.9, -1.4, 0.7)),
    "all": M.column_major(M.rotation("y", 33.0) @ np.diag([1.7, 0.6, 1.2]), (0.9, -1.4, 0.7)),
}


@pytest.mark.parametrize("what", sorted(FRAMES))
def test_model_from_frame_against_numpy(what):
    """The inverse agrees with numpy's float64 inverse rounded to float32 within an ulp of its entries (order 1:
    1.2e-7), and |M * M^-1 - I| <= 1e-6 on the float results: two float32 roundings of entries of order 1."""
    from srt_amd import _lib

    frame = FRAMES[what]
    m = _lib.TemporalModel()
    assert _lib.lib().srt_temporal_model_from_frame(frame.ctypes.data_as(C.c_void_p), C.byref(m)) == _lib.SRT_OK
    w2m, m2w = np.asarray(m.world_to_model[:], np.float32), np.asarray(m.model_to_world[:], np.float32)
    assert bits_equal(w2m, frame).all()
    assert m2w[3] == 0 and m2w[7] == 0 and m2w[11] == 0 and m2w[15] == 1
    want = M.pose_from_frame(frame)[1]
    prod = w2m.astype(np.float64).reshape(4, 4) @ m2w.astype(np.float64).reshape(4, 4)
    print(what, "max |inverse - numpy's|", np.abs(m2w - want).max(), "max |M M^-1 - I|", np.abs(prod - np.eye(4)).max())
    assert np.abs(m2w.astype(np.float64) - want).max() <= 2.0 ** -22
    assert np.abs(prod - np.eye(4)).max() <= 1e-6


def test_model_from_frame_rejects():
    from srt_amd import _lib

    fn, m = _lib.lib().srt_temporal_model_from_frame, _lib.TemporalModel()
    flat = M.column_major(np.diag([1.0, 0.0, 1.0]))                       # singular: one axis collapsed
    plane = M.column_major(np.array([[1, 2, 3], [2, 4, 6], [0, 1, 0.0]]))  # singular: dependent rows
    bottom = M.IDENTITY.copy()
    bottom[7] = 0.25
    nan = M.IDENTITY.copy()
    nan[9] = np.nan
    for bad in (flat, plane, bottom, nan):
        assert fn(bad.ctypes.data_as(C.c_void_p), C.byref(m)) == _lib.SRT_ERR_INVALID
    assert "singular" in _lib.last_error()


def test_cpp_mirror_compiles():
    """include/srt/temporal.hpp with SetModels compiles on its own against the C headers (syntax only)."""
    src = ('#include "srt/temporal.hpp"\n'
           "int use(srt::Temporal& t, const float* frame) {\n"
           "  srt_temporal_model m = srt::Temporal::ModelFromFrame(frame); t.SetModels(&m, 1); t.SetModels(nullptr, 0);\n"
           '  return t.get_int("models.bytes") + SRT_TEMPORAL_MOTION_ABI_VERSION + (int)sizeof(srt_temporal_model); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), "-x", "c++", "-"],
                   input=src, text=True, check=True)


def test_pose_bookkeeping_under_sanitizers():
    """tests/cpp/test_temporal_motion_host.cpp with csrc/temporal_host.cpp linked directly, AddressSanitizer + UBSan,
    as a stand-alone program (host code only: no HIP, no device, nothing preloaded): validation, the inverse, the
    product's element order, the first-pose and bitwise-equality rules, reset, and the upload chunks."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_temporal_motion_host_san"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_temporal_motion_host.cpp"), str(PKG / "csrc" / "temporal_host.cpp"),
                    "-o", str(exe), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "temporal motion host checks OK" in r.stdout


# ---------------------------------------------------------------------------------------------------------------
# the restatement alone
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(5, 1), (37, 23)])
def test_restatement_matches_its_per_pixel_form(w, h):
    """The vectorised restatement equals the scalar per-pixel loop bit for bit over the five frames of the moving
    two-wall scene, and at 37x23 the square's motion is in fact applied (frames 2-4 differ from a run without poses)."""
    a, b, plain = M.TemporalMotionRef(w, h), M.TemporalMotionRef(w, h), T.TemporalRef(w, h)
    differs = []
    for k, (cam, accum, fields, poses) in enumerate(M.moving_two_wall_frames(w, h)):
        a.set_models(poses)
        b.set_models(poses)
        g = D.make_guide(*fields)
        x, y = a.accumulate(accum, 3, g, cam), b.accumulate(accum, 3, g, cam, naive=True)
        assert x.dtype == np.float32 and bits_equal(x, y).all(), k
        differs.append(not bits_equal(x, plain.accumulate(accum, 3, g, cam)).all())
    if w >= 37:
        assert differs == [False, False, True, True, True]


def test_equal_poses_reproduce_the_static_restatement():
    """(a) Poses that never change, identity or not, give temporal_ref's result bit for bit on every frame."""
    w, h = 37, 23
    tilted = M.pose_from_model(M.column_major(M.rotation("z", 10.0) @ np.diag([1.1, 0.9, 1.0]), (.2, .05, .1)))
    still = M.pose_from_model(M.IDENTITY)
    for poses in ([still, still], [still, tilted]):
        a, plain = M.TemporalMotionRef(w, h), T.TemporalRef(w, h)
        a.set_models(poses)
        rng = np.random.default_rng(5)
        for k, (pos, yaw, pitch) in enumerate(M.CAMERAS):
            cam = T.camera_vectors(pos, yaw, pitch)
            g = D.make_guide(*M.posed_two_wall_guide(cam, w, h, [p[0] for p in poses])[:4])
            accum = np.ones((h, w, 4), np.float32)
            accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
            a.set_models(poses)  # setting the same poses again changes nothing
            assert not a.motion()[0].any()
            x = a.accumulate(accum, 3, g, cam)
            assert bits_equal(x, plain.accumulate(accum, 3, g, cam)).all(), k
        assert (x[..., 3] >= 2).mean() > 0.3


def test_rigid_move_of_everything_keeps_every_interior_pixel():
    """(b) Both records and the camera move by one rigid transform between two frames: every interior hit pixel
    (its 3 x 3 neighbourhood the same record) keeps its history, N == 2.  Without poses the same move loses it."""
    w, h = 37, 23
    R = M.rotation("y", 20.0) @ M.rotation("x", 10.0)
    shift = np.array([0.5, -0.2, 0.3])
    cam0 = T.camera_vectors(*M.CAMERAS[0])
    cam1 = ((R @ cam0[0].astype(np.float64) + shift).astype(np.float32),) + tuple((R @ v.astype(np.float64)).astype(np.float32)
                                                                                 for v in cam0[1:])
    still, moved = M.pose_from_model(M.IDENTITY), M.pose_from_model(M.column_major(R, shift))
    f0 = M.posed_two_wall_guide(cam0, w, h)[:4]
    f1 = M.posed_two_wall_guide(cam1, w, h, [moved[0], moved[0]])[:4]
    rng = np.random.default_rng(9)
    acc = [np.concatenate([rng.uniform(0, 6, (h, w, 3)), np.ones((h, w, 1))], -1).astype(np.float32) for _ in range(2)]
    a, plain = M.TemporalMotionRef(w, h), T.TemporalRef(w, h)
    a.set_models([still, still])
    a.accumulate(acc[0], 1, D.make_guide(*f0), cam0)
    plain.accumulate(acc[0], 1, D.make_guide(*f0), cam0)
    a.set_models([moved, moved])
    n = a.accumulate(acc[1], 1, D.make_guide(*f1), cam1)[..., 3]
    n_plain = plain.accumulate(acc[1], 1, D.make_guide(*f1), cam1)[..., 3]
    hit = f1[0] != T.MISS
    inner = M.interior(hit & (f1[3] == 0)) | M.interior(hit & (f1[3] == 1))
    print(f"{int(inner.sum())} interior hit pixels of {int(hit.sum())}; with poses {int((n[inner] == 2).sum())} keep N == 2, "
          f"without {int((n_plain[inner] == 2).sum())}")
    assert inner.sum() > 100 and (f1[3][inner] == 1).sum() > 20  # not vacuous: both records have interior pixels
    assert (n[inner] == 2).all()
    assert (n_plain[inner] == 2).mean() < 0.5


def test_history_follows_the_square():
    """(c) 64x24, the camera still at (0, 0, 4) looking down -z, the square (depth 3, so a pixel is 3/64 wide on it)
    translated along world x by k = 3 pixel widths, 9/64 exactly.  Frame 0's colours are a ramp in the square's model
    x, 1 + 2x (a step of 2 * 3/64 = 0.09375 per pixel); frame 1's sample is 0, so its output is exactly half the
    history it found.  With poses a pixel inside the square carries the previous colour of the pixel k to its left
    within 1e-4 (N == 2); without poses it differs from that colour by at least half the ramp's step over k pixels,
    0.140625: the ghost.  Observed: with poses at most 2.4e-07 off; without, at least 0.28125 off."""
    w, h, k = 64, 24, 3
    cam = T.camera_vectors((0, 0, 4), -90, 0)
    delta = np.float32(k) * np.float32(3) / np.float32(w)
    assert float(delta) == 9 / 64
    still, moved = M.pose_from_model(M.IDENTITY), M.pose_from_model(M.column_major(translation=(delta, 0, 0)))
    f0 = M.posed_two_wall_guide(cam, w, h)
    f1 = M.posed_two_wall_guide(cam, w, h, [still[0], moved[0]])
    sq0, sq1 = f0[3] == 1, f1[3] == 1
    assert (sq1[:, k:] == sq0[:, :-k]).all() and sq0.sum() > 80  # the square moved k pixels to the right
    acc0 = np.ones((h, w, 4), np.float32)
    acc0[..., :3] = np.where(sq0[..., None], (1 + 2 * f0[4][..., 0])[..., None] * np.array([1.0, 0.5, 0.25]), 5.0)
    acc1 = np.zeros((h, w, 4), np.float32)
    acc1[..., 3] = 1
    a, plain = M.TemporalMotionRef(w, h), T.TemporalRef(w, h)
    outs = []
    for ref in (a, plain):
        if ref is a:
            ref.set_models([still, still])
        prev = ref.accumulate(acc0, 1, D.make_guide(*f0[:4]), cam)
        if ref is a:
            ref.set_models([still, moved])
        outs.append(ref.accumulate(acc1, 1, D.make_guide(*f1[:4]), cam))
    inner = M.interior(sq1)
    assert inner.sum() > 40
    carried = np.roll(prev[..., 0], k, axis=1)  # the previous colour of the pixel k to the left
    step = 2 * 3 / 64
    with_poses, without = np.abs(2 * outs[0][..., 0] - carried)[inner], np.abs(2 * outs[1][..., 0] - carried)[inner]
    print(f"{int(inner.sum())} interior pixels: with poses at most {with_poses.max():.3g} off the colour {k} pixels to the "
          f"left; without poses at least {without.min():.6g} off (bounds 1e-4 and {0.5 * k * step})")
    assert (outs[0][..., 3][inner] == 2).all()
    assert with_poses.max() <= 1e-4
    assert without.min() >= 0.5 * k * step
    # the wall behind did not move: with or without poses its interior pixels keep their own history
    wall = M.interior((f1[3] == 0) & (f1[0] != T.MISS)) & M.interior((f0[3] == 0) & (f0[0] != T.MISS))
    assert wall.sum() > 100 and bits_equal(outs[0][wall], outs[1][wall]).all() and (outs[0][..., 3][wall] == 2).all()
