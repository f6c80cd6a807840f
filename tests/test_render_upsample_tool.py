"""tools/render.py --upsample F: the argument handling on the CPU (every refusal comes from the parser, before a
device is touched), and on the GPU the tool's files, in child processes: that is what these tests are about."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from srt_amd.upsample import Upsampler  # noqa: F401  (the stage the flag drives)

TOOL = str(ROOT / "tools" / "render.py")


def run_tool(*args, cwd=None):
    return subprocess.run([sys.executable, TOOL, "--scene", "rubik", *args], capture_output=True, text=True, cwd=cwd, timeout=300)


@pytest.mark.parametrize("args,text", [
    (("--upsample", "3", "--width", "64", "--height", "48"), "multiples of 3"),
    (("--upsample", "2", "--width", "64", "--height", "47"), "multiples of 2"),
    (("--upsample", "4", "--width", "66", "--height", "48"), "multiples of 4"),
    (("--upsample", "5", "--width", "60", "--height", "40"), "F in 1..4"),
    (("--upsample", "-1", "--width", "60", "--height", "40"), "F in 1..4"),
    (("--upsample", "0", "--width", "60", "--height", "40"), "F in 1..4"),
    (("--upsample", "2", "--width", "64", "--height", "48", "--albedo"), "--albedo needs --denoise"),
    (("--upsample", "2", "--width", "64", "--height", "48", "--variance"), "--variance needs --orbit"),
    (("--upsample", "x"), "invalid int value"),
])
def test_refused_arguments(args, text):
    r = run_tool(*args)
    assert r.returncode == 2 and text in r.stderr, r.stderr


def test_sphere_scenes_are_refused():
    r = subprocess.run([sys.executable, TOOL, "--scene", "spheres", "--upsample", "2", "--width", "64", "--height", "48"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "mesh scene" in r.stderr


def test_help_names_the_flag():
    r = run_tool("--help")
    assert r.returncode == 0 and "--upsample F" in r.stdout and "_upsampled" in r.stdout


@pytest.mark.gpu
def test_plain_runs_are_unchanged_and_the_flag_writes_its_files(tmp_path):
    """Without the flag two runs write the same PNG bytes (and no upsampled file); with --upsample 2 --denoise the tool
    writes the 32 x 24 frame, its 64 x 48 upsampling and the filtered image."""
    import srt_amd as S  # noqa: F401  (the package is importable from the tree)

    common = ("--width", "64", "--height", "48", "--spp", "2")
    outs = []
    for name in ("a.png", "b.png"):
        r = run_tool(*common, "--out", str(tmp_path / name))
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append((tmp_path / name).read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) > 100
    assert not list(tmp_path.glob("*_upsampled*"))
    r = run_tool(*common, "--upsample", "2", "--denoise", "--out", str(tmp_path / "u.png"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "32x24 @ 8 spp" in r.stdout
    sizes = {}
    for name in ("u.png", "u_upsampled.png", "u_denoised.png"):
        data = (tmp_path / name).read_bytes()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        sizes[name] = (int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big"))
    assert sizes == {"u.png": (32, 24), "u_upsampled.png": (64, 48), "u_denoised.png": (64, 48)}
    assert np.frombuffer((tmp_path / "u_upsampled.png").read_bytes(), np.uint8).std() > 0


def png_sizes(tmp_path, names):
    sizes = {}
    for name in names:
        data = (tmp_path / name).read_bytes()
        assert data[:8] == b"\x89PNG\r\n\x1a\n", name
        assert np.frombuffer(data, np.uint8).std() > 0
        sizes[name] = (int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big"))
    return sizes


@pytest.mark.gpu
@pytest.mark.parametrize("flags,files", [
    (("--denoise", "--albedo"), ("_denoised", "_albedo_denoised")),
    (("--orbit", "2", "--variance"), ("_denoised", "_temporal", "_svgf")),
    (("--orbit", "2", "--spin", "3"), ("_denoised", "_temporal")),
    (("--orbit", "2", "--wave", "0.25", "--denoise", "--albedo"), ("_denoised", "_temporal")),
])
def test_the_other_stages_take_the_upsampled_frame(tmp_path, flags, files):
    """--upsample 2 with the filters, the albedo-demodulated filter, the temporal reprojection (moving camera, turning
    model, deforming mesh) and the variance-guided filter: the renderer's frame is 32 x 24, every stage's image 64 x 48."""
    r = run_tool("--width", "64", "--height", "48", "--spp", "1", "--upsample", "2", *flags, "--out", str(tmp_path / "u.png"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "32x24 @ 4 spp" in r.stdout and "upsampled to 64x48" in r.stdout
    want = {"u.png": (32, 24), "u_upsampled.png": (64, 48), **{f"u{s}.png": (64, 48) for s in files}}
    assert png_sizes(tmp_path, sorted(want)) == want
    assert sorted(p.name for p in tmp_path.glob("*.png")) == sorted(want)
