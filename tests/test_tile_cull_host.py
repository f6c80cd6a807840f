"""The sky / live tile classifier (csrc/tile_cull.cpp) on the CPU: tests/cpp/test_tile_cull.cpp as a stand-alone
program under AddressSanitizer + UBSan (host code only: no HIP, no device, nothing preloaded)."""
from __future__ import annotations

import subprocess

from conftest import OBJECTS, PKG, ROOT


def test_tile_cull_under_sanitizers():
    """Exhaustive soundness (no sample of a `sky` tile passes a root box test, restated in fp32), usefulness (at
    least 80% of the tiles that miss everywhere are `sky`), and the cases that must stay live."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_tile_cull_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    str(ROOT / "tests" / "cpp" / "test_tile_cull.cpp"),
                    *[str(PKG / "csrc" / s) for s in ("tile_cull.cpp", "scene.cpp", "noise.cpp", "camera.cpp")],
                    "-o", str(exe), "-lz", "-pthread"], check=True)
    r = subprocess.run([str(exe), str(OBJECTS / "Rubik" / "Rubik.obj")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tile cull checks OK" in r.stdout
