"""Tile culling (csrc/tile_cull.hpp): timed launches trace only the tiles that are not provably sky and
accumulate_kernel supplies the sky constant for the rest.  The image must not change by a bit: every case
compares the timed render with the counting render (which keeps every tile), with the render under
SRT_TILE_CULL=0 and with the CPU oracle."""
from __future__ import annotations

import numpy as np
import pytest

import srt_amd as S
from srt_amd import render as R
from conftest import OBJECTS, bits_equal, oracle_render

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 4
TILES = (W // 8) * (H // 8)


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


def _camera(setup, which):
    """The cameras of tests/cpp/test_tile_cull.cpp: 1 the model camera, 2 the box cut by the frame edge,
    4 inside the root box, 5 turned 120 degrees away (the frame's lines miss the box behind it as well)."""
    cam = setup.camera
    if which == 2:
        cam.position = cam.position + np.array((14.0, 0.0, 0.0), np.float32)
    elif which == 4:
        cam.position = np.array((0.0738, 9.18325, 0.0), np.float32)
    elif which == 5:
        cam.Rotate(120.0, 0.0)
    return setup


def _two_model_frame():
    frame = np.eye(4, dtype=np.float32)
    frame[3, :3] = (12.0, -2.0, -5.0)  # world -> model frame of the second cube (glm column 3)
    return frame


def _setup(rubik, case, depth):
    if case == "two_models":
        second = S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")
        setup = R.make_setup(W, H, show_model=True, models=[rubik, second], max_depth=depth, bvh_count=3)
        setup.scene.bvhs[1]["frame"] = _two_model_frame().reshape(16)
        return setup
    return _camera(R.make_setup(W, H, show_model=True, models=[rubik], max_depth=depth), case)


def _render(setup, case, *, count=False, spp=SPP):
    r = R.Renderer(setup)
    try:
        if case == "two_models":
            S.UpdateModelMatrix(r.compute, 1, _two_model_frame())
        r.render(spp, count=count)
        r.finish()
        return r.accum(), r.output(), r.compute.GetInt("launch.live_tiles"), r.compute.GetInt("launch.culled_samples")
    finally:
        r.close()


@pytest.mark.parametrize("depth", [0, 5])
@pytest.mark.parametrize("case", [1, 2, 4, 5, "two_models"])
def test_timed_render_is_bit_exact(rubik, monkeypatch, case, depth):
    setup = _setup(rubik, case, depth)
    acc, out, live, culled = _render(setup, case)
    acc_c, out_c, live_c, culled_c = _render(setup, case, count=True)
    monkeypatch.setenv("SRT_TILE_CULL", "0")
    acc_0, out_0, live_0, culled_0 = _render(setup, case)
    monkeypatch.delenv("SRT_TILE_CULL")
    want_acc, want_out, _ = oracle_render(setup, SPP)
    print(f"case {case} depth {depth}: live {live} of {TILES}, culled samples {culled}")
    for name, a, o in (("counting", acc_c, out_c), ("SRT_TILE_CULL=0", acc_0, out_0), ("oracle", want_acc, want_out)):
        assert bits_equal(acc, a).all(), f"accum differs from the {name} render's"
        assert (out == o).all(), f"out differs from the {name} render's"
    assert (live_c, culled_c) == (TILES, 0) and (live_0, culled_0) == (TILES, 0)
    assert culled == (TILES - live) * 64 * SPP
    if case == 1:
        assert 0 < live < TILES
    elif case == 4:
        assert live == TILES
    elif case == 5:
        assert live == 0 and (acc[..., 3] == 1.0).all() and (out[..., 3] == 255).all()  # every pixel written
        assert (acc[..., :3] == acc[0, 0, 0]).all() and acc[0, 0, 0] > 0.0


def test_partial_dispatch_extent(rubik):
    """A 40 x 32 extent of the 64 x 48 frame: tiles outside it hold no sample, pixels outside it keep their values."""
    setup = R.make_setup(W, H, show_model=True, models=[rubik])
    acc, _, _ = oracle_render(setup, 1)
    r = R.Renderer(setup)
    try:
        r.clear()
        r.compute.write_accum(np.full((H, W, 4), 7.0, np.float32))
        c = r.compute
        c.SetBool("resetAccumBuffer", True)
        c.SetInt("accumFrames", 1)
        c.Dispatch(5, 4)
        c.SetBool("resetAccumBuffer", False)
        c.SetInt("accumFrames", 2)
        c.Dispatch(5, 4)
        c.Finish()
        g = c.read_accum()
        live, culled = c.GetInt("launch.live_tiles"), c.GetInt("launch.culled_samples")
    finally:
        r.close()
    assert bits_equal(g[:32, :40], acc[:32, :40]).all()
    assert (g[32:, :] == 7.0).all() and (g[:, 40:] == 7.0).all()
    assert 0 < live < 20 and culled == (20 - live) * 64  # the 28 tiles outside the extent hold no sample


def test_two_ranks_on_one_device(rubik):
    """2-row bands dealt to two contexts of one device: an 8-row local tile spans 14 global rows, the
    classification only gets more conservative, and the group reassembles the one-GPU frame bit for bit."""
    setup = R.make_setup(W, H, show_model=True, models=[rubik])
    want_acc, want_out, _ = oracle_render(setup, SPP)
    g = R.GroupRenderer(setup, [0, 0], band_rows=2)
    try:
        g.render(SPP)
        g.finish()
        acc, out = g.accum(), g.output()
        lives = [p.compute.GetInt("launch.live_tiles") for p in g.parts]
    finally:
        g.close()
    assert bits_equal(acc, want_acc).all() and (out == want_out).all()
    assert all(0 < n < TILES // 2 for n in lives), lives


def test_global_scene_instance(rubik, monkeypatch):
    monkeypatch.setenv("SRT_FORCE_GLOBAL_SCENE", "1")
    setup = _setup(rubik, 2, 5)
    acc, out, live, culled = _render(setup, 2)
    acc_c, out_c, _, _ = _render(setup, 2, count=True)
    want_acc, want_out, _ = oracle_render(setup, SPP)
    assert bits_equal(acc, acc_c).all() and (out == out_c).all()
    assert bits_equal(acc, want_acc).all() and (out == want_out).all()
    assert 0 < live < TILES and culled == (TILES - live) * 64 * SPP


def test_moved_camera_uses_the_new_classification(rubik, monkeypatch):
    """Two renders of one context, the camera moved between them: the second equals a fresh context's.
    (SRT_TILE_CULL_MIN_SAMPLES=0: a launch this small would otherwise not be sent a second map.)"""
    monkeypatch.setenv("SRT_TILE_CULL_MIN_SAMPLES", "0")
    first = _setup(rubik, 1, 5)
    moved = _setup(rubik, 2, 5)
    fresh_acc, fresh_out, fresh_live, _ = _render(moved, 2)
    r = R.Renderer(first)
    try:
        r.render(SPP)
        r.finish()
        live_1 = r.compute.GetInt("launch.live_tiles")
        cam = moved.camera
        r.compute.SetVec3("cameraOrigin", cam.getOrigin())
        r.compute.SetVec3("cameraDirection", cam.getForward())
        r.compute.SetVec3("cameraUp", cam.getUpVector())
        r.compute.SetVec3("cameraRight", cam.getRightVector())
        r.render(SPP)
        r.finish()
        acc, out, live_2 = r.accum(), r.output(), r.compute.GetInt("launch.live_tiles")
    finally:
        r.close()
    assert bits_equal(acc, fresh_acc).all() and (out == fresh_out).all()
    assert live_2 == fresh_live and live_2 != live_1


def test_small_launch_after_a_move_keeps_every_tile_live(rubik):
    """By default a launch that culls fewer samples than a new map costs (SRT_TILE_CULL_MIN_SAMPLES, 2^24) is not
    sent one: after a camera move a 4-spp 64 x 48 render runs with every tile live, bit for bit the fresh
    context's frame; moved back, the map still on the device serves again."""
    first = _setup(rubik, 1, 5)
    moved = _setup(rubik, 2, 5)
    fresh_acc, fresh_out, _, _ = _render(moved, 2)
    base_acc, base_out, base_live, _ = _render(first, 1)
    r = R.Renderer(first)
    try:
        r.render(SPP)
        r.compute.SetVec3("cameraOrigin", moved.camera.getOrigin())
        r.render(SPP)
        r.finish()
        acc, out = r.accum(), r.output()
        live, culled, uploads = (r.compute.GetInt(n) for n in ("launch.live_tiles", "launch.culled_samples", "cull.uploads"))
        r.compute.SetVec3("cameraOrigin", first.camera.getOrigin())
        r.render(SPP)
        r.finish()
        acc_b, out_b, live_b = r.accum(), r.output(), r.compute.GetInt("launch.live_tiles")
        uploads_b = r.compute.GetInt("cull.uploads")
    finally:
        r.close()
    assert bits_equal(acc, fresh_acc).all() and (out == fresh_out).all()
    assert (live, culled, uploads) == (TILES, 0, 1)
    assert bits_equal(acc_b, base_acc).all() and (out_b == base_out).all()
    assert live_b == base_live and uploads_b == 1


def test_ring_reuse_is_bit_exact(rubik, monkeypatch):
    """Seven renders enqueued back to back, the camera moved before each and every map sent
    (SRT_TILE_CULL_MIN_SAMPLES=0): more maps than the ring of device copies holds, so entries are rewritten
    while earlier launches are still queued.  The last equals a fresh context's."""
    monkeypatch.setenv("SRT_TILE_CULL_MIN_SAMPLES", "0")
    shifts = [0.0, 14.0, 3.0, -14.0, 7.0, -6.0, 14.0]
    first = _setup(rubik, 1, 5)
    last = _setup(rubik, 2, 5)  # the model camera moved by 14: the last shift
    fresh_acc, fresh_out, fresh_live, _ = _render(last, 2)
    r = R.Renderer(first)
    try:
        base = first.camera.position
        for dx in shifts:
            r.compute.SetVec3("cameraOrigin", base + np.array((dx, 0.0, 0.0), np.float32))
            r.render(SPP)
        r.finish()
        acc, out, live = r.accum(), r.output(), r.compute.GetInt("launch.live_tiles")
        uploads = r.compute.GetInt("cull.uploads")
    finally:
        r.close()
    assert bits_equal(acc, fresh_acc).all() and (out == fresh_out).all()
    assert live == fresh_live and uploads >= 5
