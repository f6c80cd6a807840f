"""GPU: the device refit of the path tracer's own scene (include/srt_scene_refit.h, Compute.bind_scene(scene,
refit=True) and Compute.refit) against the host path -- srt_bvh_refit, then a fresh upload -- in every dword of the
device arrays, in the rendered image and against the CPU oracle.

Context A binds with refit=True and refits on the device; context B binds refit_scene(scene, verts'), whose nodes the
host refit made (tests/test_refit_api.py holds that one to a numpy restatement).  Compute.scene_device() returns the
device arrays nodes / nodes_t / tris as uint32 [n, 4] (srt_scene_copy_device).
"""
import dataclasses

import numpy as np
import pytest

import refit_ref as RR
import srt_amd as S
import surface_scenes as SS
from conftest import bits_equal
from oracle import pyoracle as O
from srt_amd import render as R
from test_gpu_queries import MISS, rubik_rays
from test_gpu_refit import rubik, rubik_scene, small_scene, torch, verts_dev  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

SCENES = ["rubik", "grid", "one", "five", "two_models"]
# layout variants, set before the context is created (ChooseScenePolicy and srt_create read the environment)
VARIANTS = {
    "default": {},  # LDS mode at these sizes: dense triangles, no top region
    "global": {"SRT_FORCE_GLOBAL_SCENE": "1", "SRT_TRI_ALIGN": "1", "SRT_TOP_DEPTH": "3"},  # slot gaps, a top region
    "node_align": {"SRT_NODE_ALIGN": "1"},  # padding slots between chains
    "identity": {"SRT_NODE_LAYOUT": "0"},   # the input order, ref_or = 0
    "treelets": {"SRT_TREELETS": "1", "SRT_TREELET_DEPTH": "3", "SRT_FORCE_GLOBAL_SCENE": "1"},  # a treelet copy
}


def set_env(monkeypatch, variant):
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)


def expected_tri_slots(scene):
    """csrc/scene_layout.cpp LayoutTris restated: a one-triangle leaf avoids slots 2 and 5 mod 8, a two-triangle
    leaf starts at 0, 3 or 6 mod 8."""
    lead = np.zeros(len(scene.tris), np.int64)
    reach = RR.reached(scene)
    for i, n in enumerate(scene.nodes):
        if n["count"] > 0 and reach[i]:
            lead[n["first"]] = n["count"]
    s = 0
    for t in range(len(scene.tris)):
        if lead[t] == 1:
            while s & 7 in (2, 5):
                s += 1
        elif lead[t] == 2:
            while (s & 7) % 3:
                s += 1
        s += 1
    return s


def assert_arrays_equal(got, want):
    for g, w, what in zip(got, want, ("nodes", "nodes_t", "tris")):
        assert (g is None) == (w is None), what
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype == np.uint32, what
        assert (g == w).all(), f"{what}: {(g != w).sum()} dwords differ"


@pytest.mark.parametrize("name,variant", [(name, variant) for name in SCENES for variant in VARIANTS]
                         + [("many300", variant) for variant in ("default", "global", "treelets")])
def test_every_dword_equals_the_host_path(torch, rubik, monkeypatch, name, variant):
    """("many300", tests/rebuild_models_ref.py: 300 records.  srt_scene_refit schedules a record's root as a node slot of
    its height -- its tail has no loop over root records as the query refit's has -- so what 300 records add here is the
    schedule seeded by 301 roots, over 300 small trees of which many are a single leaf slot.)"""
    set_env(monkeypatch, variant)
    scene = small_scene(name, rubik)
    verts = RR.wave(scene.verts, 0.25, 0.3)
    a, b = S.Compute().Init(), S.Compute().Init()
    try:
        a.bind_scene(scene, refit=True)
        b.bind_scene(scene)
        before = a.scene_device()
        assert_arrays_equal(before, b.scene_device())  # refit=True uploads what the plain call uploads
        assert a.refit_get_int("refit.count") == 0
        heights, launches = a.refit_get_int("refit.heights"), a.refit_get_int("refit.launches")
        reached = int(RR.reached(scene).sum())
        assert a.refit_get_int("refit.bytes") >= 16 * len(scene.tris) + 8 * reached
        assert launches >= 2 and heights >= 1
        treelets = a.refit_get_int("refit.treelets")
        assert treelets == (1 if before[1] is not None else 0)
        if name == "many300":
            assert len(scene.bvhs) + 1 == 301 > 256  # the roots the schedule starts from (slot 0 among them)
        if variant == "treelets" and name in ("rubik", "grid", "two_models"):
            assert treelets == 1  # (a leaf root has no depth-3 node: those scenes carry no copy)
        if variant != "treelets":
            assert treelets == 0
        if name == "grid":
            # 713 leaves, more than 256 nodes at height 0: launches of whole heights precede the one-block tail
            assert len(scene.tris) == 1152 and launches >= 3
        elif name in ("one", "five"):
            assert len(scene.nodes) == 1 and heights == 1 and launches == 2  # the root is a leaf
        if variant == "global":
            # triangle slots by LayoutTris' rule, from the nodes alone: gaps before the leaves of one or two
            # triangles (the grid's, not Rubik's, whose leaves hold four and more)
            assert a.GetInt("scene.tri_slots") == expected_tri_slots(scene)
            if name in ("grid", "two_models"):
                assert a.GetInt("scene.tri_slots") > len(scene.tris)
        a.refit(verts_dev(torch, verts))
        assert a.refit_get_int("refit.count") == 1
        b.bind_scene(S.refit_scene(scene, verts))
        got, want = a.scene_device(), b.scene_device()
        assert_arrays_equal(got, want)
        assert not (got[0] == before[0]).all() and not (got[2] == before[2]).all()  # and it is no no-op
        assert (got[0][:2] == 0).all() and (got[0][-4:] == 0).all()  # the 32-B pad and the node_pad records
        assert (got[2][-9:] == 0).all()  # the tri_pad records
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("variant", ["default", "global", "treelets"])
def test_repeat_and_return(torch, rubik_scene, monkeypatch, variant):
    """Two refits to different phases, then back to the undeformed vertices: the fresh upload again, no drift."""
    set_env(monkeypatch, variant)
    scene = rubik_scene
    a, b = S.Compute().Init(), S.Compute().Init()
    try:
        a.bind_scene(scene, refit=True)
        b.bind_scene(scene)
        fresh = b.scene_device()
        a.refit(verts_dev(torch, RR.wave(scene.verts, 0.25, 0.3)))
        first = a.scene_device()
        a.refit(RR.wave(scene.verts, 0.4, 1.1))  # the numpy path uploads and synchronises
        second = a.scene_device()
        assert not (first[0] == second[0]).all() and not (first[2] == second[2]).all()
        b.bind_scene(S.refit_scene(scene, RR.wave(scene.verts, 0.4, 1.1)))
        assert_arrays_equal(second, b.scene_device())
        a.refit(verts_dev(torch, scene.verts))
        assert a.refit_get_int("refit.count") == 3
        assert_arrays_equal(a.scene_device(), fresh)
    finally:
        a.close()
        b.close()


def host_path_image(setup, verts):
    """4 spp on a fresh context that binds refit_scene(scene, verts): the host path."""
    rb = R.Renderer(dataclasses.replace(setup, scene=S.refit_scene(setup.scene, verts)))
    try:
        rb.render(4)
        return rb.accum().copy()
    finally:
        rb.close()


def render_pair(torch, setup, verts, read_roots, verts2=None):
    """Images on A: after the device refit, rendered again without one, and (with `verts2`) after a second refit
    enqueued while the pipeline's slot streams exist; then the host path's image(s) on fresh contexts."""
    ra = R.Renderer(setup)
    try:
        ra.compute.bind_scene(setup.scene, refit=True)
        ra.compute.refit(verts_dev(torch, verts), read_roots=read_roots)
        ra.render(4)  # nothing between the refit and the launches
        img = ra.accum().copy()
        ra.render(4)
        again = ra.accum().copy()
        third = None
        if verts2 is not None:
            # the slots' streams exist now: only the event the refit hands them orders their launches behind it
            ra.compute.refit(verts_dev(torch, verts2), read_roots=read_roots)
            ra.render(4)
            third = ra.accum().copy()
    finally:
        ra.close()
    ref = host_path_image(setup, verts)
    if verts2 is None:
        return img, again, ref
    return img, again, ref, third, host_path_image(setup, verts2)


@pytest.mark.parametrize("read_roots,force_global", [(False, False), (True, False), (False, True), (True, True)])
def test_renders_equal_the_host_path(torch, rubik, monkeypatch, read_roots, force_global):
    if force_global:
        monkeypatch.setenv("SRT_FORCE_GLOBAL_SCENE", "1")
    setup = R.make_setup(64, 48, show_model=True, models=[rubik])
    verts = RR.wave(setup.scene.verts, 0.25, 0.3)
    verts2 = RR.wave(setup.scene.verts, 0.4, 1.1)
    img, again, ref, third, ref2 = render_pair(torch, setup, verts, read_roots, verts2)
    assert bits_equal(img, ref).all()
    assert bits_equal(again, ref).all()
    assert bits_equal(third, ref2).all()  # a refit between two renders, through the slot streams' event wait
    assert not bits_equal(ref2, ref).all()
    # the deformation shows in the image: an undeformed render differs
    rc = R.Renderer(setup)
    try:
        rc.render(4)
        assert not bits_equal(rc.accum(), ref).all()
    finally:
        rc.close()


@pytest.mark.parametrize("before", ["reset", "trace_closest"])
def test_a_refit_before_the_first_pipelined_launch(torch, rubik, before):
    """bind(refit=True), then a call that leaves nothing for the first launch to synchronise on (a reset dispatch,
    or srt_trace_closest: either brings the BVH and light records up to date), then the refit behind other work on
    the caller's stream, then the context's first sample launch, which creates the pipeline's streams: the image
    is the host path's.  No slot stream exists when the refit is enqueued, so nothing but the call itself can
    order that launch behind it."""
    setup = R.make_setup(64, 48, show_model=True, models=[rubik])
    verts = RR.wave(setup.scene.verts, 0.25, 0.3)
    ra = R.Renderer(setup)
    try:
        c = ra.compute
        c.bind_scene(setup.scene, refit=True)
        ra.clear()  # accumFrames = 1 with the reset: what render(4) starts with
        if before == "trace_closest":
            c.trace_closest(rubik_rays(setup.scene, 64))
        vdev = verts_dev(torch, verts)
        # work the refit has to queue behind (Compute.refit makes the context's stream wait for this one)
        big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
        for _ in range(8):
            big.add_(1.0)
        c.refit(vdev)
        ra.render(4, clear=False)
        img = ra.accum().copy()
    finally:
        ra.close()
    del big
    assert bits_equal(img, host_path_image(setup, verts)).all()


def test_textured_render_equals_the_host_path(torch):
    """tri_uv is not touched: a sampled texture still lands where the host path puts it."""
    setup = SS.textured_setup()
    assert setup.scene.sample_textures
    verts = RR.wave(setup.scene.verts, 0.25, 0.3)
    img, again, ref = render_pair(torch, setup, verts, False)
    assert bits_equal(img, ref).all() and bits_equal(again, ref).all()
    assert (ref[..., :3] > 0).any()


def test_the_scene_object_upload_refits_alike(torch, rubik):
    """srt_upload_scene_obj_refit over a srt_scene handle: the upload and the refit of Compute.bind_scene(scene,
    refit=True), which goes through the arrays."""
    import ctypes as C

    from srt_amd import _lib

    lib = _lib.lib()
    scene = S.Scene.from_models([rubik])
    verts = RR.wave(scene.verts, 0.25, 0.3)
    hs = (C.c_void_p * 1)(rubik.handle)
    sh, rh = C.c_void_p(), C.c_void_p()
    assert lib.srt_scene_build(hs, 1, C.byref(sh)) == _lib.SRT_OK
    a, b = S.Compute().Init(), S.Compute().Init()
    try:
        rc = lib.srt_upload_scene_obj_refit(a.ctx, sh, C.byref(rh))
        assert rc == _lib.SRT_OK and rh.value, _lib.last_error()
        a._refit = rh  # (Compute owns and destroys it from here, as after bind_scene(refit=True))
        b.bind_scene(scene)
        assert_arrays_equal(a.scene_device(), b.scene_device())
        a.refit(verts_dev(torch, verts))
        b.bind_scene(S.refit_scene(scene, verts))
        assert_arrays_equal(a.scene_device(), b.scene_device())
    finally:
        lib.srt_scene_free(sh)
        a.close()
        b.close()


def test_trace_closest_after_a_refit_matches_the_oracle(torch, rubik_scene):
    verts = RR.wave(rubik_scene.verts)
    refit = S.refit_scene(rubik_scene, verts)
    rays = rubik_rays(rubik_scene, 4099)
    tri0, t0, _, _ = O.Oracle(rubik_scene).trace_closest(1, rays)
    tri1, t1, _, _ = O.Oracle(refit).trace_closest(1, rays)
    # the oracle alone: a no-op refit cannot pass for this deformation
    both = (tri0 != MISS) & (tri1 != MISS)
    assert both.sum() > 1000 and (t0[both].view(np.uint32) != t1[both].view(np.uint32)).mean() >= 0.5
    c = S.Compute().Init()
    try:
        c.bind_scene(rubik_scene, refit=True)
        c.SetUInt("bvh_count", 1)
        c.refit(verts_dev(torch, verts))
        hits, t = c.trace_closest(rays)
    finally:
        c.close()
    assert (hits == tri1).all() and bits_equal(t, t1).all()


def test_errors_leave_the_arrays_alone(torch, rubik_scene):
    from srt_amd import SrtError, _lib

    n = len(rubik_scene.verts)
    good = verts_dev(torch, RR.wave(rubik_scene.verts))
    c = S.Compute().Init()
    try:
        with pytest.raises(RuntimeError):
            c.refit(good)  # no bind_scene(refit=True) yet
        c.bind_scene(rubik_scene, refit=True)
        before = c.scene_device()
        for bad in (torch.cat([good, good[:1]]), good[:-1].contiguous()):  # a wrong n_verts
            with pytest.raises(SrtError) as e:
                c.refit(bad)
            assert e.value.code == _lib.SRT_ERR_INVALID
        flat = torch.zeros(8 * n + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(n, 8)  # contiguous, 4 B past a 16-B boundary
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        with pytest.raises(SrtError) as e:
            c.refit(view)
        assert e.value.code == _lib.SRT_ERR_INVALID
        with pytest.raises(ValueError):
            c.refit(good.cpu())
        with pytest.raises(ValueError):
            c.refit(good.to(torch.float64))
        # unknown flag bits, straight at the C entry point
        import ctypes as C
        assert _lib.lib().srt_scene_refit(c._refit, C.c_void_p(good.data_ptr()), n, 2) == _lib.SRT_ERR_INVALID
        assert c.refit_get_int("refit.count") == 0
        assert_arrays_equal(c.scene_device(), before)
        # a later upload on the context ends the object: SRT_ERR_STATE, nothing written
        stale = c._refit
        c._refit = None  # (bind_scene would destroy it; the stale handle is what is under test)
        c.bind_scene(small_scene("grid", None))
        after = c.scene_device()
        rc = _lib.lib().srt_scene_refit(stale, C.c_void_p(good.data_ptr()), n, 0)
        assert rc == _lib.SRT_ERR_STATE
        assert_arrays_equal(c.scene_device(), after)
        assert _lib.lib().srt_scene_refit_destroy(stale) == _lib.SRT_OK
        del e
    finally:
        c.close()
