"""The argument checks the stage objects share (srt_amd/_stage.py), CPU only and without a device: the ValueErrors
of Denoiser / Temporal / Surface / Query for a tensor of the wrong dtype, place, layout or size, what passes them,
and the read-modify-write of a parameter struct.  W x H = 4 x 3 on "cuda:0" (no tensor here is on it)."""
import ctypes as C

import pytest
import torch

from srt_amd import _lib
from srt_amd import _stage as S

W, H, DEV = 4, 3, 0
N = W * H
IMAGE = "accum must be a contiguous float32 [H, W, 4] tensor on cuda:0"
HITS = "hits must be the [W * H, 8] int32 srt_hit tensor on cuda:0"
ATTRS = "attrs must be the [W * H, 8] float32 srt_surface_attr tensor on cuda:0"
RAYS = "rays must be a contiguous float32 [n, 8] tensor on cuda:0 (srt_ray fields)"


class OnDevice:
    """A CPU tensor that reports itself on cuda:`index`: what a check sees of a device tensor."""

    class _Device:
        def __init__(self, index):
            self.index = index

    def __init__(self, t, index=DEV):
        self._t, self.is_cuda, self.device = t, True, self._Device(index)

    def __getattr__(self, name):
        return getattr(self._t, name)


def raises(message, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_image_and_accum_arguments():
    good = torch.zeros((H, W, 4), dtype=torch.float32)
    raises(IMAGE, S.accum_arg, good, W, H, DEV)                                    # not on the device
    raises(IMAGE, S.accum_arg, OnDevice(good, 1), W, H, DEV)                       # on another device
    raises(IMAGE, S.accum_arg, OnDevice(good.to(torch.float64)), W, H, DEV)        # wrong dtype
    raises(IMAGE, S.accum_arg, OnDevice(torch.zeros((H, W, 8))[..., ::2]), W, H, DEV)  # not contiguous
    raises(IMAGE, S.accum_arg, OnDevice(torch.zeros((H, W + 1, 4))), W, H, DEV)    # wrong element count
    raises(IMAGE, S.accum_arg, OnDevice(torch.zeros((H, W, 3))), W, H, DEV)
    for name in ("colour", "moments"):
        raises(IMAGE.replace("accum", name), S.image_arg, name, good, W, H, DEV)
    ok = OnDevice(good)
    assert S.accum_arg(ok, W, H, DEV) == (good.data_ptr(), ok)
    assert S.image_arg("colour", OnDevice(good.reshape(N, 4)), W, H, DEV)[0] == good.data_ptr()  # the count, not the shape
    assert S.accum_arg(0x7F0000001000, W, H, DEV) == (0x7F0000001000, None)         # an int is a raw device pointer


def test_hits_and_attrs_arguments():
    hits = torch.zeros((N, 8), dtype=torch.int32)
    attrs = torch.zeros((N, 8), dtype=torch.float32)
    for fn, good, text in ((S.hits_arg, hits, HITS), (S.attrs_arg, attrs, ATTRS)):
        raises(text, fn, good, N, DEV)                                              # not on the device
        raises(text, fn, OnDevice(good, 1), N, DEV)
        raises(text, fn, OnDevice(good.to(torch.int64)), N, DEV)                    # wrong dtype
        raises(text, fn, OnDevice(torch.zeros((N, 16), dtype=good.dtype)[:, ::2]), N, DEV)  # not contiguous
        for shape in ((N + 1, 8), (N, 7), (N * 8,), (H, W, 8)):                     # wrong shape, the right count included
            raises(text, fn, OnDevice(torch.zeros(shape, dtype=good.dtype)), N, DEV)
        raises(text, fn, None, N, DEV)                                              # required by default
        raises(text, fn, None, N, DEV, required=True)
        assert fn(None, N, DEV, required=False) == (None, None)
        ok = OnDevice(good)
        assert fn(ok, N, DEV) == (good.data_ptr(), ok)
        raises(text, fn, OnDevice(good.to(torch.float64)), N, DEV, required=False)  # optional, but checked when given
    raises(HITS, S.hits_arg, OnDevice(attrs), N, DEV)                               # each the other's dtype
    raises(ATTRS, S.attrs_arg, OnDevice(hits), N, DEV)

    class Hits:  # srt_amd.query.Hits: the tensor is its `raw`
        raw = OnDevice(hits)

    assert S.hits_arg(Hits(), N, DEV) == (hits.data_ptr(), Hits.raw)
    # Surface.shade's wording, for the hits of n rays
    text = "hits must be the [n, 8] int32 srt_hit tensor of the rays"
    raises(text + " on cuda:0", S.hits_arg, OnDevice(hits), N - 1, DEV, text=text)


def test_rays_argument():
    rays = torch.zeros((5, 8), dtype=torch.float32)
    raises(RAYS, S.rays_arg, rays, DEV)
    raises(RAYS, S.rays_arg, OnDevice(rays, 1), DEV)
    raises(RAYS, S.rays_arg, OnDevice(rays.to(torch.float16)), DEV)
    raises(RAYS, S.rays_arg, OnDevice(torch.zeros((5, 16))[:, ::2]), DEV)
    raises(RAYS, S.rays_arg, OnDevice(torch.zeros((5, 7))), DEV)
    raises(RAYS, S.rays_arg, OnDevice(torch.zeros((40,))), DEV)
    raises(RAYS, S.rays_arg, OnDevice(torch.zeros((5, 1, 8))), DEV)
    ok = OnDevice(rays)
    assert S.rays_arg(ok, DEV) == (rays.data_ptr(), ok)
    assert S.rays_arg(OnDevice(torch.zeros((0, 8))), DEV)[1] is not None            # no ray is a valid batch


def test_params_read_modify_write():
    cur = {"max_history": 32, "depth_tol": 0.05, "normal_min": 0.9}
    p = S.updated_params(_lib.TemporalParams, cur, {"max_history": 7.0, "normal_min": 0}, "temporal")
    assert isinstance(p, _lib.TemporalParams)
    assert (p.max_history, p.depth_tol, p.normal_min) == (7, C.c_float(0.05).value, 0.0)
    assert cur["max_history"] == 32                                                  # the caller's dict is left alone
    assert S.updated_params(_lib.TemporalParams, cur, {"max_history": 0xFFFFFFFF}, "temporal").max_history == 0xFFFFFFFF
    with pytest.raises(TypeError) as e:
        S.updated_params(_lib.TemporalParams, cur, {"history": 3, "depth": 1.0}, "temporal")
    assert str(e.value) == "unknown temporal parameter(s): ['depth', 'history']"
    with pytest.raises(TypeError) as e:
        S.updated_params(_lib.DenoiseParams, {"passes": 5, "normal_squarings": 5, "sigma_color": 1.0, "sigma_depth": 1.0},
                         {"sigma": 2.0}, "denoiser")
    assert str(e.value) == "unknown denoiser parameter(s): ['sigma']"
    for bad in (1 << 32, (1 << 32) + 5, -1):
        raises("max_history must fit an unsigned 32-bit integer", S.updated_params, _lib.TemporalParams, cur,
               {"max_history": bad}, "temporal")
        raises("min_history must fit an unsigned 32-bit integer", S.updated_params, _lib.DenoiseVarParams,
               {"sigma_lum": 4.0, "min_history": 4}, {"min_history": bad}, "variance")
    with pytest.raises(TypeError) as e:
        S.updated_params(_lib.DenoiseVarParams, {"sigma_lum": 4.0, "min_history": 4}, {"sigma": 1}, "variance")
    assert str(e.value) == "unknown variance parameter(s): ['sigma']"


def test_stage_host_under_sanitizers():
    """tests/cpp/test_stage_host.cpp with csrc/stage_host.cpp and the scene producers linked directly, AddressSanitizer
    + UBSan, as a stand-alone program (`make SAN=1 test_stage_host`: host code only, no HIP runtime, no device, nothing
    preloaded): SaturateInt, the alignment predicate, and SceneArrays against srt_scene_sizes / srt_scene_copy."""
    import subprocess

    from conftest import PKG

    r = subprocess.run(["make", "-s", "-C", str(PKG), "SAN=1", "-j8", "test_stage_host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_stage_host: OK" in r.stdout


def test_a_closed_object_names_its_class():
    """The lifecycle of the base without a library call: no handle was ever created."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.surface import Surface
    from srt_amd.temporal import Temporal

    for cls, prefix in ((Query, "srt_query"), (Denoiser, "srt_denoise"), (Temporal, "srt_temporal"), (Surface, "srt_surface")):
        assert issubclass(cls, S._Stage) and cls._prefix == prefix
        obj = cls.__new__(cls)
        S._Stage.__init__(obj, 0, None)
        assert obj._own_stream and obj._stream_arg is None
        with pytest.raises(RuntimeError) as e:
            obj.handle
        assert str(e.value) == f"{cls.__name__} is closed"
        obj.close()  # nothing to destroy
        with obj as same:
            assert same is obj
        S._Stage.__init__(obj, 0, 0x1234)  # a raw hipStream_t
        assert not obj._own_stream and obj._stream_arg.value == 0x1234
