"""Guided upsampling of low-resolution progressive frames (include/srt_upsample.h).

``Upsampler(low_w, low_h, factor)`` reconstructs a ``factor * low_w`` x ``factor * low_h`` frame from the
accumulation image of a ``low_w`` x ``low_h`` render, with joint-bilateral weights from two guides: ``Query.closest``
of ``Denoiser.primary_rays`` at the low and at the full size.  ``run`` returns device tensors; its float result is a
valid accumulation image over ``frames = 1`` for ``Temporal.accumulate`` and ``Denoiser.run``.  Nothing leaves the
device and no call synchronises.  Full frames and integer factors 1..4 only.
"""
from __future__ import annotations

import ctypes as C

from ._lib import UpsampleParams, check, lib
from ._stage import _Stage, accum_arg, get_params, hits_arg, updated_params

__all__ = ["Upsampler"]


class Upsampler(_Stage):
    """An upsampler from ``low_w`` x ``low_h`` by ``factor`` on ``device``.

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle.  With the default (None) the object runs
    on a stream of its own and orders every call with ``torch.cuda.current_stream()`` by events, exactly as
    :class:`srt_amd.denoise.Denoiser` does.
    """

    _prefix = "srt_upsample"

    def __init__(self, low_w: int, low_h: int, factor: int, device: int = 0, stream=None):
        super().__init__(device, stream)
        self.low_width, self.low_height, self.factor = int(low_w), int(low_h), int(factor)
        self._create(self.low_width, self.low_height, self.factor)
        self.width, self.height = self.get_int("width"), self.get_int("height")

    # -- state ----------------------------------------------------------------
    @property
    def params(self) -> dict:
        return get_params(UpsampleParams, lib().srt_upsample_get_params, self.handle, "srt_upsample_get_params")

    def set_params(self, **kw):
        """Any of normal_squarings, sigma_depth; the other keeps its value."""
        p = updated_params(UpsampleParams, self.params, kw, "upsampler")
        check(lib().srt_upsample_set_params(self.handle, C.byref(p)), "srt_upsample_set_params")

    # -- work -----------------------------------------------------------------
    def run(self, low_accum, frames: int, low_hits, full_hits, *, srgb: bool = False):
        """Upsample ``low_accum`` (the SUM over ``frames``): a contiguous float32 ``[low_h, low_w, 4]`` device tensor,
        or a raw device pointer (int).  ``low_hits`` / ``full_hits``: the guides of the pixel-centre rays at the two
        sizes, each a :class:`srt_amd.query.Hits` or its ``[n, 8]`` int32 tensor.  Returns the float32 ``[H, W, 4]``
        result on the device, and with ``srgb=True`` the pair (float32 image, uint8 ``[H, W, 4]`` sRGB image)."""
        import torch
        dev = f"cuda:{self.device}"
        acc_ptr, keep = accum_arg(low_accum, self.low_width, self.low_height, self.device)
        low_ptr, low_raw = hits_arg(low_hits, self.low_width * self.low_height, self.device,
                                    text="low_hits must be the [low_w * low_h, 8] int32 srt_hit tensor")
        full_ptr, full_raw = hits_arg(full_hits, self.width * self.height, self.device,
                                      text="full_hits must be the [W * H, 8] int32 srt_hit tensor")
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        out8 = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=dev) if srgb else None
        self._run(lambda: lib().srt_upsample_run(self.handle, C.c_void_p(acc_ptr), int(frames), C.c_void_p(low_ptr),
                                                 C.c_void_p(full_ptr), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(out8.data_ptr()) if srgb else None), "srt_upsample_run")
        del keep, low_raw, full_raw
        return (out, out8) if srgb else out
