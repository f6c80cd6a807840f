"""What the stage objects share (``Query``, ``Denoiser``, ``Temporal``, ``Surface``): the handle's life, the
stream a call runs on and its ordering with torch's current stream, ``get_int``, the checks of the tensors a call
is given, and the read-modify-write of a parameter struct."""
from __future__ import annotations

import ctypes as C
import gc

from ._lib import check, lib


class _Stage:
    """The handle of one ``<prefix>_create``d object (``_prefix``: ``srt_query``, ``srt_denoise``, ...).

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle.  With None the object runs on a stream of
    its own and ``_run`` orders every call with ``torch.cuda.current_stream()`` by events: the call waits for the
    work already queued there, and that stream waits for the results."""

    _prefix = ""

    def __init__(self, device, stream):
        self.device = int(device)
        self._h = None
        self._ext = None
        handle = getattr(stream, "cuda_stream", stream)
        self._own_stream = not handle
        self._stream_arg = C.c_void_p(handle) if handle else None

    def _fn(self, name):
        return getattr(lib(), f"{self._prefix}_{name}")

    def _create(self, *args, name="create"):
        """``<prefix>_<name>(device, stream, *args, &handle)``."""
        # Device tensors that only unreachable reference cycles still hold (a dead frame kept by its own traceback,
        # say) are returned now, at the one call of an object's life that allocates, and not at whatever later
        # moment the collector would pick: a caller who watches torch.cuda.memory_allocated() around the
        # enqueue-only calls then sees what those calls do, not a collection that happened to fall between them.
        gc.collect()
        h = C.c_void_p()
        check(self._fn(name)(self.device, self._stream_arg, *args, C.byref(h)), f"{self._prefix}_{name}")
        self._h = h

    # -- lifecycle ------------------------------------------------------------
    def close(self):
        if self._h is not None:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError(f"{type(self).__name__} is closed")
        return self._h

    def get_int(self, name: str) -> int:
        v = C.c_int()
        check(self._fn("get_int")(self.handle, name.encode(), C.byref(v)), f"{self._prefix}_get_int({name})")
        return v.value

    # -- work -----------------------------------------------------------------
    def _ordered(self, torch):
        """The library's own stream as a torch stream (default-stream mode), else None."""
        if not self._own_stream:
            return None
        if self._ext is None:
            self._ext = torch.cuda.ExternalStream(int(self._fn("stream")(self.handle)), device=self.device)
        return self._ext

    def _run(self, call, what):
        import torch
        ext = self._ordered(torch)
        cur = torch.cuda.current_stream(self.device) if ext is not None else None
        if ext is not None:
            ext.wait_stream(cur)
        check(call(), what)
        if ext is not None:
            cur.wait_stream(ext)

    def synchronize(self):
        """Wait for the work enqueued so far."""
        import torch
        torch.cuda.ExternalStream(int(self._fn("stream")(self.handle) or 0), device=self.device).synchronize()


# -- arguments: each returns (device pointer or None, the object that keeps it alive) ------------------------------
def _on_device(t, dtype, device):
    return t.dtype == dtype and t.is_cuda and t.device.index == device and t.is_contiguous()


def image_arg(name, t, W, H, device):
    """A contiguous float32 ``[H, W, 4]`` tensor on ``cuda:device``."""
    import torch
    if not _on_device(t, torch.float32, device) or t.numel() != W * H * 4:
        raise ValueError(f"{name} must be a contiguous float32 [H, W, 4] tensor on cuda:{device}")
    return t.data_ptr(), t


def accum_arg(t, W, H, device):
    """The accumulation image: ``image_arg``, or a raw device pointer (int)."""
    return (t, None) if isinstance(t, int) else image_arg("accum", t, W, H, device)


def _records_arg(t, n, device, required, dtype, text):
    raw = getattr(t, "raw", t)
    if raw is None and not required:
        return None, None
    if raw is None or not _on_device(raw, dtype, device) or tuple(raw.shape) != (n, 8):
        raise ValueError(f"{text} on cuda:{device}")
    return raw.data_ptr(), raw


def hits_arg(hits, n, device, required=True, text="hits must be the [W * H, 8] int32 srt_hit tensor"):
    """A :class:`srt_amd.query.Hits` or its ``[n, 8]`` int32 tensor; None passes when not ``required``."""
    import torch
    return _records_arg(hits, n, device, required, torch.int32, text)


def attrs_arg(attrs, n, device, required=True):
    """``Surface.shade``'s ``[n, 8]`` float32 tensor; None passes when not ``required``."""
    import torch
    return _records_arg(attrs, n, device, required, torch.float32, "attrs must be the [W * H, 8] float32 srt_surface_attr tensor")


def rays_arg(rays, device):
    """A contiguous float32 ``[n, 8]`` tensor of ``srt_ray`` records on ``cuda:device``."""
    import torch
    if not _on_device(rays, torch.float32, device) or rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"rays must be a contiguous float32 [n, 8] tensor on cuda:{device} (srt_ray fields)")
    return rays.data_ptr(), rays


def verts_arg(verts, device):
    """A contiguous float32 ``[n_verts, 8]`` tensor of ``srt_vertex`` records on ``cuda:device``."""
    import torch
    if not _on_device(verts, torch.float32, device) or verts.dim() != 2 or verts.shape[1] != 8:
        raise ValueError(f"verts must be a contiguous float32 [n_verts, 8] tensor on cuda:{device} (srt_vertex fields)")
    return verts.data_ptr(), verts


# -- parameter structs ---------------------------------------------------------------------------------------------
def get_params(struct, getter, handle, what) -> dict:
    p = struct()
    check(getter(handle, C.byref(p)), what)
    return {n: getattr(p, n) for n, _ in struct._fields_}


def updated_params(struct, cur: dict, kw: dict, kind: str):
    """``struct`` from ``cur`` with ``kw`` over it: TypeError for a name the struct lacks, ValueError for an
    unsigned 32-bit field out of range."""
    unknown = set(kw) - set(cur)
    if unknown:
        raise TypeError(f"unknown {kind} parameter(s): {sorted(unknown)}")
    cur = {**cur, **kw}
    vals = []
    for n, t in struct._fields_:
        if t is C.c_float:
            vals.append(float(cur[n]))
        else:
            vals.append(int(cur[n]))
            if t is C.c_uint32 and not 0 <= vals[-1] <= 0xFFFFFFFF:
                raise ValueError(f"{n} must fit an unsigned 32-bit integer")
    return struct(*vals)
