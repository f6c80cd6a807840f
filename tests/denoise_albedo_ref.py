"""The numpy float32 restatement of srt_denoise_run_albedo (include/srt_surface.h; DESIGN.md section 5, "Surface
attributes and demodulation"), built on tests/denoise_ref.py: the filter itself is denoise_ref.atrous, unchanged.

For a hit pixel a = max(albedo, floor) per channel (the floor where the albedo is not greater), C0 = (accum.xyz /
float(frames)) / a, the passes run on C0, and the output is C_passes * a.  Miss pixels keep accum.xyz / float(frames)
through every pass (the filter leaves them alone) and are not multiplied.  It never calls into the library.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D


def floored(albedo, floor):
    """max(albedo, floor) as the kernel takes it: albedo where it is greater than the floor, else the floor."""
    albedo = np.asarray(albedo, np.float32)
    return np.where(albedo > np.float32(floor), albedo, np.float32(floor)).astype(np.float32)


def demodulate(accum, frames, guide, albedo, floor):
    """(C0, a): the first pass's input and the per-pixel divisor ((H, W, 3) each; a is 1 where it is not applied)."""
    hit = (guide["tri"] != D.MISS)[..., None]
    a = np.where(hit, floored(albedo, floor), np.float32(1)).astype(np.float32)
    mean = D.mean_colour(accum, frames)
    with np.errstate(all="ignore"):
        C0 = np.where(hit, mean / a, mean).astype(np.float32)
    return C0, a


def run_albedo(accum, frames, guide, albedo, floor, passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2):
    """The float output's colour (H, W, 3).  `albedo` is (H, W, 3): the attrs' albedo, index j * W + i reshaped.
    passes == 0 is srt_denoise_run's result: the mean."""
    if passes == 0:
        return D.mean_colour(accum, frames)
    hit = (guide["tri"] != D.MISS)[..., None]
    C0, a = demodulate(accum, frames, guide, albedo, floor)
    C = D.atrous(C0, guide, passes, normal_squarings, sigma_color, sigma_depth)
    with np.errstate(all="ignore"):
        out = np.where(hit, C * a, C).astype(np.float32)
    return out
