"""Render a scene to an image file on the GPU: the reference's progressive loop, headless.

usage: python tools/render.py [--scene rubik|spheres|synthetic|torusknot|airplane_knot] [--width W] [--height H] [--spp N]
                              [--max-depth D] [--out frame.png] [--denoise] [--albedo] [--orbit K] [--spin DEG] [--variance]
                              [--wave A [--orbit K [--albedo] [--rebuild-every K [--rebuild-leaf L]]]]
                              [--upsample F]
The output is image0 after N sampled frames (src/main.cpp:642-659 accumulation schedule),
written top row first (PNG or PPM by extension).
"""
import argparse
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "simple-ray-tracer_amd"))

from srt_amd import render as R  # noqa: E402


def parse_args(ap, argv=None):
    """The arguments, with the checks of --upsample F (the others are main's)."""
    a = ap.parse_args(argv)
    if a.upsample is not None:
        if not 1 <= a.upsample <= 4:
            ap.error("--upsample F: F in 1..4")
        if a.width % a.upsample or a.height % a.upsample:
            ap.error(f"--upsample {a.upsample}: --width and --height must be multiples of {a.upsample}")
        if a.scene == "spheres":
            ap.error("--upsample needs a mesh scene: the guides are ray queries")
    return a


def scene_models(a):
    """The models of a mesh scene."""
    if a.scene == "rubik":
        return [R.rubik_model(ROOT / "tests" / "golden" / "objects")]
    if a.scene == "synthetic":
        return [R.synthetic_model(a.synthetic_tris)]
    if a.scene == "torusknot":
        return [R.torus_knot_model()]
    sys.path.insert(0, str(ROOT))  # airplane_knot: the surface mesh carrying the Airplane's textured materials (bench.py leg)
    import bench

    return [bench.airplane_knot_model()]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rubik", choices=("rubik", "spheres", "synthetic", "torusknot", "airplane_knot"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--synthetic-tris", type=int, default=1_000_000)
    ap.add_argument("--out", default="frame.png")
    ap.add_argument("--denoise", action="store_true",
                    help="also write <out>_denoised.<ext>: the frame through the edge-avoiding filter, guided by a "
                         "closest-hit query of the pixel-centre rays (mesh scenes; sphere pixels pass unfiltered)")
    ap.add_argument("--albedo", action="store_true",
                    help="with --denoise (mesh scenes): also write <out>_albedo_denoised.<ext>, the frame through the "
                         "albedo-demodulated filter (include/srt_surface.h): srt_surface_shade of the guide, run_albedo")
    ap.add_argument("--orbit", type=int, default=0, metavar="K",
                    help="mesh scenes: render K frames of --spp each along a small fixed camera path, resetting the "
                         "accumulation per frame as the frame loop does while the camera moves, and write the last "
                         "frame three ways: <out> (raw), <out>_denoised and <out>_temporal (accumulated over the path "
                         "by temporal reprojection, then denoised)")
    ap.add_argument("--spin", type=float, default=0.0, metavar="DEG",
                    help="with --orbit K: the camera stands still and the first model turns by DEG degrees per frame "
                         "about the vertical axis through its bounds' centre; each frame's matrix goes to the renderer, "
                         "the query and the temporal object, whose history follows the model")
    ap.add_argument("--variance", action="store_true",
                    help="with --orbit K (and --spin): the temporal object also integrates luminance moments, and the "
                         "last frame is written a fourth way, <out>_svgf: temporally accumulated, then through the "
                         "variance-guided filter (include/srt_variance.h)")
    ap.add_argument("--wave", type=float, default=0.0, metavar="A",
                    help="mesh scenes: displace the model's vertices by a sine of amplitude A before rendering "
                         "(include/srt_refit.h): the tracer gets the host-refit scene (refit_scene + bind_scene), and with "
                         "--denoise the guide query is refit on the device (Query(scene, refit=True).refit), as is "
                         "the surface object of --albedo (Surface(scene, refit=True).refit).  With --orbit K the camera "
                         "stands still and the wave's phase advances by WAVE_PHASE_STEP per frame: each frame's vertices "
                         "go to the renderer (bound once with refit=True, then Compute.refit on the device: "
                         "include/srt_scene_refit.h), the query, the temporal object, whose history follows the "
                         "surface (include/srt_temporal_deform.h), and with --albedo the surface object")
    ap.add_argument("--rebuild-every", type=int, default=0, metavar="K",
                    help="with --wave A --orbit N: every K-th frame the guide query gets a new tree, built on the device "
                         "(Query(scene, refit=True, rebuild=True).rebuild, include/srt_rebuild.h), and is refit otherwise")
    ap.add_argument("--rebuild-leaf", type=int, default=None, metavar="L",
                    help="with --rebuild-every K: those trees collapse every subtree of at most L triangles (1..255) into one "
                         "leaf (Query.set_rebuild_leaf, include/srt_rebuild_leaf.h); the default is one triangle a leaf")
    ap.add_argument("--upsample", type=int, default=None, metavar="F",
                    help="mesh scenes: render at (W / F) x (H / F) with F * F * spp samples (the same ray budget), write "
                         "that frame to <out> and its guided upsampling to W x H (include/srt_upsample.h; guides: closest-hit "
                         "queries of the pixel-centre rays at the two sizes) to <out>_upsampled.<ext>.  Every other stage "
                         "asked for (--denoise, --albedo, --orbit, --spin, --variance, --wave) runs at W x H on the "
                         "upsampled frame, a sum over one frame, with the full-size guide.  F in 1..4; W and H must be "
                         "multiples of F")
    a = parse_args(ap, argv)
    f = a.upsample or 0  # 0: no upsampling, the frame is rendered at W x H
    if a.rebuild_every and (a.rebuild_every < 0 or not (a.wave and a.orbit)):
        ap.error("--rebuild-every K (K > 0) needs --wave A --orbit N")
    if a.rebuild_leaf is not None and (not a.rebuild_every or not 1 <= a.rebuild_leaf <= 255):
        ap.error("--rebuild-leaf L (1..255) needs --rebuild-every K")
    if a.wave and a.scene == "spheres":
        ap.error("--wave A needs a mesh scene")
    if a.wave and a.orbit and a.spin:
        ap.error("--wave A --orbit K advances the wave under a still camera: without --spin")
    if a.albedo and (not a.denoise or a.scene == "spheres" or (a.orbit and not a.wave)):
        ap.error("--albedo needs --denoise on a mesh scene, and with --orbit K also --wave A")
    if a.variance and not a.orbit:
        ap.error("--variance needs --orbit K")
    if a.spin and not a.orbit:
        ap.error("--spin DEG needs --orbit K")
    if a.orbit and a.scene == "spheres":
        ap.error("--orbit needs a mesh scene: the guide is a ray query")
    if a.orbit < 0:
        ap.error("--orbit K: K >= 1")
    models, show = (None, False) if a.scene == "spheres" else (scene_models(a), True)
    width, height, spp = (a.width // f, a.height // f, f * f * a.spp) if f else (a.width, a.height, a.spp)
    setup = R.make_setup(width, height, show_model=show, models=models, max_depth=a.max_depth)
    r = R.Renderer(setup)
    wave_verts = None
    if a.wave:  # the host half: the same topology, the boxes refit to the displaced vertices, uploaded again
        import srt_amd as S

        wave_verts = R.wave_vertices(setup.scene.verts, a.wave)
        r.compute.bind_scene(S.refit_scene(setup.scene, wave_verts))
    if a.orbit:
        try:
            t0 = time.perf_counter()
            paths = orbit(r, setup, a.orbit, spp, a.out, a.spin, a.variance, a.wave, a.albedo, a.rebuild_every, a.rebuild_leaf,
                          upsample=f)
            dt = time.perf_counter() - t0
        finally:
            r.close()
        print(f"{a.orbit} frames of {width}x{height} @ {spp} spp in {dt:.3f} s; the last one:")
        whats = ("raw", "denoised", "temporal + denoised") + (("temporal + variance-guided filter",) if a.variance else ())
        if f:
            whats = tuple(f"upsampled to {a.width}x{a.height}, {w}" for w in whats[1:])
            whats = ("raw",) + whats + (f"upsampled to {a.width}x{a.height}",)
        for what, p in zip(whats, paths):
            print(f"{p}: {what}")
        return
    try:
        t0 = time.perf_counter()
        r.render(spp)
        r.finish()
        dt = time.perf_counter() - t0
        r.compute.save_image(a.out)
        if a.denoise or f:
            written = denoise(r, setup, a.out, a.albedo, wave_verts, upsample=f, filtered=a.denoise)
    finally:
        r.close()
    print(f"{a.out}: {width}x{height} @ {spp} spp in {dt:.3f} s")
    if f:
        print(f"{written[-1]}: upsampled to {a.width}x{a.height}")
    if a.denoise:
        print(f"{written[0]}: filtered")
        if a.albedo:
            print(f"{written[1]}: filtered on albedo-demodulated radiance")


def denoise(r, setup, out, albedo=False, wave_verts=None, upsample=0, filtered=True):
    """The finished frame of Renderer `r` through srt_amd.denoise.Denoiser, written beside `out`; with `albedo` also
    through run_albedo on the attrs of srt_amd.surface.Surface.  With `wave_verts` (the displaced vertices the frame
    was rendered with) the guide query is created over the undeformed scene and refit to them on the device.
    With `upsample` = F the frame is first upsampled by F (srt_amd.upsample.Upsampler; a second guide at the frame's own
    size), written to <out>_upsampled, and the filters run at the full size on that image, a sum over one frame;
    `filtered` False stops there.  Returns the paths written, the upsampled one last."""
    import srt_amd as S
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.surface import Surface

    out = pathlib.Path(out)
    path = out.with_name(out.stem + "_denoised" + out.suffix)
    upath = out.with_name(out.stem + "_upsampled" + out.suffix)
    acc_ptr, _ = r.compute.image_pointers()
    frames = r.accum_frames
    f = upsample or 1
    with Denoiser(f * setup.width, f * setup.height) as dn:
        hits = None
        if setup.scene is not None:
            with Query(setup.scene, refit=wave_verts is not None) as q:
                q.set_bvh_count(setup.bvh_count)
                if wave_verts is not None:
                    q.refit(wave_verts)
                rays = dn.primary_rays(setup.camera)
                hits = q.closest(rays)
                if upsample:
                    from srt_amd.upsample import Upsampler

                    with Denoiser(setup.width, setup.height) as dl, Upsampler(setup.width, setup.height, f) as up:
                        acc_ptr, rgba8 = up.run(acc_ptr, frames, q.closest(dl.primary_rays(setup.camera)), hits, srgb=True)
                        frames = 1  # the upsampled image is a sum over one frame
                        up.synchronize()
                    S.write_image(upath, rgba8.cpu().numpy())
                q.synchronize()
            if not filtered:
                return (upath,)
            if albedo:
                with Surface(setup.scene, refit=wave_verts is not None) as surf:
                    surf.set_bvh_count(setup.bvh_count)
                    if wave_verts is not None:
                        surf.refit(wave_verts)
                    attrs = surf.shade(rays, hits)
                    surf.synchronize()
                apath = out.with_name(out.stem + "_albedo_denoised" + out.suffix)
                _, rgba8 = dn.run_albedo(acc_ptr, frames, hits, attrs, srgb=True)
                dn.synchronize()
                S.write_image(apath, rgba8.cpu().numpy())
        else:
            dn.set_params(passes=0)  # a sphere scene has no mesh to query: the frame passes through
        _, rgba8 = dn.run(acc_ptr, frames, hits, srgb=True)
        dn.synchronize()
        S.write_image(path, rgba8.cpu().numpy())
    return ((path, apath) if albedo else (path,)) + ((upath,) if upsample else ())


ORBIT_STEP = (0.5, -1.0)  # per frame: MoveRight(0.5), then Rotate(-1 degree of yaw, 0): the camera circles the model
WAVE_PHASE_STEP = 0.3     # per frame, radians: --wave A --orbit K


def spin_frame(scene, degrees):
    """Record 0's `frame` (world -> model, glm column-major) with the model turned by `degrees` about the vertical
    axis through the centre of the scene's bounds: the inverse rotation about that axis."""
    import numpy as np

    v = scene.verts["pos"].astype(np.float64)
    centre = (v.min(0) + v.max(0)) / 2
    c, s = np.cos(np.radians(-degrees)), np.sin(np.radians(-degrees))
    m = np.eye(4)
    m[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    m[:3, 3] = centre - m[:3, :3] @ centre
    return m.T.reshape(16).astype(np.float32)


def orbit(r, setup, frames, spp, out, spin=0.0, variance=False, wave=0.0, albedo=False, rebuild_every=0, rebuild_leaf=None,
          upsample=0):
    """`frames` frames of `spp` samples, each after a reset of the accumulation: along ORBIT_STEP, or with `spin`
    (degrees per frame) under a still camera while the first model turns, or with `wave` (the amplitude) under a
    still camera while the wave's phase advances -- the per-frame calls of a deforming mesh, all on the device
    vertices: Compute.refit for the renderer (bound once with refit=True; no per-frame bind_scene), Query.refit,
    Temporal.set_vertices and, with `albedo`, Surface.refit, whose attrs
    then demodulate the two filtered images.  Every frame goes through
    srt_amd.temporal.Temporal (guide: a closest-hit query of the pixel-centre rays).  Writes the last frame raw,
    denoised, and temporally accumulated then denoised, and with `variance` also temporally accumulated then through
    the variance-guided filter (<out>_svgf); returns the paths.  With `upsample` = F the renderer's frames are F times
    smaller than the stages': each is upsampled first (srt_amd.upsample.Upsampler; a second guide at the frame's own
    size), and the temporal object, the filters and the surface object work at the full size on that image, a sum over
    one frame, with the full-size guide; the last upsampled frame is written too (<out>_upsampled, the last path)."""
    import contextlib

    import numpy as np
    import torch

    import srt_amd as S
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.surface import Surface
    from srt_amd.temporal import Temporal
    from srt_amd.upsample import Upsampler

    out = pathlib.Path(out)
    paths = [out] + [out.with_name(out.stem + s + out.suffix) for s in ("_denoised", "_temporal") + (("_svgf",) if variance else ()) +
                     (("_upsampled",) if upsample else ())]
    cam, c = setup.camera, r.compute
    acc_ptr, _ = c.image_pointers()
    f = upsample or 1
    W, H = f * setup.width, f * setup.height
    with Denoiser(W, H) as dn, Temporal(W, H) as tp, \
            (Denoiser(setup.width, setup.height) if upsample else contextlib.nullcontext()) as dl, \
            (Upsampler(setup.width, setup.height, f) if upsample else contextlib.nullcontext()) as up, \
            Query(setup.scene, refit=bool(wave), rebuild=bool(rebuild_every), rebuild_leaf=rebuild_leaf) as q, \
            (Surface(setup.scene, refit=True) if albedo else contextlib.nullcontext()) as surf:
        q.set_bvh_count(setup.bvh_count)
        if wave:
            tp.set_mesh(setup.scene)
            c.bind_scene(setup.scene, refit=True)  # once: the frames refit it on the device (srt_scene_refit.h)
        if albedo:
            surf.set_bvh_count(setup.bvh_count)
        if variance:
            tp.enable_moments()
            dn.enable_variance()
        for k in range(frames):
            if spin:  # the three per-frame calls of a moving model
                frame = spin_frame(setup.scene, spin * (k + 1))
                S.UpdateModelMatrix(c, 0, frame)
                q.update_model_matrix(0, frame)
                tp.set_models([frame])
            elif wave:  # the per-frame calls of a deforming mesh
                verts = R.wave_vertices(setup.scene.verts, wave, WAVE_PHASE_STEP * k)
                vdev = torch.from_numpy(np.ascontiguousarray(verts).view(np.float32).reshape(-1, 8)).to(f"cuda:{r.compute.device}")
                c.refit(vdev)
                if rebuild_every and k % rebuild_every == rebuild_every - 1:
                    q.rebuild(vdev)  # a new tree for the guide; its hits keep the scene's triangle indices
                else:
                    q.refit(vdev)
                tp.set_vertices(vdev)
                if albedo:
                    surf.refit(vdev)
            elif k:
                cam.MoveRight(ORBIT_STEP[0])
                cam.Rotate(ORBIT_STEP[1], 0.0)
                c.SetVec3("cameraOrigin", cam.getOrigin())
                c.SetVec3("cameraDirection", cam.getForward())
                c.SetVec3("cameraUp", cam.getUpVector())
                c.SetVec3("cameraRight", cam.getRightVector())
            r.render(spp)  # clears first: the frame loop resets on any input
            r.finish()
            rays = dn.primary_rays(cam)
            hits = q.closest(rays)
            frame, n = acc_ptr, r.accum_frames
            if upsample:  # the stages below see a full-size sum over one frame
                frame, rgba8_u = up.run(acc_ptr, n, q.closest(dl.primary_rays(cam)), hits, srgb=True)
                n = 1
            if variance:
                acc, mom = tp.accumulate_moments(frame, n, hits, cam)
            else:
                acc = tp.accumulate(frame, n, hits, cam)
        c.save_image(paths[0])
        if upsample:
            up.synchronize()
            S.write_image(paths[-1], rgba8_u.cpu().numpy())
        if albedo:
            attrs = surf.shade(rays, hits)
            _, rgba8 = dn.run_albedo(frame, n, hits, attrs, srgb=True)
            _, rgba8_t = dn.run_albedo(acc, 1, hits, attrs, srgb=True)
        else:
            _, rgba8 = dn.run(frame, n, hits, srgb=True)
            _, rgba8_t = dn.run(acc, 1, hits, srgb=True)
        dn.synchronize()
        S.write_image(paths[1], rgba8.cpu().numpy())
        S.write_image(paths[2], rgba8_t.cpu().numpy())
        if variance:
            _, rgba8_v, _ = dn.run_variance(acc, 1, hits, mom, srgb=True)
            dn.synchronize()
            S.write_image(paths[3], rgba8_v.cpu().numpy())
    return paths


if __name__ == "__main__":
    main()
