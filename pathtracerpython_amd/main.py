#!/usr/bin/env python3
"""Command line mirror of the reference's main.py (main.py:125-139, :165-293).

    python -m pathtracerpython_amd.main objs/cornellroom.sdl --out out.png -r 1 -b 2

Same positional scene argument and flags (-r spp, -b bounces, --out,
--show-img); the whole spp x bounce loop runs on the GPU (render.py).  Extra
flags of this build: --seed (RNG key; default the SDL `seed`), --rr
(Russian roulette), --size W H (override the SDL size), --devices N (N GPUs:
one rank process per GPU, rows interleaved, one RCCL gather; launch.py),
--chunk-spp K [--checkpoint F] (the samples in launches of K, resumable from
F; progressive.py), --noise TOL [--min-spp N] [--step-spp K] [--save-aov P]
(adaptive sampling to the noise target TOL with -r as the per-pixel budget;
adaptive.py; with --checkpoint F the run resumes from F and writes it after
every pass), --denoise [--denoise-iters N] [--denoise-sigma S] (the
edge-avoiding filter on the device: --out / --save-raw get the filtered
frame; without --noise the -r samples go through the accumulator),
--local-devices N (N GPUs of this process, no rank processes: interleaved row
bands, also for --noise / --denoise; render.MultiRenderer), --aa
(antialiasing: a jittered primary ray per sample, PT_FLAG_AA; combines with
every flag above; scenes with a BVH keep the wavefront kernels), --aperture R
--focus-z Z (a thin-lens camera: a lens point per sample on a disc of radius R
around the eye, focused on the plane z = Z, PT_FLAG_LENS; the two go together;
with --aa, --noise, --denoise, --checkpoint, --chunk-spp and --local-devices,
not with --devices N > 1; always the single kernel), --look-at EX EY EZ TX
TY TZ [--up UX UY UZ] [--fov DEG] (a pinhole at E looking at T in place of the
scene's camera: cameras.look_at_rays through Renderer.render_rays,
pt_radiance, which takes the wavefront kernels on a scene with a BVH and the
single ray kernel otherwise; with -r, -b, --rr, --seed, --size, --out and
--save-raw; with --ray-accum also --noise, --denoise, --save-aov and
--checkpoint (with --noise): the frame then goes through an H x W ray
accumulator, Renderer.render_rays_adaptive, whose passes run the list kernel
over ray records; never with --aa, --aperture, --devices N > 1,
--local-devices or --chunk-spp).  The
reference's interactive 3-D viewer flags (--show-scene, --show-normals,
--show-screen, --show-inter -> plot.py) are accepted and ignored with a
notice: the pyqtgraph viewer is out of scope.
"""
import argparse
import sys

import numpy as np


def setup(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('scene', help='SDL scene')
    parser.add_argument('--out', help='Output image')
    parser.add_argument('-r', dest='n_rays', type=int, default=1, help='Number of rays per pixel')
    parser.add_argument('-b', dest='n_bounces', type=int, default=1, help='Number of bounces')
    parser.add_argument('--show-img', default=False, action='store_true')
    parser.add_argument('--show-scene', default=False, action='store_true')
    parser.add_argument('--show-normals', default=False, action='store_true')
    parser.add_argument('--show-screen', default=False, action='store_true')
    parser.add_argument('--show-inter', default=False, action='store_true')
    parser.add_argument('--seed', type=int, default=None, help='RNG key (default: SDL seed)')
    parser.add_argument('--rr', default=False, action='store_true', help='Russian roulette')
    parser.add_argument('--aa', default=False, action='store_true',
                        help='antialiasing: a jittered primary ray per sample (box filter one '
                             'pixel wide); the features and --denoise keep the centre ray')
    parser.add_argument('--aperture', type=float, default=None, metavar='R',
                        help='thin-lens camera: the radius of the lens disc around the eye '
                             '(with --focus-z); the features and --denoise keep the pinhole')
    parser.add_argument('--focus-z', type=float, default=None, metavar='Z',
                        help='with --aperture: the z of the plane in focus (the screen is z = 0)')
    parser.add_argument('--look-at', type=float, nargs=6, default=None,
                        metavar=('EX', 'EY', 'EZ', 'TX', 'TY', 'TZ'),
                        help='render through a pinhole at E looking at T instead of the scene\'s '
                             'camera (cameras.look_at_rays through Renderer.render_rays: the '
                             'wavefront kernels on a scene with a BVH, else the single ray kernel); with '
                             '-r, -b, --rr, --seed, --size, --out and --save-raw, and with --ray-accum '
                             'also --noise, --denoise, --save-aov and --checkpoint')
    parser.add_argument('--ray-accum', default=False, action='store_true',
                        help='with --look-at and --noise or --denoise: the frame through a ray accumulator '
                             '(Renderer.render_rays_adaptive); then also --save-aov and, with --noise, '
                             '--checkpoint')
    parser.add_argument('--up', type=float, nargs=3, default=None, metavar=('UX', 'UY', 'UZ'),
                        help='with --look-at: the direction towards the top of the image (default 0 1 0)')
    parser.add_argument('--fov', type=float, default=None, metavar='DEG',
                        help='with --look-at: the vertical field of view in degrees (default 40)')
    parser.add_argument('--size', type=int, nargs=2, metavar=('W', 'H'), default=None)
    parser.add_argument('--save-raw', default=None,
                        help='also save the float framebuffer (.npy, before normalisation)')
    parser.add_argument('--devices', type=int, default=1,
                        help='GPUs: one rank process each (torch.distributed over RCCL); '
                             'started here unless already under torch.distributed.run')
    parser.add_argument('--chunk-spp', type=int, default=None,
                        help='render the -r samples in launches of this many (progressive.py)')
    parser.add_argument('--checkpoint', default=None,
                        help='with --chunk-spp: .npz written after every chunk; with --noise: '
                             'the moments, written after every pass; a rerun resumes from it')
    parser.add_argument('--local-devices', type=int, default=None, metavar='N',
                        help='render on N GPUs of this process (row bands, no rank processes); '
                             'also with --noise / --denoise')
    parser.add_argument('--noise', type=float, default=None, metavar='TOL',
                        help='adaptive sampling: stop a pixel at this relative standard error; '
                             '-r becomes the per-pixel sample budget (adaptive.py)')
    parser.add_argument('--min-spp', type=int, default=8,
                        help='with --noise: samples every pixel gets at least')
    parser.add_argument('--step-spp', type=int, default=8,
                        help='with --noise: samples a pass adds per active pixel')
    parser.add_argument('--save-aov', default=None, metavar='PREFIX',
                        help='with --noise or --denoise: write PREFIX_counts.npy, _err.npy, '
                             '_obj.npy, _normal.npy, _point.npy, _var.npy (and _noisy.npy '
                             'with --denoise)')
    parser.add_argument('--denoise', default=False, action='store_true',
                        help='filter the frame on the device (variance- and first-hit-guided '
                             'a-trous filter); --out / --save-raw get the filtered frame')
    parser.add_argument('--denoise-iters', type=int, default=5,
                        help='with --denoise: iterations (stride 2^i), 1..8')
    parser.add_argument('--denoise-sigma', type=float, default=2.0,
                        help='with --denoise: the luminance stop in standard deviations')
    return parser.parse_args(argv)


def render_ranks(scene, args, W, H):
    """This rank's band (rows iy % world == rank) into a device tile, one
    RCCL gather to rank 0, the frame assembled there.  Returns (image array
    or None, f64 framebuffer) on rank 0, (None, None) elsewhere."""
    import torch
    import torch.distributed as dist
    from .distributed import assemble_bands_device, gather_tiles, max_band_rows
    from .launch import pg_timeout, rank_env
    from .render import Renderer, image_u8_device
    rank, local, world = rank_env()
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device("cuda", local), timeout=pg_timeout())
    ok = False
    try:
        with Renderer(scene) as r:
            p = r.params(W, H, args.n_rays, args.n_bounces, args.seed, args.rr, out_f64=True,
                         row_step=world, row_phase=rank, aa=args.aa)
            tile = torch.zeros((max_band_rows(H, world), W, 3), dtype=torch.float64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            r.render_device(p, tile.data_ptr(), s)
            tiles = gather_tiles(tile)
            if rank == 0:
                print(f'render: {W}x{H}, {args.n_rays} spp, {args.n_bounces} bounces on {world} '
                      f'GPUs, rank-0 kernel {r.last_kernel_ms():.3f} ms')
        if rank != 0:
            ok = True
            return None, None
        frame = assemble_bands_device(torch.stack(tiles),
                                      torch.empty((H, W, 3), dtype=torch.float64, device="cuda"))
        arr = None
        if W == H:
            img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
            image_u8_device(frame.data_ptr(), W, H, True, img.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
            arr = img.cpu().numpy()
        ok = True
        return arr, frame.cpu().numpy()
    finally:
        # the closing barrier only on success: after an error here the peers
        # may be blocked in the gather and would never reach it (the parent,
        # launch.spawn_ranks, stops them once this rank exits non-zero)
        if ok:
            dist.barrier()
        dist.destroy_process_group()


def check_args(args):
    """Reject flag combinations before any rank process starts."""
    if (args.aperture is None) != (args.focus_z is None):
        raise SystemExit('--aperture and --focus-z go together')
    if args.look_at is None and (args.up is not None or args.fov is not None):
        raise SystemExit('--up and --fov go with --look-at')
    if args.look_at is None and args.ray_accum:
        raise SystemExit('--ray-accum goes with --look-at')
    if args.look_at is not None:
        args.up = [0.0, 1.0, 0.0] if args.up is None else args.up
        args.fov = 40.0 if args.fov is None else args.fov
        # (a ray batch, or with --ray-accum a ray accumulator, lives on one device
        # in one process: no jitter, no lens, no sample chunks)
        for on, name in ((args.aa, '--aa'), (args.aperture is not None, '--aperture'),
                         (args.devices > 1, '--devices > 1'), (args.local_devices is not None, '--local-devices'),
                         (args.chunk_spp, '--chunk-spp')):
            if on:
                raise SystemExit(f'--look-at does not combine with {name}: it takes -r, -b, --rr, --seed, '
                                 '--size, --out and --save-raw, and with --ray-accum also --noise, --denoise, '
                                 '--save-aov and --checkpoint')
        if not args.ray_accum:
            # without the switch a look-at frame is one render_rays launch, as it
            # always was: what needs an accumulator is refused by name
            for on, name in ((args.noise is not None, '--noise'), (args.denoise, '--denoise'),
                             (args.checkpoint, '--checkpoint'), (args.save_aov, '--save-aov')):
                if on:
                    raise SystemExit(f'--look-at does not combine with {name} unless --ray-accum is given (the '
                                     'frame then goes through a ray accumulator); without it, it takes -r, -b, '
                                     '--rr, --seed, --size, --out and --save-raw')
        elif args.noise is None and not args.denoise:
            raise SystemExit('--look-at --ray-accum goes with --noise or --denoise')
        elif args.checkpoint and args.noise is None:
            raise SystemExit('--look-at takes --checkpoint with --noise only (the resumable adaptive run)')
        if not 0.0 < args.fov < 180.0:
            raise SystemExit('--fov: need 0 < DEG < 180')
    if args.aperture is not None and args.devices > 1:
        raise SystemExit('--aperture runs in one process (--devices 1; --local-devices N for more GPUs)')
    if args.local_devices is not None:
        if args.local_devices < 1:
            raise SystemExit('--local-devices must be >= 1')
        if args.devices > 1:
            raise SystemExit('--local-devices does not combine with --devices > 1 (rank processes)')
        if args.chunk_spp or args.checkpoint:
            raise SystemExit('--local-devices does not combine with --chunk-spp / --checkpoint')
    if args.checkpoint and not args.chunk_spp and args.noise is None:
        raise SystemExit('--checkpoint needs --chunk-spp')
    if args.chunk_spp and args.devices > 1:
        raise SystemExit('--chunk-spp runs on one device (--devices 1)')
    if args.denoise:
        if args.devices > 1:
            raise SystemExit('--denoise runs on one device (--devices 1)')
        if args.chunk_spp or (args.checkpoint and args.noise is None):
            raise SystemExit('--denoise does not combine with --chunk-spp / --checkpoint')
        if not 1 <= args.denoise_iters <= 8:
            raise SystemExit('--denoise-iters: need 1 <= iters <= 8')
        if not args.denoise_sigma > 0:
            raise SystemExit('--denoise-sigma must be > 0')
        if args.noise is None and args.n_rays < 2:
            raise SystemExit('--denoise needs -r >= 2 (the variance of one sample is unknown)')
    if args.noise is None:
        if args.save_aov and not args.denoise:
            raise SystemExit('--save-aov needs --noise or --denoise')
        return
    if args.chunk_spp:   # (--noise --checkpoint F alone: the resumable adaptive run)
        raise SystemExit('--noise does not combine with --chunk-spp / --checkpoint')
    if args.devices > 1:
        raise SystemExit('--noise runs on one device (--devices 1)')
    from .adaptive import check_rule
    try:
        check_rule(args.noise, args.n_rays, min(args.min_spp, args.n_rays), args.step_spp)
    except ValueError as e:
        raise SystemExit(f'--noise: {e} (-r is max_spp)')


def local_device_ids(n):
    """The devices of --local-devices n: 0..n-1, all of which must exist."""
    from ._native import device_count
    have = device_count()
    if n > have:
        raise SystemExit(f'--local-devices {n} but this process sees {have} GPU(s)')
    return list(range(n))


def lens_arg(args):
    """Renderer's lens of --aperture / --focus-z, or None."""
    return None if args.aperture is None else (args.aperture, args.focus_z)


def adaptive_args(args):
    """The render_adaptive arguments of --noise / --denoise."""
    dn = dict(iters=args.denoise_iters, sigma_l=args.denoise_sigma) if args.denoise else None
    if args.noise is not None:   # adaptive sampling
        return dict(tol=args.noise, min_spp=min(args.min_spp, args.n_rays), step_spp=args.step_spp,
                    denoise=dn, aa=args.aa)
    # --denoise alone: the uniform render, min_spp = max_spp = -r (also yields Q)
    return dict(tol=0.0, min_spp=args.n_rays, step_spp=args.n_rays, denoise=dn, aa=args.aa)


def main(argv=None):
    args = setup(argv)
    check_args(args)
    from .launch import rank_env, spawn_ranks, under_launcher
    if args.devices > 1 and not under_launcher():
        # one fresh process per GPU; this parent never touches the GPU
        raise SystemExit(spawn_ranks(args.devices, ['-m', 'pathtracerpython_amd.main'] +
                                     list(sys.argv[1:] if argv is None else argv)))
    from .render import Renderer
    from .scene_reader import Scene
    scene = Scene(args.scene)
    W, H = (args.size if args.size else (scene.width, scene.height))
    print(f'Number of objects: {len(scene.objects)}')
    print(f'Number of triangles: {sum(len(o["geometry"].triangles) for o in scene.objects)}')
    if args.show_scene or args.show_normals or args.show_screen or args.show_inter:
        print('note: the 3-D scene viewer (plot.py) is not part of this build; ignoring --show-*',
              file=sys.stderr)
    rank, _, world = rank_env()
    if world != args.devices:
        raise SystemExit(f'--devices {args.devices} but WORLD_SIZE={world}')
    if world > 1:
        arr, fb = render_ranks(scene, args, W, H)
        if rank != 0:
            return None
        return finish(args, arr, fb)
    if args.look_at is not None:
        return finish(args, None, render_look_at(scene, args, W, H))
    through_accum = args.noise is not None or args.denoise   # (adaptive.py)
    if args.local_devices is not None:   # N GPUs of this process (render.MultiRenderer)
        from .render import MultiRenderer, image_u8
        with MultiRenderer(scene, local_device_ids(args.local_devices), lens=lens_arg(args)) as m:
            if through_accum:
                res = m.render_adaptive(W, H, args.n_rays, args.n_bounces, args.seed, args.rr,
                                        **adaptive_args(args))
                fb = report_adaptive(args, res, W, H)
            else:
                fb = m.render(W, H, args.n_rays, args.n_bounces, args.seed, args.rr, out_f64=True,
                              aa=args.aa)
            arr = image_u8(fb) if W == H else None
        spp = f'up to {args.n_rays}' if args.noise is not None else f'{args.n_rays}'
        print(f'render: {W}x{H}, {spp} spp, {args.n_bounces} bounces on {args.local_devices} '
              f'local GPUs')
        return finish(args, arr, fb)
    with Renderer(scene, lens=lens_arg(args)) as r:   # (with a lens every render below goes through it)
        chunks = []
        if through_accum:
            from .render import image_u8
            ck = dict(checkpoint=args.checkpoint) if args.checkpoint else {}
            res = r.render_adaptive(W, H, args.n_rays, args.n_bounces, args.seed, args.rr,
                                    **adaptive_args(args), **ck)
            fb = report_adaptive(args, res, W, H)
            arr = image_u8(fb) if W == H else None
            chunks.append(res.samples)
        elif args.chunk_spp:   # chunked, resumable (progressive.py)
            from .progressive import render_progressive
            from .render import image_u8

            def progress(d, n):
                chunks.append(d)
                print(f'samples {d}/{n}', flush=True)
            fb = render_progressive(r, W, H, args.n_rays, args.n_bounces, args.seed, args.rr,
                                    chunk_spp=args.chunk_spp, checkpoint=args.checkpoint,
                                    on_chunk=progress, aa=args.aa)
            arr = image_u8(fb) if W == H else None
        elif W == H:   # make_image on the device (utils.py:150-161)
            arr, fb = r.render_image(W, H, spp=args.n_rays, bounces=args.n_bounces,
                                     seed=args.seed, rr=args.rr, return_fb=True, aa=args.aa)
        else:        # the reference's placement for W != H (utils.py:154-156), on the host
            fb = r.render(W, H, spp=args.n_rays, bounces=args.n_bounces, seed=args.seed,
                          rr=args.rr, aa=args.aa)
            arr = None
        last = f'kernel {r.last_kernel_ms():.3f} ms' if chunks or not args.chunk_spp \
            else 'all samples from the checkpoint'
        spp = f'up to {args.n_rays}' if args.noise is not None else f'{args.n_rays}'
        print(f'render: {W}x{H}, {spp} spp, {args.n_bounces} bounces, {last}')
    return finish(args, arr, fb)


def render_look_at(scene, args, W, H):
    """The f64 frame of --look-at: cameras.look_at_rays through
    Renderer.render_rays, the scene prepared for the eye point; with
    --ray-accum (and --noise or --denoise) through an H x W ray accumulator
    (Renderer.render_rays_adaptive on the rays in image order)."""
    from .cameras import look_at_rays, rays_to_image, to_image_order
    from .render import Renderer
    eye = args.look_at[:3]
    try:
        o, d, keys = look_at_rays(eye, args.look_at[3:], args.up, args.fov, W, H)
    except ValueError as e:
        raise SystemExit(f'--look-at: {e}')
    with Renderer(scene, ray_box=(eye, eye)) as r:
        if args.ray_accum:
            kw = adaptive_args(args)
            kw.pop('aa')
            dn = kw.pop('denoise')
            ck = dict(checkpoint=args.checkpoint) if args.checkpoint else {}
            res = r.render_rays_adaptive(*to_image_order(o, d, keys, W, H), shape=(H, W), max_spp=args.n_rays,
                                         bounces=args.n_bounces, seed=args.seed, rr=args.rr,
                                         denoise=dn is not None, **(dn or {}), **kw, **ck)
            fb = report_adaptive(args, res, W, H)
            spp = f'up to {args.n_rays}' if args.noise is not None else f'{args.n_rays}'
            print(f'render: {W}x{H} through --look-at, {spp} spp, {args.n_bounces} bounces, '
                  f'ray accumulator, last pass {r.last_kernel_ms():.3f} ms')
            return np.ascontiguousarray(fb)
        rgb = r.render_rays(o, d, keys, spp=args.n_rays, bounces=args.n_bounces, seed=args.seed, rr=args.rr)
        from ._abi import PATH_NAMES
        print(f'render: {W}x{H} through --look-at, {args.n_rays} spp, {args.n_bounces} bounces, '
              f'{PATH_NAMES[r.last_launch()["path"]]} path, kernel {r.last_kernel_ms():.3f} ms')
    return np.ascontiguousarray(rays_to_image(rgb, W, H))


def report_adaptive(args, res, W, H):
    """The lines and --save-aov files of a run through the accumulator; returns
    the frame --out / --save-raw get."""
    uniform = W * H * args.n_rays
    if args.noise is not None:
        print(f'adaptive: {len(res.passes)} passes, {res.samples} samples, '
              f'{res.samples / uniform:.3f} of the uniform budget ({uniform})')
    if args.denoise:
        print(f'denoise: {args.denoise_iters} iterations, sigma {args.denoise_sigma:g}')
    if args.save_aov:
        np.save(args.save_aov + '_counts.npy', res.counts)
        np.save(args.save_aov + '_err.npy', res.err)
        if args.denoise:
            feat = res.features
            np.save(args.save_aov + '_obj.npy', feat['obj'])
            np.save(args.save_aov + '_normal.npy', feat['N'])
            np.save(args.save_aov + '_point.npy', feat['P'])
            np.save(args.save_aov + '_var.npy', res.denoised_var)
            np.save(args.save_aov + '_noisy.npy', res.fb)
    return res.denoised if args.denoise else res.fb


def finish(args, arr, fb):
    """--save-raw / --out / --show-img of a rendered frame (rank 0)."""
    from .utils import framebuffer_to_image
    if args.save_raw:
        np.save(args.save_raw, fb)
    if arr is not None:
        from PIL import Image
        im = Image.fromarray(arr)
    else:
        im = framebuffer_to_image(fb)
    if args.out is not None:
        im.save(args.out)
    if args.show_img:
        im.show()
    return fb


if __name__ == '__main__':
    main()
