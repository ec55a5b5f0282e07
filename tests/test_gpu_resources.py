"""What contexts and handles hold (svs_ctx_get_stat: "live_device_bytes", "live_pinned_bytes", "live_sync_objects") goes back EXACTLY to the
readings taken before the case: after create / use / destroy of every handle at the smallest shape it accepts, and after a create that is refused
late.  The counters are process-wide and every allocation of the library goes through the owners that keep them (csrc/owned.h); torch's memory and the
caller's svs_malloc blocks are not counted.  Only argument-driven refusals are provoked, never an out-of-memory one."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("live_device_bytes", "live_pinned_bytes", "live_sync_objects")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SVS_ERR_INVALID, SVS_ERR_UNSUPPORTED = 1, 5


def live(ctx):
    return tuple(ctx.get_stat(n) for n in NAMES)


def baseline(ctx):
    gc.collect()      # wrappers other tests dropped without close() give their handles back now, not in the middle of the case
    ctx.sync()
    return live(ctx)


def small_cam(w, h):
    from scavislam_amd import synth
    return dict(synth.CAM_DEFAULT, w=w, h=h, cx=w / 2.0, cy=h / 2.0, f=synth.CAM_DEFAULT["f"] * w / 640.0)


def test_fast(gpu_ctx):
    from scavislam_amd import synth
    from scavislam_amd.frontend import FastGrid, FramePyramid
    ctx, stream = gpu_ctx
    w, h = 64, 48      # test_gpu_edge_cases.py::test_fast_small_image_and_capacity
    fr = FramePyramid(ctx, stream, dict(synth.CAM_DEFAULT, w=w, h=h, cx=32.0, cy=24.0), batch=1, with_float=False)
    fr.upload(synth.noise_image(w, h, 77)[None])
    fr.preprocessing()
    base = baseline(ctx)
    fg = FastGrid(ctx, fr)
    fg.detectAdaptively(trials=6)
    ctx.sync()
    assert live(ctx)[0] > base[0]
    fg.close()
    assert live(ctx) == base


def test_stereo(gpu_ctx):
    from scavislam_amd import synth
    from scavislam_amd.frontend import FramePyramid, StereoMatcher
    ctx, stream = gpu_ctx
    w, h = 64, 32
    img = synth.noise_image(w, h, 3)
    fr = FramePyramid(ctx, stream, small_cam(w, h), batch=1, with_float=False)
    fr.upload(img[None])
    base = baseline(ctx)
    sm = StereoMatcher(ctx, fr)
    sm.upload_right(np.roll(img, -4, axis=1)[None])
    sm.calcDisparityCpu()
    ctx.sync()
    assert live(ctx)[0] > base[0]
    sm.close()
    assert live(ctx) == base


def rectify_maps(w, h):
    """the identity map: every output pixel its own source pixel, no fraction"""
    xy = np.zeros((h, w, 2), np.int16)
    xy[..., 0], xy[..., 1] = np.arange(w)[None, :], np.arange(h)[:, None]
    return xy, np.zeros((h, w), np.uint16)


def test_rectify(gpu_ctx):
    from scavislam_amd.frontend import FrameGrabber
    ctx, _ = gpu_ctx
    w, h = 8, 4
    base = baseline(ctx)
    fg = FrameGrabber(ctx, small_cam(w, h), max_batch=1)
    fg.setMaps(rectify_maps(w, h), rectify_maps(w, h))
    assert live(ctx)[0] == base[0] + 2 * 4 * w * h      # two maps of one packed word per pixel
    fg.close()
    assert live(ctx) == base


def test_loop(gpu_ctx):
    from scavislam_amd.loop import GeometricChecker
    ctx, _ = gpu_ctx
    rng = np.random.default_rng(5)
    base = baseline(ctx)
    gcx = GeometricChecker(ctx, small_cam(640, 480), desc_dim=64, max_desc=8, max_places=2, max_hyp=4, max_checks=2)
    uvu = np.column_stack([rng.uniform(10, 600, 8), rng.uniform(10, 400, 8), rng.uniform(1, 9, 8)])
    uvu[:, 2] = uvu[:, 0] - uvu[:, 2]
    gcx.set_place(0, rng.standard_normal((8, 64)).astype(np.float32), uvu)
    ctx.sync()
    now = live(ctx)
    assert now[0] > base[0] and now[1] > base[1] and now[2] > base[2]
    gcx.close()
    assert live(ctx) == base


@pytest.mark.parametrize("n_streams,block_matching", [(1, False), (2, False), (1, True)])
def test_frontend(gpu_ctx, n_streams, block_matching):
    """one stream: the results live in one block (d_small | d_res | d_gated); two: in three blocks of their own"""
    import torch
    from scavislam_amd import capi, synth
    from scavislam_amd.frontend import StereoFrontend
    ctx, stream = gpu_ctx
    cam = small_cam(160, 128)      # the smallest of tests/test_gpu_frame_sizes.py
    sc = synth.Scene(2011)
    left, right, disp = synth.render_stereo(sc, cam, synth.trajectory(2)[1], seed=1)
    if n_streams > 1:
        with torch.cuda.stream(stream):
            d_left = torch.as_tensor(np.stack([left] * n_streams)).cuda()
            d_disp = torch.as_tensor(np.stack([disp] * n_streams).astype(np.float32)).cuda()
    base = baseline(ctx)
    fe = StereoFrontend(ctx, cam, max_points=64, max_keyframes=1, params=capi.FrontendParams.reference(use_block_matching=block_matching), n_streams=n_streams)
    if n_streams > 1:
        fe.processFirstFrames(d_left, disp=d_disp)
    elif block_matching:
        fe.processFirstFrame(left, right=right)
    else:
        fe.processFirstFrame(left, disp=disp)
    ctx.sync()
    now = live(ctx)
    assert now[0] > base[0] and now[1] > base[1] and now[2] > base[2]
    fe.close()
    assert live(ctx) == base


def test_ba(gpu_ctx):
    from scavislam_amd import synth
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams, Cam
    ctx, stream = gpu_ctx
    g = np.load(os.path.join(GOLD, "ba_small.npz"))
    cam = Cam(*[float(x) for x in g["cam"][:4]], int(g["cam"][4]), int(g["cam"][5]))
    edges, cons = g["edges"].view(synth.BA_EDGE_DTYPE).reshape(-1), g["cons"].view(synth.BA_CONSTRAINT_DTYPE).reshape(-1)
    base = baseline(ctx)
    opt = SlamGraphOptimizer(ctx, stream)
    opt.copyDataToG2o(g["poses"], g["psi"], edges, cons, cam, BaParams.reference_defaults())
    assert live(ctx)[0] > base[0]
    opt.optimize()      # (adds what the solve needs on first use: its profile, the control block, events)
    ctx.sync()
    first = live(ctx)
    opt.copyDataToG2o(g["poses"], g["psi"], edges, cons, cam, BaParams.reference_defaults())      # the same window again: every grow-only buffer is reused, none made again
    assert live(ctx) == first
    opt.close()
    assert live(ctx) == base


def test_second_context(gpu_ctx):
    from scavislam_amd import capi
    ctx, _ = gpu_ctx
    base = baseline(ctx)
    other = capi.Context(ctx.device)      # its own stream and two events
    assert live(ctx)[2] == base[2] + 3
    other.close()
    assert live(ctx) == base


def test_rectify_late_refusal_releases_the_left_map(gpu_ctx):
    ctx, _ = gpu_ctx
    w, h = 8, 4
    lxy, lfr = rectify_maps(w, h)
    rxy, rfr = rectify_maps(w, h)
    rfr[0, 0] = 1024      # a fraction word beyond 5 + 5 bits: found while the RIGHT map is packed, after the left one was uploaded
    base = baseline(ctx)
    out = C.c_void_p()
    rc = ctx.lib.svs_rectify_create(ctx.h, w, h, 1, lxy.ctypes.data, lfr.ctypes.data, rxy.ctypes.data, rfr.ctypes.data, C.byref(out))
    assert rc == SVS_ERR_INVALID and not out.value
    assert live(ctx) == base


def test_frontend_late_refusal_releases_everything(gpu_ctx):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import Cam
    ctx, _ = gpu_ctx
    cam = small_cam(160, 128)
    prm = capi.FrontendParams.reference(use_block_matching=True)
    prm.stereo.sad_window = 9      # refused by the block matcher, which the front end creates last
    base = baseline(ctx)
    out = C.c_void_p()
    rc = ctx.lib.svs_frontend_create_batch(ctx.h, C.byref(Cam(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])), C.byref(prm), 64, 1, 1, C.byref(out))
    assert rc == SVS_ERR_UNSUPPORTED and not out.value
    assert ctx.lib.svs_last_error(ctx.h).decode().startswith("svs_stereo: only SADWindowSize 7")
    assert live(ctx) == base
