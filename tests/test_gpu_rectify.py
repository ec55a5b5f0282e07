"""svs_rectify_frames / svs_depth_to_disp on the GPU, bit for bit against the NumPy model (tests/rectify_model.py), and through the front end:
frames rectified on the device into svs_frontend_input_view's buffers must give what host-rectified frames give."""
import functools

import numpy as np
import pytest

import rectify_model as RM

pytestmark = pytest.mark.gpu

CAMS = dict(RM.CAMERAS, **{"328x244": (328, 244, 270.0, 163.5, 121.5)})


@functools.lru_cache(maxsize=None)
def _maps(camera, lens):
    w, h, f, cx, cy = CAMS[camera]
    dist, rv = RM.LENS_SETS[lens]
    K = RM.intrinsics(f, cx, cy)
    return RM.build_maps(K, dist, RM.rodrigues(rv), K, w, h)


def _raw(B, w, h, ch, seed):
    """B distinct images with structure (a smooth ramp + blobs + noise), so neighbouring taps differ"""
    rng = np.random.default_rng(seed)
    shape = (B, h, w) if ch == 1 else (B, h, w, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (xx * 3 + yy * 5) % 256
    img = rng.integers(0, 256, shape, dtype=np.int64)
    img = (img + (base[None, :, :, None] if ch == 3 else base[None])) % 256
    return img.astype(np.uint8)


def _dev(stream, a, pad_cols=0, pad_rows=0):
    """host [B, h, w(, 3)] -> device tensor view of that shape inside a buffer whose rows are pad_cols pixels and whose streams pad_rows rows longer (filled with 0xEE)"""
    import torch
    B, h, w = a.shape[:3]
    with torch.cuda.stream(stream):
        buf = torch.full((B, h + pad_rows, w + pad_cols) + a.shape[3:], 0xEE, dtype=torch.uint8, device="cuda")
        v = buf[:, :h, :w]
        v.copy_(torch.as_tensor(a).cuda())
    return v


def _rectify(gpu_ctx, left, right, maps_l, maps_r, pad_in=0, pad_out=0, grabber=None):
    """-> (left_out [B, h, w], right_out or None) as numpy; checks that the padding of the outputs is untouched"""
    import torch
    from scavislam_amd.frontend import FrameGrabber
    ctx, stream = gpu_ctx
    B, h, w = left.shape[:3]
    g = grabber or FrameGrabber(ctx, dict(f=1.0, cx=0.0, cy=0.0, b=1.0, w=w, h=h), max_batch=B)
    if grabber is None:
        g.setMaps(maps_l, maps_r)
    dl = _dev(stream, left, pad_in, 1 if pad_in else 0)
    dr = _dev(stream, right, pad_in, 0) if right is not None else None
    so = w + pad_out
    with torch.cuda.stream(stream):
        ol = torch.full((B, h + (2 if pad_out else 0), so), 0xAB, dtype=torch.uint8, device="cuda")
        orr = torch.full((B, h, so), 0xAB, dtype=torch.uint8, device="cuda") if right is not None else None
    g.rectifyFrame(dl, ol, dr, orr)
    ctx.sync()
    if grabber is None:
        g.close()
    outs = []
    for o in (ol, orr):
        if o is None:
            outs.append(None)
            continue
        o = o.cpu().numpy()
        assert np.all(o[:, :h, w:] == 0xAB) and np.all(o[:, h:] == 0xAB), "wrote outside the w x h output"
        outs.append(o[:, :h, :w])
    return outs


def _model(raw, maps):
    return np.stack([RM.rectify(r, *(maps if maps is not None else (None, None))) for r in raw])


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("with_right", [True, False])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("camera,lens", [("640x480", "first"), ("512x384", "second"), ("328x244", "first")])
def test_rectify_equals_model(gpu_ctx, camera, lens, ch, with_right, pad):
    w, h = CAMS[camera][:2]
    ml, mr = _maps(camera, lens), _maps(camera, "second" if lens == "first" else "first")
    left = _raw(3, w, h, ch, 11)
    right = _raw(3, w, h, 1, 12) if with_right else None
    ol, orr = _rectify(gpu_ctx, left, right, ml, mr if with_right else None, pad_in=12 if pad else 0, pad_out=8 if pad else 0)
    assert np.array_equal(ol, _model(left, ml))
    if with_right:
        assert np.array_equal(orr, _model(right, mr))


def test_batches_of_1_3_40_give_every_stream_the_same_bits(gpu_ctx):
    from scavislam_amd.frontend import FrameGrabber
    ctx, _ = gpu_ctx
    w, h = CAMS["640x480"][:2]
    ml, mr = _maps("640x480", "first"), _maps("640x480", "second")
    left, right = _raw(40, w, h, 3, 21), _raw(40, w, h, 1, 22)
    g = FrameGrabber(ctx, dict(f=1.0, cx=0.0, cy=0.0, b=1.0, w=w, h=h), max_batch=40)
    g.setMaps(ml, mr)
    l40, r40 = _rectify(gpu_ctx, left, right, ml, mr, grabber=g)
    assert np.array_equal(l40, _model(left, ml)) and np.array_equal(r40, _model(right, mr))
    for b0, n in ((0, 1), (5, 1), (39, 1), (0, 3), (37, 3)):
        ln, rn = _rectify(gpu_ctx, left[b0:b0 + n], right[b0:b0 + n], ml, mr, grabber=g)
        assert np.array_equal(ln, l40[b0:b0 + n]) and np.array_equal(rn, r40[b0:b0 + n]), (b0, n)
    g.close()


def test_harsh_lens_with_taps_outside(gpu_ctx):
    w, h = CAMS["640x480"][:2]
    m = _maps("640x480", "harsh")
    n_in = RM.taps_inside(m[0], w, h).sum(axis=0)
    # the case must cover what it is here for (the model measured 23 %, 0.3 % and 2 %)
    assert (n_in == 0).mean() > 0.10, "more than 10 % of the pixels with all four taps outside"
    assert ((n_in > 0) & (n_in < 4)).sum() > 0, "pixels with one to three taps outside"
    assert (m[0] < 0).any(axis=-1).sum() > 0, "negative coordinates"
    print("harsh: all out %.3f, partly out %.4f, negative %.3f" % ((n_in == 0).mean(), ((n_in > 0) & (n_in < 4)).mean(), (m[0] < 0).any(axis=-1).mean()))
    for ch in (1, 3):
        left, right = _raw(2, w, h, ch, 31), _raw(2, w, h, 1, 32)
        ol, orr = _rectify(gpu_ctx, left, right, m, m)
        assert np.array_equal(ol, _model(left, m)) and np.array_equal(orr, _model(right, m))


def test_caller_made_maps_without_locality_and_at_the_extremes(gpu_ctx):
    w, h = CAMS["640x480"][:2]
    rng = np.random.default_rng(41)
    xy = np.stack([rng.integers(-3, w + 3, (h, w)), rng.integers(-3, h + 3, (h, w))], axis=-1).astype(np.int16)      # [-3, w + 2] x [-3, h + 2]
    fr = rng.integers(0, 1024, (h, w)).astype(np.uint16)
    # entries at -1, w - 1, h - 1, -32768 and 32767, in every combination, with full-range fractions
    ext_x, ext_y = [-1, w - 1, -32768, 32767, 0, w - 2], [-1, h - 1, -32768, 32767, 0, h - 2]
    k = 0
    for ex in ext_x:
        for ey in ext_y:
            for f in (0, 31, 31 * 32, 1023, 16 * 32 + 16):
                xy[k // w + 7, k % w] = (ex, ey)
                fr[k // w + 7, k % w] = f
                k += 1
    for ch in (1, 3):
        left, right = _raw(2, w, h, ch, 42), _raw(2, w, h, 1, 43)
        ol, orr = _rectify(gpu_ctx, left, right, (xy, fr), (xy[::-1].copy(), fr[::-1].copy()))
        assert np.array_equal(ol, _model(left, (xy, fr)))
        assert np.array_equal(orr, _model(right, (xy[::-1], fr[::-1])))


@pytest.mark.parametrize("ch", [1, 3])
def test_null_maps_convert_or_copy_only(gpu_ctx, ch):
    w, h = CAMS["512x384"][:2]
    left, right = _raw(3, w, h, ch, 51), _raw(3, w, h, 1, 52)
    ol, orr = _rectify(gpu_ctx, left, right, None, None, pad_in=4, pad_out=4)
    assert np.array_equal(ol, RM.bgr_to_gray(left) if ch == 3 else left) and np.array_equal(orr, right)
    # maps for one side only
    m = _maps("512x384", "second")
    ol, orr = _rectify(gpu_ctx, left, right, None, m)
    assert np.array_equal(ol, _model(left, None)) and np.array_equal(orr, _model(right, m))


def test_fraction_out_of_range_is_rejected_at_create(gpu_ctx):
    from scavislam_amd import capi
    from scavislam_amd.frontend import FrameGrabber
    ctx, _ = gpu_ctx
    w, h = CAMS["320x240"][:2]
    xy, fr = (a.copy() for a in _maps("320x240", "first"))
    fr[h // 2, w // 2] = 1024
    g = FrameGrabber(ctx, dict(f=1.0, cx=0.0, cy=0.0, b=1.0, w=w, h=h))
    with pytest.raises(capi.SvsError, match="status 1"):
        g.setMaps((xy, fr), None)
    with pytest.raises(capi.SvsError, match="status 1"):
        g.setMaps(None, (xy, fr))
    fr[h // 2, w // 2] = 1023
    g.setMaps((xy, fr), None)
    g.close()


@pytest.mark.parametrize("pad", [0, 6])
def test_depth_to_disp_over_all_depth_values(gpu_ctx, pad):
    import torch
    from scavislam_amd import synth
    from scavislam_amd.frontend import FrameGrabber
    ctx, stream = gpu_ctx
    cam = dict(synth.CAM_RGBD, w=256, h=128)
    B, h, w = 2, cam["h"], cam["w"]
    d16 = np.arange(65536, dtype=np.uint16).reshape(B, h, w)      # every value once, 0 included
    d16[1] = d16[1, ::-1, ::-1]
    g = FrameGrabber(ctx, cam, max_batch=B)
    with torch.cuda.stream(stream):
        src = torch.zeros((B, h, w + pad), dtype=torch.int16, device="cuda")
        src[:, :, :w] = torch.as_tensor(d16.view(np.int16)).cuda()
        dst = torch.full((B, h + 1, w + 2 * pad), -7.0, dtype=torch.float32, device="cuda")
    g.depthToDisp(src[:, :, :w], dst[:, :h, :w])
    ctx.sync()
    out = dst.cpu().numpy()
    want = RM.depth_to_disp(d16, cam["f"], cam["b"])
    assert np.isposinf(want[0, 0, 0]) and np.isfinite(want.reshape(-1)[1:65536]).all()
    assert np.array_equal(out[:, :h, :w].view(np.uint32), want.view(np.uint32))
    assert np.all(out[:, :h, w:] == -7.0) and np.all(out[:, h:] == -7.0)


# ---- through the front end ------------------------------------------------------------------------------------------------------------------------------
def _fe_streams(n, block_matching):
    """per stream three consecutive frames of the synthetic scene (keyframe, previous, current), taken as RAW frames of the first lens set"""
    from scavislam_amd import synth
    cam = synth.CAM_DEFAULT
    sc = synth.Scene(2011)
    traj = synth.trajectory(n + 3)
    out = []
    for b in range(n):
        fr = [synth.render_stereo(sc, cam, traj[b + i], seed=10 * b + i) if block_matching else sc.render(cam, traj[b + i], seed=10 * b + i) + (None,)
              for i in range(3)]
        fr = [(f[0], f[1], f[2]) if block_matching else (f[0], None, f[1]) for f in fr]      # (left, right, disp)
        rng = np.random.default_rng(7 + b)
        pts = synth.candidate_points(rng, cam, np.maximum(fr[0][2], 0), traj[b], (400, 200, 60))
        T_guess = synth.pose_mul(traj[b + 2], synth.pose_inv(traj[b + 1]))
        out.append(dict(fr=fr, pts=pts, n_new=150, T_guess=T_guess, T_kf=traj[b], T_act=traj[b + 1]))
    return cam, out


@pytest.mark.parametrize("n_streams,block_matching,colour", [(1, False, False), (8, False, True), (3, True, True)])
def test_device_rectified_frames_through_the_front_end(gpu_ctx, n_streams, block_matching, colour):
    """(a) rectified by the model on the host and fed the usual way == (b) rectified by svs_rectify_frames into svs_frontend_input_view, then in == NULL"""
    import torch
    from scavislam_amd import capi
    from scavislam_amd.frontend import FrameGrabber, StereoFrontend
    ctx, stream = gpu_ctx
    cam, S = _fe_streams(n_streams, block_matching)
    B, h, w = n_streams, cam["h"], cam["w"]
    dist, rv = RM.LENS_SETS["first"]
    dist_r, rv_r = RM.LENS_SETS["second"]
    K = RM.intrinsics(cam["f"], cam["cx"], cam["cy"])
    ml = RM.build_maps(K, dist, RM.rodrigues(rv), K, w, h)
    mr = RM.build_maps(K, dist_r, RM.rodrigues(rv_r), K, w, h) if block_matching else None
    prm = capi.FrontendParams.reference(use_block_matching=block_matching)
    Tg, Ta = np.stack([s["T_guess"].reshape(12) for s in S]), np.stack([s["T_act"].reshape(12) for s in S])

    def raw_left(i):
        g = np.stack([s["fr"][i][0] for s in S])
        return np.stack([g, g, g], axis=-1) if colour else g      # B = G = R: the gray value itself

    def run(device_rectifier):
        fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2, params=prm, n_streams=B)
        grab = FrameGrabber(ctx, cam, max_batch=B)
        if device_rectifier:
            grab.intializeRectifier(rv, dist, rv_r if block_matching else None, dist_r if block_matching else None)

        def frames(i):
            L = raw_left(i)
            R = np.stack([s["fr"][i][1] for s in S]) if block_matching else None
            D = None if block_matching else np.stack([s["fr"][i][2] for s in S]).astype(np.float32)
            if device_rectifier:
                (pl, sl, bl), (pr, sr, br), (pd, sd, bd) = fe.inputView()
                grab.rectifyFrame(_dev(stream, L, 8, 0), (pl, sl, bl), _dev(stream, R) if block_matching else None, (pr, sr, br) if block_matching else None)
                if not block_matching:
                    for b in range(B):
                        Dp = np.zeros((h, sd), np.float32); Dp[:, :w] = D[b]
                        ctx.call("svs_memcpy_h2d", pd + 4 * b * bd, Dp.ctypes.data, Dp.nbytes)
                return {}
            with torch.cuda.stream(stream):
                kw = dict(left=torch.as_tensor(_model(L, ml)).cuda(),
                          right=torch.as_tensor(_model(R, mr)).cuda() if block_matching else None,
                          disp=None if block_matching else torch.as_tensor(D).cuda())
            stream.synchronize()
            return kw

        fe.processFirstFrames(**frames(0))
        for b, s in enumerate(S):
            fe.keepKeyframe(0, s["T_kf"], stream=b)
        fe.processFirstFrames(**frames(1))
        for b, s in enumerate(S):
            fe.setCandidates(s["pts"], s["n_new"], stream=b)
        fe.processFrames(Tg, Ta, **frames(2))
        T_all, ok_all = fe.poses()
        res = [fe.results(b) for b in range(B)]
        fe.close(); grab.close()
        return T_all, ok_all, res

    assert all(np.array_equal(a, b) for a, b in zip(ml, FrameGrabber.build_maps(cam, rv, dist))), "the library's maps differ from the model's"
    Ta_h, ok_h, res_h = run(False)
    Ta_d, ok_d, res_d = run(True)
    assert np.array_equal(Ta_h, Ta_d) and np.array_equal(ok_h, ok_d)
    for b in range(B):
        (oh, mh, gh), (od, md, gd) = res_h[b], res_d[b]
        assert np.array_equal(np.array(oh.T_cur_from_actkey), np.array(od.T_cur_from_actkey)), f"pose of stream {b}"
        assert (oh.dense_passes, oh.n_points, oh.n_matched, oh.tracking_ok) == (od.dense_passes, od.n_points, od.n_matched, od.tracking_ok), f"svs_frame_result of stream {b}"
        assert bytes(oh.point_stats) == bytes(od.point_stats) and bytes(oh.pose_stats) == bytes(od.pose_stats), f"svs_frame_result of stream {b}"
        assert mh.tobytes() == md.tobytes(), f"match records of stream {b}"
        assert gh.tobytes() == gd.tobytes(), f"gated points of stream {b}"
        assert oh.n_points == len(S[b]["pts"])
        print("stream", b, "matched", oh.n_matched, "of", oh.n_points, "dense passes", oh.dense_passes, "tracking_ok", oh.tracking_ok)
