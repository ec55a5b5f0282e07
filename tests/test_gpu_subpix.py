"""svs_match_subpixel (scavislam_amd/csrc/match_subpix.inc) against its definition tests/subpix_model.py: the device's match records and svs_subpix_info records,
byte for byte.  The scenes are tests/subpix_cases.py's (64 x 48 on level 0; "big" is 128 x 96, where level 2 has pixels inside the matcher's margin); the match
records are hand-made, so the stateless call is tested without a matcher run.  tests/test_subpix_cpu.py checks on the CPU that the scenes hold what their names say."""
import ctypes as C

import numpy as np
import pytest

import subpix_cases as SC
import subpix_model as M

pytestmark = pytest.mark.gpu
SENTINEL = 0xAB


def _pad_to(s, want, info, n):
    """a scene's lists lengthened to n records with SVS_MATCH_NO_ANCHOR ones (streams of a batch share n_pts)"""
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, MATCH_RESULT_DTYPE
    k = n - len(s["res"])
    pp, rr = np.zeros(k, CANDIDATE_DTYPE), np.zeros(k, MATCH_RESULT_DTYPE)
    pp["kf_index"], rr["status"], rr["u"], rr["v"] = -1, 1, -12345, 1 << 30
    ii = np.zeros(k, M.INFO_DTYPE)
    ii["state"] = M.UNTOUCHED
    return np.concatenate([s["pts"], pp]), np.concatenate([s["res"], rr]), np.concatenate([want, rr]), np.concatenate([info, ii])


def run_device(ctx, stream, scenes, iterations, max_shift, eps, pad=0, strided=False, want_info=True, res_override=None):
    """The scenes as one batch through svs_match_subpixel.  pad: extra elements per image row, filled with 0xFF bytes; strided: kf / pts / out strides wider than
    the lists, the slack filled with SENTINEL bytes.  Returns (records [B][n], info [B][n] or None, slack bytes untouched)."""
    import torch
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, KEYFRAME_DTYPE, MATCH_RESULT_DTYPE, SubpixParams
    B, n = len(scenes), len(scenes[0][0])
    s0 = scenes[0][2]
    n_kf = len(s0["kf_T"])
    kf_b, pts_b, out_b = (n_kf + 1, n + 5, n + 3) if strided else (n_kf, n, n)
    keep = []

    def dev(a):
        with torch.cuda.stream(stream):
            t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
        keep.append(t)
        return t

    def padded(img):                                  # [h, w] -> device rows w + pad apart, the padding 0xFF bytes
        h, w = img.shape
        buf = np.full((h, (w + pad) * img.itemsize), 0xFF, np.uint8)
        buf[:, :w * img.itemsize] = np.ascontiguousarray(img).view(np.uint8).reshape(h, -1)
        return dev(buf)
    kfs = np.zeros((B, kf_b), KEYFRAME_DTYPE)
    pts = np.frombuffer(bytes([SENTINEL]) * (B * pts_b * 64), CANDIDATE_DTYPE).reshape(B, pts_b).copy()
    res = np.frombuffer(bytes([SENTINEL]) * (B * out_b * 64), MATCH_RESULT_DTYPE).reshape(B, out_b).copy()
    for b, (p, r, s) in enumerate(scenes):
        pts[b, :n], res[b, :n] = p, (r if res_override is None else res_override[b])
        for k in range(n_kf):
            kfs[b, k]["T_anchor_from_w"] = s["kf_T"][k]
            for l in range(3):
                t = padded(s["kf_pyr"][k][l])
                kfs[b, k]["pyr"][l], kfs[b, k]["stride"][l] = t.data_ptr(), s["kf_pyr"][k][l].shape[1] + pad
    a = capi.MatchArgs()
    # the current images and disparities of a batch lie a fixed stride apart: one buffer per level
    for l in range(3):
        h, w = s0["cur_pyr"][l].shape
        buf = np.full((B, h + 1, w + pad), 0xFF, np.uint8)
        for b, sc in enumerate(scenes):
            buf[b, :h, :w] = sc[2]["cur_pyr"][l]
        t = dev(buf)
        a.d_cur_pyr[l], a.cur_stride[l], a.cur_bstride[l] = t.data_ptr(), w + pad, (h + 1) * (w + pad)
        a.cam_vec[l] = s0["cams"][l]
    h, w = s0["disp"].shape
    dbuf = np.full((B, h + 2, (w + pad) * 4), 0xFF, np.uint8)
    for b, sc in enumerate(scenes):
        dbuf[b, :h, :w * 4] = np.ascontiguousarray(sc[2]["disp"]).view(np.uint8).reshape(h, -1)
    t = dev(dbuf)
    a.d_disp, a.disp_stride, a.disp_bstride = t.data_ptr(), w + pad, (h + 2) * (w + pad)
    d_kfs, d_pts, d_res = dev(kfs.view(np.uint8).reshape(-1)), dev(pts.view(np.uint8).reshape(-1)), dev(res.view(np.uint8).reshape(-1))
    d_T = dev(np.stack([sc[2]["T_cur_from_w"] for sc in scenes]))
    d_info = dev(np.full(B * out_b * 16, SENTINEL, np.uint8)) if want_info else None
    a.d_kfs, a.n_kf, a.d_pts, a.n_pts = d_kfs.data_ptr(), n_kf, d_pts.data_ptr(), n
    a.d_T_cur_from_w, a.d_T_w_from_actkey = d_T.data_ptr(), None
    a.search_radius, a.thr_mean, a.thr_std, a.n_batch = 8, 22, 10, B
    if strided:
        a.kf_bstride, a.pts_bstride, a.out_bstride = kf_b, pts_b, out_b
    else:
        a.kf_bstride = kf_b if B > 1 else 0
    prm = SubpixParams.default(iterations, max_shift, eps)
    stream.synchronize()
    ctx.call("svs_match_subpixel", C.byref(a), C.byref(prm), d_res.data_ptr(), d_info.data_ptr() if want_info else None)
    ctx.sync()
    got = d_res.cpu().numpy().view(MATCH_RESULT_DTYPE).reshape(B, out_b)
    info = d_info.cpu().numpy().view(M.INFO_DTYPE).reshape(B, out_b) if want_info else None
    slack_ok = bool((got[:, n:].view(np.uint8) == SENTINEL).all()) and (info is None or bool((info[:, n:].view(np.uint8) == SENTINEL).all()))
    return got[:, :n], (info[:, :n] if want_info else None), slack_ok


def _batch(names, params):
    """[(pts, res, scene)], wanted records, wanted info of the scenes as one batch"""
    sc = [SC.scene(nm) for nm in names]
    mod = [SC.model(nm, *params) for nm in names]
    n = max(len(s["res"]) for s in sc)
    packed = [_pad_to(s, m[0], m[1], n) for s, m in zip(sc, mod)]
    return [(p[0], p[1], s) for p, s in zip(packed, sc)], [p[2] for p in packed], [p[3] for p in packed]


def _assert_same(got, info, want, want_info, what):
    for b in range(len(want)):
        assert got[b].tobytes() == np.ascontiguousarray(want[b]).tobytes(), (what, b, "records", np.flatnonzero(got[b] != want[b])[:5])
        if info is not None:
            assert info[b].tobytes() == np.ascontiguousarray(want_info[b]).tobytes(), (what, b, "info", np.flatnonzero(info[b] != want_info[b])[:5])


@pytest.mark.parametrize("params", [(1, 1.5, 0.03), (8, 1.5, 0.03), (8, 1.5, 0.0)], ids=["it1", "it8", "it8-eps0"])
def test_mixed_batches(gpu_ctx, params):
    """Levels 0 .. 2, anchors in two keyframe slots, 20 degrees of roll and a 1.3 x depth change (key patches partly outside the keyframe), every other status mixed
    in: batch 1, and batch 3 with kf_bstride, pts_bstride and out_bstride set (the slack behind the lists stays as it was)."""
    ctx, stream = gpu_ctx
    for names, strided in ((["mixed0"], False), (["mixed0", "mixed1", "mixed2"], True)):
        scenes, want, want_info = _batch(names, params)
        got, info, slack = run_device(ctx, stream, scenes, *params, strided=strided)
        _assert_same(got, info, want, want_info, names)
        assert slack
    if params[0] == 8 and params[2] > 0:
        scenes, want, want_info = _batch(["big"], params)                      # level 2 inside the margin
        got, info, _ = run_device(ctx, stream, scenes, *params)
        _assert_same(got, info, want, want_info, "big")


@pytest.mark.parametrize("name", ["margin_lo", "margin_hi", "margin_l1"])
def test_margins_and_padded_strides(gpu_ctx, name):
    """Matches on the outermost admissible columns and rows with max_shift = 2 and the image moved so that p goes to the limit: taps on the image's first / last
    column and row.  Row strides wider than the images, padding 0xFF (disparity: NaN), give the same bytes as tight strides."""
    ctx, stream = gpu_ctx
    params = (8, 2.0, 0.03)
    scenes, want, want_info = _batch([name], params)
    got, info, _ = run_device(ctx, stream, scenes, *params)
    _assert_same(got, info, want, want_info, name)
    got_p, info_p, _ = run_device(ctx, stream, scenes, *params, pad=13)
    _assert_same(got_p, info_p, want, want_info, name + " padded")


def test_ok_record_outside_the_margin_is_shift(gpu_ctx):
    ctx, stream = gpu_ctx
    scenes, want, want_info = _batch(["u2"], (8, 1.5, 0.03))
    got, info, _ = run_device(ctx, stream, scenes, 8, 1.5, 0.03)
    _assert_same(got, info, want, want_info, "u2")
    assert list(info[0]["state"][:4]) == [M.SHIFT] * 4 and got[0][:4].tobytes() == scenes[0][1][:4].tobytes()      # u = 2, v = 3, u = W - 3, v = H - 3: untouched


def test_every_other_status_comes_back_untouched(gpu_ctx):
    """Statuses 1 .. 7 with u, v far outside the image and candidates that name no keyframe or level: the records byte for byte, the info UNTOUCHED."""
    ctx, stream = gpu_ctx
    scenes, _, _ = _batch(["mixed0"], (8, 1.5, 0.03))
    p, r, s = scenes[0]
    r = r.copy()
    r["status"] = 1 + np.arange(len(r)) % 7
    r["u"], r["v"] = 10**8, -10**8
    got, info, _ = run_device(ctx, stream, [(p, r, s)], 8, 1.5, 0.03, res_override=[r])
    assert got[0].tobytes() == r.tobytes()
    assert (info[0]["state"] == M.UNTOUCHED).all() and (info[0]["n_iter"] == 0).all() and (info[0]["dx"] == 0).all() and (info[0]["dy"] == 0).all()


@pytest.mark.parametrize("name, state", [("flat", M.SINGULAR), ("edge", M.SINGULAR), ("far", M.SHIFT)])
def test_singular_patches_and_far_displacement(gpu_ctx, name, state):
    """A constant key patch and a pure vertical edge (gy == 0, det == 0 exactly): SINGULAR, obs kept.  A current image displaced by 3 pixels: SHIFT, n_iter the model's."""
    ctx, stream = gpu_ctx
    scenes, want, want_info = _batch([name], (8, 1.5, 0.03))
    got, info, _ = run_device(ctx, stream, scenes, 8, 1.5, 0.03)
    _assert_same(got, info, want, want_info, name)
    assert (info[0]["state"] == state).all() and got[0].tobytes() == scenes[0][1].tobytes()
    assert name != "far" or (info[0]["n_iter"] >= 1).all()


def test_disparity_holes(gpu_ctx):
    """Disparity positive at (u, v) but 0, negative or NaN at the truncated refined position: SVS_MATCH_NO_DISP / NO_DISP, obs as it was."""
    ctx, stream = gpu_ctx
    scenes, want, want_info = _batch(["holes"], (8, 1.5, 0.03))
    got, info, _ = run_device(ctx, stream, scenes, 8, 1.5, 0.03)
    _assert_same(got, info, want, want_info, "holes")
    nd = info[0]["state"] == M.NO_DISP
    assert nd.sum() >= 6 and (got[0]["status"][nd] == 6).all() and got[0]["obs"][nd].tobytes() == scenes[0][1]["obs"][nd].tobytes()


def test_shapes_and_refusals(gpu_ctx):
    """n_pts = 0; one stream of 70 000 records (more than a grid dimension of 65 535); d_info = NULL; parameters refused before any launch."""
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import SubpixParams
    ctx, stream = gpu_ctx
    a = capi.MatchArgs()
    a.n_pts, a.n_batch = 0, 1
    ctx.call("svs_match_subpixel", C.byref(a), C.byref(SubpixParams.default()), None, None)      # nothing to do, nothing needed
    scenes, want, want_info = _batch(["mixed2"], (8, 1.5, 0.03))
    p, r, s = scenes[0]
    reps = -(-70000 // len(r))
    big = [(np.tile(p, reps)[:70000], np.tile(r, reps)[:70000], s)]
    got, info, _ = run_device(ctx, stream, big, 8, 1.5, 0.03)
    assert got[0].tobytes() == np.tile(want[0], reps)[:70000].tobytes() and info[0].tobytes() == np.tile(want_info[0], reps)[:70000].tobytes()
    got, info, _ = run_device(ctx, stream, scenes, 8, 1.5, 0.03, want_info=False)
    assert info is None
    _assert_same(got, None, want, want_info, "no info")
    for bad in (dict(max_shift=0.0), dict(max_shift=2.5), dict(iterations=0), dict(iterations=17), dict(eps=-1e-3), dict(max_shift=float("nan"))):
        prm = dict(iterations=8, max_shift=1.5, eps=0.03)
        prm.update(bad)
        with pytest.raises(capi.SvsError):
            run_device(ctx, stream, scenes, prm["iterations"], prm["max_shift"], prm["eps"])
    got, info, _ = run_device(ctx, stream, scenes, 8, 1.5, 0.03)                 # the context is as good as before
    _assert_same(got, info, want, want_info, "after the refusals")
