"""match_kernel3 with its operands staged in the LDS, global loads and 24-bit offsets (match.hip): held to match_kernel (`match_legacy` 1) with array_equal on every
field of every stream, and one stream of every case to oracle.match, on the smallest inputs that reach each path of the kernel:

  frames     160 x 128 and 336 x 240 (row strides 192 / 128 / 64 and 384 / 192 / 128: padded on every level), three streams with three different frames -- two views
             of the synthetic scene and white noise -- each its own keyframe, so a wrong stream base or keyframe record shows;
  radii      8 (17 rows: the 17th-row path) and 4;
  points     every three consecutive points are of the three levels, and the non-OK statuses (no anchor, border, depth) stand between them inside the same waves;
             lists of 1, 15, 17 and 263 points (dead groups read record n_pts - 1);
  windows    anchors at each of the four borders (x0 < 0, rows below 6, past xhi / yhi) and at a cell-column boundary; FAST at the floor threshold (10) in every
             cell, so that windows hold more than 16 and more than 32 corners (the later trips of stage (5)) -- counted on the oracle's side, on the oracle's own
             corners, so the test cannot pass without them;
  order      xcd_swizzle 0 / 1, and 17 streams x 2 000 points, which reaches the 32 768-point bar of match_order_kernel;
  refusal    rows or strides that do not fit 24 bits are refused on the host, without a launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
FLOOR = 10                       # the lowest threshold a cell may hold (svs_fast_set_thresholds)
N_FULL = 250 + 13
_HOST = {}


def cam_of(w, h):
    return dict(f=570.342 * w / 640, cx=0.5 * w - 0.3125, cy=0.5 * h + 0.1875, b=0.075, w=w, h=h)


def _guess():
    """T_cur_from_actkey: the identity moved by about a pixel, so that the warp is no pure translation"""
    from scavislam_amd import synth
    return synth.pose(synth.so3_exp(np.array([0.002, -0.003, 0.004])), np.array([0.004, -0.003, 0.002]))


def _point(cam, disp, lvl, ul, vl, kf):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    s = 1 << lvl
    u0, v0 = int(ul) * s, int(vl) * s
    d = float(disp[v0, u0]) if disp[v0, u0] > 0.5 else 6.0
    z = cam["f"] * cam["b"] / d
    r = np.zeros(1, CANDIDATE_DTYPE)
    r["xyz_anchor"] = ((u0 - cam["cx"]) / cam["f"] * z, (v0 - cam["cy"]) / cam["f"] * z, z)
    r["anchor_obs_pyr"] = (ul, vl, (u0 - d) / s)
    r["anchor_level"] = lvl
    r["kf_index"] = kf
    return r


def host_case(w, h):
    """Everything of a frame size that does not need the device, made once: three frames, their pyramids, the oracle's corners at the floor threshold (and the
    trees over them), and the point list of every stream."""
    if (w, h) in _HOST:
        return _HOST[(w, h)]
    import oracle as O
    from scavislam_amd import synth
    cam = cam_of(w, h)
    sc, traj = synth.Scene(2011), synth.trajectory(8)
    rng = np.random.default_rng(100 + w)
    frames = [sc.render(cam, traj[5], seed=3), sc.render(cam, traj[2], seed=4),
              (rng.integers(0, 256, (h, w)).astype(np.uint8), np.full((h, w), 6.0, np.float32))]
    frames[1][1][h // 2:, : w // 3] = 0.0            # a region without disparity: SVS_MATCH_NO_DISP
    imgs, disps = [f[0] for f in frames], [f[1] for f in frames]
    pyrs = [O.build_pyramid(i) for i in imgs]
    grids, corners, trees = [], [], []
    for b in range(3):
        cb, tb = [], []
        for l in range(3):
            g = O.fastgrid_for_level(pyrs[b][l].shape[1], pyrs[b][l].shape[0], l)
            for c in range(g.gx * g.gy):
                g.thr[c] = FLOOR
            xy, cc = O.fastgrid_detect(g, pyrs[b][l])
            cb.append((xy, cc))
            tb.append(O.quadtree_from_corners(xy, cc, pyrs[b][l].shape[1], pyrs[b][l].shape[0]))
            if b == 0:
                grids.append(g)
        corners.append(cb)
        trees.append(tb)
    pts = []
    for b in range(3):
        per_level = []
        for l in range(3):
            wl, hl, g = w >> l, h >> l, grids[l]
            xy = corners[b][l][0].astype(np.int64)
            inner = xy[(xy[:, 0] >= 12) & (xy[:, 0] < wl - 12) & (xy[:, 1] >= 12) & (xy[:, 1] < hl - 12)]
            on_corners = inner[rng.permutation(len(inner))[:48]]            # anchors ON corners: the corner itself is the match
            ys, xs = rng.integers(8, hl - 8, 100), rng.integers(8, wl - 8, 100)
            edge = [(4 + k % 4, ys[k]) for k in range(6)] + [(wl - 5 - k % 4, ys[6 + k]) for k in range(6)] + \
                   [(xs[k], 4 + k % 4) for k in range(6)] + [(xs[6 + k], hl - 5 - k % 4) for k in range(6)] + \
                   [(g.cell_w * (1 + k % max(g.gx - 1, 1)) - 3 + k, ys[12 + k]) for k in range(6 if g.gx > 1 else 0)]
            anywhere = list(zip(xs[20:], ys[20:]))
            rows = [_point(cam, disps[b], l, u, v, b) for u, v in list(on_corners) + edge + anywhere]
            per_level.append(rows)
        # the three levels in turn, and a point of every non-OK status after every sixth of them: all inside the same waves
        n = min(len(r) for r in per_level)
        seq = []
        for k in range(n):
            for l in range(3):
                seq.append(per_level[l][k])
            if k % 2 == 1:
                bad = per_level[k % 3][k].copy()
                kind = (k // 2) % 4
                if kind == 0:
                    bad["kf_index"] = -1
                elif kind == 1:
                    bad["kf_index"] = 3
                elif kind == 2:
                    bad["anchor_obs_pyr"][0, :2] = (2.0, 2.0)
                else:
                    bad["xyz_anchor"] *= 2e-4 / bad["xyz_anchor"][0, 2]      # a point 0.2 mm away: the guess's translation changes its depth tenfold
                seq.append(bad)
        p = np.concatenate(seq)
        assert len(p) >= N_FULL, len(p)
        pts.append(p[:N_FULL])
    _HOST[(w, h)] = dict(cam=cam, imgs=imgs, disps=disps, pyrs=pyrs, grids=grids, corners=corners, trees=trees, pts=np.stack(pts), T=_guess())
    return _HOST[(w, h)]


def window_counts(H, b, radius, ref):
    """For the searched points of stream b (oracle status OK, NONE or NO_DISP: texture passed): the oracle's corners inside the window of radius - 1 about the
    predicted position (one pixel less than the kernel's: a bound from below that does not depend on how the prediction rounds), inside [6, w - 6) x [6, h - 6)"""
    from scavislam_amd.ctypes_types import level_cams
    cam, T = H["cam"], H["T"]
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    out = np.zeros(len(ref), np.int64)
    for k, p in enumerate(H["pts"][b][:len(ref)]):
        if ref["status"][k] not in (0, 5, 6):
            continue
        l = int(p["anchor_level"])
        q = T[:, :3] @ p["xyz_anchor"] + T[:, 3]
        u, v = cams[l].f * q[0] / q[2] + cams[l].cx, cams[l].f * q[1] / q[2] + cams[l].cy
        xy = H["corners"][b][l][0].astype(np.int64)
        wl, hl = cam["w"] >> l, cam["h"] >> l
        r = radius - 1
        out[k] = int(((np.abs(xy[:, 0] - int(u)) <= r) & (np.abs(xy[:, 1] - int(v)) <= r) & (xy[:, 0] >= 6) & (xy[:, 0] < wl - 6) & (xy[:, 1] >= 6) & (xy[:, 1] < hl - 6)).sum())
    return out


def border_windows(H, b, radius):
    """How many windows of stream b's list hang over each border or cross a cell-column boundary (from the anchors: the prediction lies within two pixels)"""
    n = dict(left=0, top=0, right=0, bottom=0, column=0)
    for p in H["pts"][b]:
        l = int(p["anchor_level"])
        wl, hl, g = H["cam"]["w"] >> l, H["cam"]["h"] >> l, H["grids"][l]
        u, v = p["anchor_obs_pyr"][0], p["anchor_obs_pyr"][1]
        n["left"] += u - radius < -2
        n["top"] += v - radius < 6 - 2
        n["right"] += u + radius >= wl - 6 + 2
        n["bottom"] += v + radius >= hl - 6 + 2
        n["column"] += any(u - radius + 2 < g.cell_w * c <= u + radius - 2 for c in range(1, g.gx))
    return n


def _device(ctx, stream, H, batch=3):
    """the frames on the device (stream s holds frame s % 3), FAST at the floor threshold, and the corners held to the oracle's"""
    from scavislam_amd.frontend import FastGrid, FramePyramid, GuidedMatcher
    fr = FramePyramid(ctx, stream, H["cam"], batch=batch, with_float=False)
    fr.upload(np.stack([H["imgs"][s % 3] for s in range(batch)]), np.stack([H["disps"][s % 3] for s in range(batch)]))
    fr.preprocessing()
    assert all(fr.stride[l] != fr.w[l] for l in range(3)), "row strides equal to the widths"
    fg = FastGrid(ctx, fr, corner_cap=64 * 1024)
    for s in range(batch):
        for l in range(3):
            fg.set_thresholds(s, l, [FLOOR] * (H["grids"][l].gx * H["grids"][l].gy))
    fg.detect()
    for s in range(min(batch, 3)):
        for l in range(3):
            xy, cc, _, _ = fg.corners(s, l)
            assert np.array_equal(xy, H["corners"][s][l][0]) and np.array_equal(cc, H["corners"][s][l][1]), (s, l)
    return fr, fg, GuidedMatcher(ctx, fr, fg)


def _run(ctx, gm, fr, H, pts, radius, legacy, swizzle=1):
    ctx.set_option("match_legacy", legacy)
    ctx.set_option("xcd_swizzle", swizzle)
    try:
        return gm.match([(fr.pyr, s, I34.reshape(12)) for s in range(3)], H["T"].reshape(12), I34.reshape(12), pts, radius)
    finally:
        ctx.set_option("match_legacy", 0)
        ctx.set_option("xcd_swizzle", 1)


def takes_kernel3(H, radius):
    """svs_match's own rule: windows narrower than a FAST cell on every level, and at most 17 rows"""
    return 2 * radius + 1 <= min(17, min(min(g.cell_w, g.cell_h) for g in H["grids"]))


def _oracle(H, b, pts, radius):
    import oracle as O
    from scavislam_amd.ctypes_types import level_cams
    cam = H["cam"]
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    return O.match(H["pyrs"], [I34.reshape(12)] * 3, H["T"], I34, H["pyrs"][b], H["disps"][b], H["trees"][b], cams, pts, radius)


def _same(res, ref, what):
    for k in ref.dtype.names:
        assert np.array_equal(res[k], ref[k]), (what, k, int((res[k] != ref[k]).sum()))


def _hold_to_oracle(res, ref, what):
    for k in ("status", "znssd"):
        assert np.array_equal(res[k], ref[k]), (what, k)
    found, ok = (ref["status"] == 0) | (ref["status"] == 6), ref["status"] == 0
    assert np.array_equal(res["u"][found], ref["u"][found]) and np.array_equal(res["v"][found], ref["v"][found]), what
    assert np.array_equal(res["obs"][ok], ref["obs"][ok]), what
    np.testing.assert_allclose(res["xyz_actkey"][found], ref["xyz_actkey"][found], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("radius", [8, 4])
@pytest.mark.parametrize("w,h", [(160, 128), (336, 240)])
def test_three_streams_every_window_kind(gpu_ctx, w, h, radius):
    ctx, stream = gpu_ctx
    H = host_case(w, h)
    # (160 x 128 has cells of 20 x 16 pixels on level 2: a window of radius 8 is wider, and the library takes match_kernel whatever the option says)
    assert takes_kernel3(H, radius) == ((w, h, radius) != (160, 128, 8))
    fr, fg, gm = _device(ctx, stream, H)
    res = _run(ctx, gm, fr, H, H["pts"], radius, 0)
    leg = _run(ctx, gm, fr, H, H["pts"], radius, 1)
    _same(res, leg, (w, h, radius))
    for b in range(3):
        ref = _oracle(H, b, H["pts"][b], radius)
        _hold_to_oracle(res[b], ref, (w, h, radius, b))
        st = set(np.unique(ref["status"]).tolist())
        assert st >= {0, 1, 2, 3}, (b, st)                         # OK, no anchor, border, depth in one list (texture, none, no disparity where the frame has them)
        assert (ref["status"] == 0).sum() >= 20, (b, np.bincount(ref["status"]))
        lv = H["pts"][b]["anchor_level"][ref["status"] == 0]
        assert set(lv.tolist()) == {0, 1, 2}, (b, "OK matches on every level")
        cnt = window_counts(H, b, radius, ref)
        nb = border_windows(H, b, radius)
        print((w, h, radius, b), "statuses", np.bincount(ref["status"], minlength=7).tolist(), "windows over 16 / 32 corners:", int((cnt > 16).sum()), int((cnt > 32).sum()), nb)
        assert all(v >= 3 for k, v in nb.items() if radius == 8 or k != "left"), nb      # (an anchor lies 4 columns inside the frame: radius 4 never reaches x0 < 0)
        assert (cnt > 16).sum() >= 5, (b, int(cnt.max()))          # the later trips of stage (5) ...
        if radius == 8:
            assert (cnt > 32).sum() >= 5, (b, int(cnt.max()))      # ... and a third trip (a window of radius 4 has 81 positions: none of these frames fills 33)
        if b == 1:
            assert 6 in st, "no match over the region without disparity"
    fg.close()


@pytest.mark.parametrize("n_pts", [1, 15, 17])
def test_short_lists(gpu_ctx, n_pts):
    ctx, stream = gpu_ctx
    H = host_case(336, 240)
    assert takes_kernel3(H, 8)
    fr, fg, gm = _device(ctx, stream, H)
    pts = np.ascontiguousarray(H["pts"][:, :n_pts])
    res, leg = _run(ctx, gm, fr, H, pts, 8, 0), _run(ctx, gm, fr, H, pts, 8, 1)
    _same(res, leg, n_pts)
    n_ok = 0
    for b in range(3):
        ref = _oracle(H, b, pts[b], 8)
        _hold_to_oracle(res[b], ref, (n_pts, b))
        n_ok += int((ref["status"] == 0).sum())
    assert n_ok >= 1, "no match in the short lists"
    fg.close()


@pytest.mark.parametrize("swizzle", [0, 1])
def test_block_order(gpu_ctx, swizzle):
    ctx, stream = gpu_ctx
    H = host_case(336, 240)
    assert takes_kernel3(H, 8)
    fr, fg, gm = _device(ctx, stream, H)
    res = _run(ctx, gm, fr, H, H["pts"], 8, 0, swizzle)
    for b in range(3):
        _hold_to_oracle(res[b], _oracle(H, b, H["pts"][b], 8), (swizzle, b))
    fg.close()


def test_ordered_run_of_17_streams(gpu_ctx):
    """17 x 2 000 points: above the bar from which svs_match sorts a stream's points by image cell first (match_order_kernel)"""
    ctx, stream = gpu_ctx
    H = host_case(336, 240)
    B, n = 17, 2000
    assert B * n >= 32768 and takes_kernel3(H, 8)
    fr, fg, gm = _device(ctx, stream, H, batch=B)
    rng = np.random.default_rng(5)
    pts = np.stack([H["pts"][s % 3][rng.integers(0, N_FULL, n)] for s in range(B)])      # (a stream's points name the keyframe of its frame: s % 3)
    res, leg = _run(ctx, gm, fr, H, pts, 8, 0), _run(ctx, gm, fr, H, pts, 8, 1)
    _same(res, leg, "ordered")
    ref = _oracle(H, 16 % 3, pts[16], 8)
    _hold_to_oracle(res[16], ref, "ordered, last stream")
    assert (ref["status"] == 0).sum() >= 20
    ctx.set_option("match_order", 0)
    try:
        _same(_run(ctx, gm, fr, H, pts, 8, 0), res, "list order")
    finally:
        ctx.set_option("match_order", 1)
    fg.close()


@pytest.mark.parametrize("field", ["cur_stride", "disp_stride", "rows", "n_pts"])
def test_sizes_beyond_24_bits_are_refused_on_the_host(gpu_ctx, field):
    """match_kernel3 forms its offsets with 24-bit multiplies: svs_match returns an error for such a call, whichever kernel it would have taken, before it allocates
    or launches anything (the output stays as it was)"""
    ctx, stream = gpu_ctx
    H = host_case(160, 128)
    fr, fg, gm = _device(ctx, stream, H)
    a = gm.prepare([(fr.pyr, s, I34.reshape(12)) for s in range(3)], H["T"].reshape(12), I34.reshape(12), H["pts"], 8)
    if field == "cur_stride":
        a.cur_stride[1] = 1 << 24
    elif field == "disp_stride":
        a.disp_stride = 1 << 24
    elif field == "rows":
        a.cam_vec[0].h = 1 << 24
    else:
        a.n_pts = 1 << 24
    gm._keep[4].fill_(0x5a)
    rc = ctx.lib.svs_match(ctx.h, C.byref(a), fg.h, gm._keep[4].data_ptr())
    ctx.sync()
    assert rc != 0, field
    assert bool((gm._keep[4] == 0x5a).all()), "the refused call wrote results"
    fg.close()
