"""The two wave-per-point matchers (csrc/match_wave.inc: match_kernel = `match_legacy` 1, match_kernel2 = `match_legacy` 2) on search windows that need several
trips of their scan loops, against the oracle bit for bit: status, u, v, znssd with array_equal, obs exactly on OK records.

A trip hands 64 tasks to the wave.  match_kernel2's task is 8 positions of a window row: radius 12 = 25 x 4 = 100 tasks = 2 trips, radius 29 = 59 x 8 = 472 tasks
= 8 trips (the tested radii elsewhere, 4 ... 10, are one trip).  match_kernel's task is 4 positions: radius 29 = 59 x 15 = 885 tasks = 14 trips; it scores whenever
its list holds 64 hits and carries a shorter list into the next trip.  No list can overflow: a match_kernel2 trip offers at most 64 x 8 = 512 positions (CAND_CAP2),
a match_kernel trip adds at most 256 hits to fewer than 64 carried (320 slots).

One frame of 336 x 240 (level 2: 84 x 60), white noise, FAST at a low static threshold with ONE cell per level: cells of at least 84 x 60 pixels, so a window of
59 is narrower than a cell and option 2 really runs match_kernel2; windows hold dozens to hundreds of corners.  The setup and the oracle's answer are computed once
per radius and shared by the two kernels."""
import functools

import numpy as np
import pytest

W, H = 336, 240
FAST_THR = 5            # FastGrid::detect at a low static threshold: on white noise a third of the pixels are corners
DISP = 6.0
RADII = (12, 29)


def _cam():
    from scavislam_amd import synth
    return dict(synth.CAM_DEFAULT, w=W, h=H, cx=W / 2.0, cy=H / 2.0)


def _window_counts(corner_img, ui, vi, radius, pos_per_task):
    """(corners inside the searched part of the window, corners inside the positions of the wave's first 64 tasks) for a window centred on (ui, vi): rows and
    columns [6, size - 6) of the level (isInFrame(uv, 6); one cell covers the level), tasks in row-major order, `pos_per_task` positions each."""
    h, w = corner_img.shape
    side = 2 * radius + 1
    per_row = (side + pos_per_task - 1) // pos_per_task
    total = first = 0
    for wy in range(side):
        y = vi - radius + wy
        if y < 6 or y >= h - 6:
            continue
        x0, x1 = max(ui - radius, 6), min(ui + radius + 1, w - 6)
        if x1 <= x0:
            continue
        total += int(corner_img[y, x0:x1].sum())
        n_tasks = min(max(64 - wy * per_row, 0), per_row)                    # tasks of this row among the first 64
        xe = min(ui - radius + n_tasks * pos_per_task, ui + radius + 1, x1)
        if xe > x0:
            first += int(corner_img[y, x0:xe].sum())
    return total, first


@functools.lru_cache(maxsize=None)
def _case(radius):
    """Image, pyramid, the oracle's corners and trees, the anchors and the oracle's match records at `radius`; asserts that the windows hold what the test is about."""
    import oracle as O
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, level_cams
    cam = _cam()
    img = np.random.default_rng(41).integers(0, 256, (H, W)).astype(np.uint8)      # white noise: corners everywhere
    disp = np.full((H, W), DISP, np.float32)
    pyr = O.build_pyramid(img)
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    corners, trees, corner_imgs = [], [], []
    for l in range(3):
        h, w = pyr[l].shape
        g = O.fastgrid_for_level(w, h, l)
        g.gx = g.gy = 1
        g.cell_w, g.cell_h = w, h
        g.thr[0] = FAST_THR
        assert 2 * radius + 1 <= min(g.cell_w, g.cell_h), (l, radius)          # windows narrower than a cell: `match_legacy` 2 takes match_kernel2
        xy, cc = O.fastgrid_detect(g, pyr[l])
        corners.append((xy, cc))
        trees.append(O.quadtree_from_corners(xy, cc, w, h))
        ci = np.zeros((h, w), bool)
        ci[xy[:, 1], xy[:, 0]] = True
        corner_imgs.append(ci)
    # anchors ON corners under identity motion (the corner itself is the perfect match): per level the ones whose window hangs over the left, right, top and
    # bottom border, a sample of the rest, and the ones with the most corners in their window
    z = cam["f"] * cam["b"] / DISP
    rng = np.random.default_rng(19)
    rows, over = [], np.zeros(4, int)
    for l in range(3):
        xy = corners[l][0].astype(np.int64)
        h, w = pyr[l].shape
        s = 1 << l
        xy = xy[rng.permutation(len(xy))]
        dense = np.argsort([-_window_counts(corner_imgs[l], x, y, radius, 4)[0] for x, y in xy[:2000]], kind="stable")[:4]      # the fullest windows of a sample
        sel = [xy[xy[:, 0] < radius][:8], xy[xy[:, 0] >= w - radius][:8], xy[xy[:, 1] < radius][:8], xy[xy[:, 1] >= h - radius][:8], xy[:12], xy[dense]]
        over += [len(a) for a in sel[:4]]
        for ul, vl in np.concatenate(sel):
            r = np.zeros(1, CANDIDATE_DTYPE)
            u0, v0 = ul * s, vl * s
            r["xyz_anchor"] = ((u0 - cam["cx"]) / cam["f"] * z, (v0 - cam["cy"]) / cam["f"] * z, z)
            r["anchor_obs_pyr"] = (ul, vl, (u0 - DISP) / s)
            r["anchor_level"] = l
            rows.append(r)
    pts = np.concatenate(rows)
    assert (over >= 8).all(), over
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    ref = O.match([pyr], [I.reshape(12)], I, I, pyr, disp, trees, cams, pts, radius, thr_std=0)
    # what the searched windows hold, from the oracle's corners: every point that reaches the search (thr_std = 0: no texture gate) at its predicted position
    searched = np.isin(ref["status"], (0, 5, 6))                               # OK, NONE, NO_DISP
    assert searched.sum() >= 60, np.bincount(ref["status"])
    cnt = []
    for p in pts[searched]:
        ui, vi = int(p["anchor_obs_pyr"][0]), int(p["anchor_obs_pyr"][1])      # identity motion: the prediction is the anchor
        cnt.append(_window_counts(corner_imgs[int(p["anchor_level"])], ui, vi, radius, 4))      # (match_kernel's tasks: 4 positions)
    tot, first = np.array(cnt).T
    assert (tot > 64).any(), tot.max()                                         # more than one scoring round of 64 lanes
    assert (tot > 256).any(), tot.max()                                        # more hits than one match_kernel trip can add: hits carried from trip to trip
    if radius == 29:                                                           # `ncand < 64 && !last`: a first trip that ends short of 64 hits, with more to come
        assert ((first < 64) & (tot > 64)).any()
    return dict(cam=cam, img=img, disp=disp, pyr=pyr, corners=corners, pts=pts, ref=ref, max_hits=int(tot.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("legacy", [1, 2])
@pytest.mark.parametrize("radius", RADII)
def test_wave_matchers_many_scan_trips(gpu_ctx, radius, legacy):
    """match_kernel (1) and match_kernel2 (2) at radii 12 and 29 against the oracle on the same corners: every record's status, u, v, znssd, and obs of the OK ones."""
    from scavislam_amd.frontend import FastGrid, FramePyramid, GuidedMatcher, fastgrid_for_level
    ctx, stream = gpu_ctx
    c = _case(radius)
    fr = FramePyramid(ctx, stream, c["cam"], batch=1, with_float=False)
    fr.upload(c["img"][None], c["disp"][None])
    fr.preprocessing()
    grids = []
    for l in range(3):
        g = fastgrid_for_level(fr.w[l], fr.h[l], l)
        g.gx = g.gy = 1
        g.cell_w, g.cell_h = fr.w[l], fr.h[l]
        g.thr[0] = FAST_THR                                                    # (in the grid the handle is created from: it keeps no score below the lowest threshold it was given)
        assert 2 * radius + 1 <= min(g.cell_w, g.cell_h), (l, radius)
        grids.append(g)
    fg = FastGrid(ctx, fr, corner_cap=64 * 1024, grids=grids)
    fg.detect()                                                                # FastGrid::detect: one pass at the stored thresholds
    for l in range(3):                                                         # the device's corners are the oracle's: the trees of the reference hold what the bitmap holds
        xy, cc, et, ts = fg.corners(0, l)
        assert np.array_equal(xy, c["corners"][l][0]) and np.array_equal(cc, c["corners"][l][1]), l
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    gm = GuidedMatcher(ctx, fr, fg)
    ctx.set_option("match_legacy", legacy)
    try:
        res = gm.match([(fr.pyr, 0, I.reshape(12))], I.reshape(12), I.reshape(12), c["pts"], radius, thr_std=0)[0]
    finally:
        ctx.set_option("match_legacy", 0)
    fg.close()
    ref = c["ref"]
    ok = ref["status"] == 0
    print(f"radius {radius}, match_legacy {legacy}: {len(ref)} points, {int(ok.sum())} matched, up to {c['max_hits']} corners in a window")
    assert np.array_equal(res["status"], ref["status"])
    assert ok.sum() >= 60, np.bincount(ref["status"])
    assert np.array_equal(res["u"], ref["u"]) and np.array_equal(res["v"], ref["v"])
    assert np.array_equal(res["znssd"], ref["znssd"])
    assert np.array_equal(res["obs"][ok], ref["obs"][ok])
