"""The definition of the matcher's sub-pixel refinement (svs_match_subpixel), in NumPy: what GuidedMatcher::subpixelAccuracy (matcher.cpp:241-309) would do if its
body were not behind `#if 0`, iterated, with a declared departure (the 2 x 2 solve is f64; the dead code solves with Eigen's f32 ldlt).

Every operation below is one IEEE operation of the stated format (NumPy does not contract): f64 for the warp of the key patch, the sums and the solve, f32 for the
gradients, the bilinear taps, the residual and the offset.  The device (scavislam_amd/csrc/match_subpix.inc on subpix_core.h) and the host build of subpix_core.h
(tests/cpp/subpix_host.cpp) are held to this file bit for bit.

    inv, key_uv      affine_inv(): the inverse of warpAffinve's local affine, formed as the matcher's prediction forms it (match_predict.inc)
    K[iy][ix]        key_patch(): the 10 x 10 warp (half size 5); K[1..8][1..8] is the matcher's KEY_PATCH
    refine_patch()   one record from its K, the current level image and the disparity image
    refine()         a batch of match records from the arguments svs_match took
"""
import numpy as np

REFINED, UNTOUCHED, SINGULAR, SHIFT, NO_DISP = range(5)
MATCH_OK, MATCH_NO_DISP = 0, 6
INFO_DTYPE = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("n_iter", "<i4"), ("state", "<i4")])
f32 = np.float32


def pose_mul(A, B):
    """pose.h: a row is (a0 b0 + a1 b1) + a2 b2, the translation added last"""
    A, B = [float(v) for v in np.asarray(A).reshape(12)], [float(v) for v in np.asarray(B).reshape(12)]
    out = [0.0] * 12
    for i in range(3):
        for j in range(4):
            out[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j]
        out[4 * i + 3] += A[4 * i + 3]
    return out


def pose_inv(A):
    A = [float(v) for v in np.asarray(A).reshape(12)]
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = A[4 * j + i]
    for i in range(3):
        out[4 * i + 3] = -(out[4 * i] * A[3] + out[4 * i + 1] * A[7] + out[4 * i + 2] * A[11])
    return out


def _warp_f(T, depth, cam, ku, kv):
    """d_warp_f (match_predict.inc): project(T * unproject(ku, kv, depth))"""
    f, cx, cy = float(cam.f), float(cam.cx), float(cam.cy)
    p = (depth * ((ku - cx) / f), depth * ((kv - cy) / f), depth * 1.0)
    q = [T[4 * r] * p[0] + T[4 * r + 1] * p[1] + T[4 * r + 2] * p[2] + T[4 * r + 3] for r in range(3)]
    return f * (q[0] / q[2]) + cx, f * (q[1] / q[2]) + cy


def affine_inv(T_cur_from_w, T_anchor_from_w, pt, cam):
    """inv[4] of the candidate `pt` (a CANDIDATE_DTYPE record) on its level's camera: matcher.cpp:113 and :411-426 in the matcher's operation order"""
    T = pose_mul(T_cur_from_w, pose_inv(T_anchor_from_w))
    ku, kv, depth = float(pt["anchor_obs_pyr"][0]), float(pt["anchor_obs_pyr"][1]), float(pt["xyz_anchor"][2])
    f0, fu, fv = _warp_f(T, depth, cam, ku + 0.0, kv + 0.0), _warp_f(T, depth, cam, ku + 1.0, kv + 0.0), _warp_f(T, depth, cam, ku + 0.0, kv + 1.0)
    a00, a01, a10, a11 = fu[0] - f0[0], fu[1] - f0[1], fv[0] - f0[0], fv[1] - f0[1]
    invdet = 1.0 / (a00 * a11 - a01 * a10)
    return a11 * invdet, -a01 * invdet, -a10 * invdet, a00 * invdet


def key_patch(inv, key_uv, kimg):
    """warpAffinve at half size 5 (matcher.cpp:403-458; key_pixel of match_wave.inc for all 100 pixels).  kimg: the keyframe's level image [H, W] (a view: a wider
    row stride does not show)."""
    H, W = kimg.shape
    K = np.zeros((10, 10), np.uint8)
    i00, i01, i10, i11 = (float(v) for v in inv)
    for iy in range(10):
        for ix in range(10):
            dx, dy = float(ix - 5), float(iy - 5)
            r0 = (i00 * dx + i01 * dy) + float(key_uv[0])
            r1 = (i10 * dx + i11 * dy) + float(key_uv[1])
            x, y = np.floor(r0), np.floor(r1)
            if not (x >= 0) or not (y >= 0) or x + 1 >= W or y + 1 >= H:
                continue
            sx, sy = r0 - x, r1 - y
            wx0, wx1, wy0, wy1 = 1 - sx, sx, 1 - sy, sy
            xi, yi = int(x), int(y)
            v00, v01, v10, v11 = float(kimg[yi, xi]), float(kimg[yi + 1, xi]), float(kimg[yi, xi + 1]), float(kimg[yi + 1, xi + 1])
            s = (wx0 * wy0) * v00 + (wx0 * wy1) * v01 + (wx1 * wy0) * v10 + (wx1 * wy1) * v11
            K[iy, ix] = int(s if s < 255.0 else 255.0)
    return K


def gradients(K):
    """cv::Sobel ksize 1, scale 0.5 on the 8 x 8 centre: f32 central differences"""
    Kf = K.astype(f32)
    return f32(0.5) * (Kf[1:9, 2:10] - Kf[1:9, 0:8]), f32(0.5) * (Kf[2:10, 1:9] - Kf[0:8, 1:9])


def normal_matrix(gx, gy):
    """H00, H01, H11, det in f64 (the sums are exact in any order)"""
    gxd, gyd = gx.astype(np.float64), gy.astype(np.float64)
    H00, H01, H11 = float((gxd * gxd).sum()), float((gxd * gyd).sum()), float((gyd * gyd).sum())
    return H00, H01, H11, H00 * H11 - H01 * H01


def current_patch(cimg, u, v, px, py):
    """warp2d at offset p (matcher.cpp:218-238 with interpolateMat_8u, maths_utils.cpp:67-86) in the reference's patch coordinates: f32 [8, 8]"""
    idx = np.arange(1, 9).astype(f32)
    xf, yf = f32(px) + idx, f32(py) + idx
    x0, y0 = np.floor(xf), np.floor(yf)
    sx, sy = (xf - x0)[None, :], (yf - y0)[:, None]
    col, row = (u - 5 + x0.astype(np.int64))[None, :], (v - 5 + y0.astype(np.int64))[:, None]
    assert col.min() >= 0 and row.min() >= 0 and col.max() + 1 < cimg.shape[1] and row.max() + 1 < cimg.shape[0], "a tap outside the image"
    wx0, wx1, wy0, wy1 = f32(1) - sx, sx, f32(1) - sy, sy
    v00, v01, v10, v11 = (cimg[row + a, col + b].astype(f32) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1)))
    return (wx0 * wy0) * v00 + (wx0 * wy1) * v01 + (wx1 * wy0) * v10 + (wx1 * wy1) * v11


def tree_sum(x):
    """64 doubles by a balanced tree over the index, adjacent pairs first"""
    x = np.asarray(x, np.float64).reshape(-1)
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return float(x[0])


def gn_step(K, gx, gy, H00, H01, H11, det, cimg, u, v, px, py):
    """(delta.x, delta.y) in f32, and the pieces (residual image, b0, b1)"""
    d = current_patch(cimg, u, v, px, py) - K[1:9, 1:9].astype(f32)
    b0 = tree_sum(gx.astype(np.float64) * d.astype(np.float64))
    b1 = tree_sum(gy.astype(np.float64) * d.astype(np.float64))
    dx = f32(-(H11 * b0 - H01 * b1) / det)
    dy = f32(-(H00 * b1 - H01 * b0) / det)
    return dx, dy, d, b0, b1


def refine_patch(K, cimg, disp, lvl, u, v, obs, iterations=8, max_shift=1.5, eps=0.03):
    """One SVS_MATCH_OK record.  cimg: current image of level lvl [H, W]; disp: level-0 disparity [H0, W0] f32.
    Returns (status, obs[3], info) -- status and obs as they are afterwards."""
    max_shift, eps = f32(max_shift), f32(eps)
    info = np.zeros((), INFO_DTYPE)
    obs = np.array(obs, np.float64)
    H, W = cimg.shape
    if not (u >= 6 and v >= 6 and u < W - 6 and v < H - 6):      # outside isInFrame(uv, 6): nothing is read
        info["state"] = SHIFT
        return MATCH_OK, obs, info
    gx, gy = gradients(K)
    H00, H01, H11, det = normal_matrix(gx, gy)
    if not det > 0:
        info["state"] = SINGULAR
        return MATCH_OK, obs, info
    px, py = f32(0), f32(0)
    for it in range(1, iterations + 1):
        dx, dy, _, _, _ = gn_step(K, gx, gy, H00, H01, H11, det, cimg, u, v, px, py)
        info["n_iter"] = it
        nx, ny = px + dx, py + dy
        if not (np.abs(nx) <= max_shift and np.abs(ny) <= max_shift):
            info["state"] = SHIFT
            return MATCH_OK, obs, info
        px, py = nx, ny
        if np.abs(dx) < eps and np.abs(dy) < eps:
            break
    info["dx"], info["dy"] = px, py
    nu, nv = f32(u) + px, f32(v) + py
    iu, iv = int(nu), int(nv)
    d = float(disp[iv << lvl, iu << lvl]) * (1.0 / float(1 << lvl))
    if not d > 0:
        info["state"] = NO_DISP
        return MATCH_NO_DISP, obs, info
    sc = float(1 << lvl)
    info["state"] = REFINED
    return MATCH_OK, np.array([float(nu) * sc, float(nv) * sc, (float(nu) - d) * sc]), info


def refine(res, pts, kf_T, kf_pyr, T_cur_from_w, cur_pyr, disp, cams, iterations=8, max_shift=1.5, eps=0.03):
    """One stream.  res: MATCH_RESULT_DTYPE [n]; pts: CANDIDATE_DTYPE [n]; kf_T[k]: T_anchor_from_w of keyframe slot k; kf_pyr[k][l], cur_pyr[l]: level images
    [H_l, W_l]; disp: [H_0, W_0] f32; cams[l]: f, cx, cy, w, h of level l.  Returns (records afterwards, INFO_DTYPE [n]); records that are not OK come back as
    they are and are read no further than their status."""
    out = res.copy()
    info = np.zeros(len(res), INFO_DTYPE)
    info["state"] = UNTOUCHED
    for i in np.flatnonzero(res["status"] == MATCH_OK):
        p = pts[i]
        l, k = int(p["anchor_level"]), int(p["kf_index"])
        inv = affine_inv(T_cur_from_w, kf_T[k], p, cams[l])
        K = key_patch(inv, p["anchor_obs_pyr"][:2], kf_pyr[k][l])
        st, obs, info[i] = refine_patch(K, cur_pyr[l], disp, l, int(res["u"][i]), int(res["v"][i]), res["obs"][i], iterations, max_shift, eps)
        out["status"][i], out["obs"][i] = st, obs
    return out, info
