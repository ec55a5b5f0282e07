"""Scenes for the sub-pixel refinement's tests (tests/test_subpix_cpu.py, tests/test_gpu_subpix.py): a textured plane seen by two keyframes and a current camera,
rendered per pyramid level, with hand-made match records -- the stateless call needs no matcher run.  One scene = one stream; the model's answer is computed once
per (scene, parameters) and shared.

Cameras are dyadic (f = 64, cx = 32, cy = 24 on level 0, plane at depth 2): with identity poses the affine warp is the identity EXACTLY, so the singular and the
margin scenes do what their names say.

Roll: warpAffinve fills its matrix A by ROWS with the images of the two unit steps (matcher.cpp:416), which is the transpose of the warp's Jacobian; the matcher
reproduces that bit for bit.  Under an in-plane rotation the key patch is therefore turned the wrong way, and on the 20-degree scenes the refinement mostly ends in
SHIFT.  The tests hold the device to the model whatever the outcome; "mixed2" (2 degrees) is the scene on which most records are refined."""
import functools

import numpy as np

import subpix_model as M
from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, MATCH_RESULT_DTYPE, level_cams

Z0 = 2.0
I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)


def cams_for(w=64, h=48):
    return level_cams(float(w), w / 2.0, h / 2.0, 0.125, w, h)


def rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def pose(R, t):
    return np.hstack([R, np.asarray(t, float).reshape(3, 1)]).reshape(12)


def texture(seed, kind="waves"):
    """tex(X, Y, footprint) -> grey value; wavelengths of 12 .. 30 pixels of the level that is rendered (footprint = metres per pixel on the plane)"""
    rng = np.random.default_rng(seed)
    ang, lam, ph = rng.uniform(0, np.pi, 5), rng.uniform(12, 30, 5), rng.uniform(0, 2 * np.pi, 5)

    def tex(X, Y, fp):
        if kind == "flat":
            return np.full_like(X, 117.0)
        if kind == "edge":                                                     # a step in x
            return np.where(X > 0.05, 190.0, 60.0)
        v = sum(np.sin(2 * np.pi * (np.cos(a) * X + np.sin(a) * Y) / (l * fp) + p) for a, l, p in zip(ang, lam, ph))
        return 128.0 + 22.0 * v
    return tex


def _rays(T, cam):
    """per pixel: depth s along the camera's z of the plane Z_w = Z0, and the plane point"""
    T = np.asarray(T).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    ys, xs = np.mgrid[0:cam.h, 0:cam.w].astype(np.float64)
    d = np.stack([(xs - cam.cx) / cam.f, (ys - cam.cy) / cam.f, np.ones_like(xs)], -1)
    dw, tw = d @ R, R.T @ t                                                    # R^T d, R^T t
    s = (Z0 + tw[2]) / dw[..., 2]
    P = s[..., None] * dw - tw
    return s, P


def render(T, cam, tex):
    s, P = _rays(T, cam)
    return np.clip(np.rint(tex(P[..., 0], P[..., 1], Z0 / cam.f)), 0, 255).astype(np.uint8)


def make_scene(seed, T_cur, kf_T=None, n_per_level=(40, 30, 10), w=64, h=48, kind="waves", jitter=True, fixed_uv=None, n_bad=8):
    """One stream.  fixed_uv: {level: [(u, v), ...]} -- records at exactly these matches, anchored at the keyframe pixel that projects there under an identity
    relative pose (scenes with translation-only motion)."""
    rng = np.random.default_rng(seed)
    cams = cams_for(w, h)
    kf_T = [I34, pose(rot_z(-5.0), (0.05, -0.03, 0.1))] if kf_T is None else kf_T
    tex = texture(seed, kind)
    kf_pyr = [[render(T, cams[l], tex) for l in range(3)] for T in kf_T]
    cur_pyr = [render(T_cur, cams[l], tex) for l in range(3)]
    disp = np.full((h, w), 4.0, np.float32)
    Tc = np.asarray(T_cur).reshape(3, 4)
    pts, res = [], []
    for l in range(3):
        cam = cams[l]
        cand = []
        if fixed_uv is not None:
            cand = [(0, u, v, u, v) for u, v in fixed_uv.get(l, [])]
        else:
            tries = 0
            while tries < 40 * n_per_level[l]:
                tries += 1
                k = int(rng.integers(len(kf_T)))
                ku, kv = int(rng.integers(4, cam.w - 4)), int(rng.integers(4, cam.h - 4))
                cand.append((k, ku, kv, None, None))
        depth = [_rays(T, cam)[0] for T in kf_T]
        kept = 0
        for k, ku, kv, fu, fv in cand:
            Tk = np.asarray(kf_T[k]).reshape(3, 4)
            z = depth[k][kv, ku]
            xyz = z * np.array([(ku - cam.cx) / cam.f, (kv - cam.cy) / cam.f, 1.0])
            xc = Tc[:, :3] @ (Tk[:, :3].T @ (xyz - Tk[:, 3])) + Tc[:, 3]
            pu, pv = cam.f * xc[0] / xc[2] + cam.cx, cam.f * xc[1] / xc[2] + cam.cy
            if fu is None:
                fu, fv = int(np.rint(pu)), int(np.rint(pv))
                if jitter:
                    fu, fv = fu + int(rng.choice([-1, 0, 0, 0, 0, 0, 0, 1])), fv + int(rng.choice([-1, 0, 0, 0, 0, 0, 0, 1]))
                inside = 6 <= fu < cam.w - 6 and 6 <= fv < cam.h - 6
                if not inside and (l < 2 or cam.h > 12) and rng.random() < 0.9:      # most records inside the margin (a 16 x 12 level has no such pixel)
                    continue
                if not (0 <= fu < cam.w and 0 <= fv < cam.h) or kept >= n_per_level[l]:
                    continue
            kept += 1
            p = np.zeros((), CANDIDATE_DTYPE)
            p["xyz_anchor"], p["anchor_obs_pyr"] = xyz, (ku, kv, ku - 4.0 / (1 << l))
            p["anchor_level"], p["kf_index"], p["point_id"] = l, k, len(pts)
            r = np.zeros((), MATCH_RESULT_DTYPE)
            sc = float(1 << l)
            r["status"], r["u"], r["v"], r["znssd"] = 0, fu, fv, int(rng.integers(0, 30000))
            r["obs"] = (fu * sc, fv * sc, (fu - 4.0 / sc) * sc)
            r["xyz_actkey"] = rng.normal(size=3)
            pts.append(p)
            res.append(r)
    pts, res = np.array(pts, CANDIDATE_DTYPE), np.array(res, MATCH_RESULT_DTYPE)
    if n_bad:                                                                    # every other status, with positions far outside the image; never read beyond the status
        bp, br = np.zeros(n_bad, CANDIDATE_DTYPE), np.zeros(n_bad, MATCH_RESULT_DTYPE)
        bp["kf_index"], bp["anchor_level"] = rng.integers(-3, 9, n_bad), rng.integers(-2, 6, n_bad)
        br["status"] = 1 + np.arange(n_bad) % 7
        br["u"], br["v"] = rng.integers(-10**6, 10**6, n_bad), rng.integers(-10**6, 10**6, n_bad)
        br["obs"], br["xyz_actkey"], br["znssd"] = rng.normal(size=(n_bad, 3)), rng.normal(size=(n_bad, 3)), 0x7fffffff
        order = rng.permutation(len(pts) + n_bad)
        pts, res = np.concatenate([pts, bp])[order], np.concatenate([res, br])[order]
    return dict(cams=cams, kf_T=[np.asarray(T, np.float64).reshape(12) for T in kf_T], kf_pyr=kf_pyr, T_cur_from_w=np.asarray(T_cur, np.float64).reshape(12),
                cur_pyr=cur_pyr, disp=disp, pts=pts, res=res, w=w, h=h)


def shift_pose(px, py):
    """the current camera translated so that the level-0 image moves by (px, py) pixels (half of it on level 1): a match at the anchor's pixel is off by that much"""
    return pose(np.eye(3), (px * Z0 / 64.0, py * Z0 / 64.0, 0.0))


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "mixed0":       # 20 degrees roll, the camera moved back to 1.3 x the depth
        return make_scene(11, pose(rot_z(20.0), (0.02, -0.01, 0.3 * Z0)))
    if name == "mixed1":       # the other way: closer by 1.3, rolled back
        return make_scene(12, pose(rot_z(-20.0), (-0.03, 0.02, -0.23 * Z0)))
    if name == "mixed2":       # hardly any roll: the scene on which most records converge (see the module's note on roll)
        return make_scene(13, pose(rot_z(2.0), (0.0, 0.04, 0.15 * Z0)))
    if name == "big":          # 128 x 96: a level 2 of 32 x 24, on which records pass the margin
        return make_scene(14, pose(rot_z(-2.0), (0.02, -0.01, 0.2 * Z0)), n_per_level=(20, 20, 40), w=128, h=96)
    if name in ("margin_lo", "margin_hi"):      # matches on the first / last admissible column and row, the image moved 1.9 level pixels away from the border side
        sg = -1.0 if name == "margin_lo" else 1.0
        uv = {}
        for l in range(2):
            wl, hl = 64 >> l, 48 >> l
            e_u, e_v = (6, 6) if name == "margin_lo" else (wl - 7, hl - 7)
            uv[l] = [(e_u, v) for v in range(6, hl - 6, 3)] + [(u, e_v) for u in range(6, wl - 6, 3)] + [(e_u, e_v)]
        uv[2] = [(2, 6), (6, 5)]
        s = make_scene(21 + (sg > 0), shift_pose(1.9 * sg, 1.9 * sg), kf_T=[I34, I34], fixed_uv=uv, n_bad=0)
        return s
    if name == "margin_l1":    # the same for level 1: 1.9 level-1 pixels
        uv = {1: [(6, v) for v in range(6, 18, 2)] + [(u, 6) for u in range(6, 26, 2)]}
        return make_scene(23, shift_pose(-3.8, -3.8), kf_T=[I34, I34], fixed_uv=uv, n_bad=0)
    if name == "u2":           # an OK record inside the image but outside the matcher's margin
        return make_scene(24, shift_pose(0.3, 0.2), kf_T=[I34, I34], fixed_uv={0: [(2, 20), (20, 3), (61, 20), (20, 45), (20, 20)]}, n_bad=0)
    if name == "flat":
        return make_scene(31, shift_pose(0.3, 0.2), kf_T=[I34, I34], fixed_uv={0: [(20, 20), (30, 25)], 1: [(12, 10)]}, kind="flat", n_bad=0)
    if name == "edge":
        return make_scene(32, shift_pose(0.3, 0.0), kf_T=[I34, I34], fixed_uv={0: [(33, 20), (35, 25), (31, 12)], 1: [(16, 10)]}, kind="edge", n_bad=0)
    if name == "far":          # the current image displaced by 3 pixels
        return make_scene(33, shift_pose(3.0, 0.0), kf_T=[I34, I34], fixed_uv={0: [(u, v) for u in range(10, 50, 8) for v in range(10, 40, 8)]}, n_bad=0)
    if name == "holes":        # moved by (-0.6, -0.4): the truncated refined position is the pixel up and left of the match
        s = dict(make_scene(34, shift_pose(-0.6, -0.4), kf_T=[I34, I34], fixed_uv={0: [(u, v) for u in range(10, 54, 6) for v in range(10, 40, 6)],
                                                                                 1: [(u, v) for u in range(8, 24, 4) for v in range(8, 16, 4)]}, n_bad=0))
        full, info = model("holes_full")
        disp = s["disp"].copy()
        k = 0
        for r, i in zip(s["res"], info):
            l = int(s["pts"][r_index(s, r)]["anchor_level"])
            iu, iv = int(np.float32(r["u"]) + i["dx"]), int(np.float32(r["v"]) + i["dy"])
            if i["state"] == M.REFINED and (iu, iv) != (int(r["u"]), int(r["v"])) and k < 9:
                disp[iv << l, iu << l] = (0.0, -1.0, np.nan)[k % 3]
                k += 1
        s["disp"], s["n_holes"] = disp, k
        for r in s["res"]:      # no hole at a match itself
            l = int(s["pts"][r_index(s, r)]["anchor_level"])
            assert disp[int(r["v"]) << l, int(r["u"]) << l] > 0
        return s
    if name == "holes_full":
        return make_scene(34, shift_pose(-0.6, -0.4), kf_T=[I34, I34], fixed_uv={0: [(u, v) for u in range(10, 54, 6) for v in range(10, 40, 6)],
                                                                               1: [(u, v) for u in range(8, 24, 4) for v in range(8, 16, 4)]}, n_bad=0)
    raise KeyError(name)


def r_index(s, r):
    return int(np.flatnonzero((s["res"]["u"] == r["u"]) & (s["res"]["v"] == r["v"]) & (s["res"]["znssd"] == r["znssd"]))[0])


@functools.lru_cache(maxsize=None)
def model(name, iterations=8, max_shift=1.5, eps=0.03):
    """(records afterwards, info) of scene `name` by tests/subpix_model.py"""
    s = scene(name)
    return M.refine(s["res"], s["pts"], s["kf_T"], s["kf_pyr"], s["T_cur_from_w"], s["cur_pyr"], s["disp"], s["cams"], iterations, max_shift, eps)


# (scene, iterations, max_shift, eps): what the GPU tests run, and what the host build of subpix_core.h is held to on the CPU
GPU_CASES = [("mixed0", 1, 1.5, 0.03), ("mixed0", 8, 1.5, 0.03), ("mixed0", 8, 1.5, 0.0), ("mixed1", 8, 1.5, 0.03), ("mixed2", 8, 1.5, 0.03), ("mixed1", 1, 1.5, 0.03),
             ("mixed2", 8, 1.5, 0.0), ("big", 8, 1.5, 0.03), ("big", 1, 1.5, 0.0), ("margin_lo", 8, 2.0, 0.03), ("margin_hi", 8, 2.0, 0.03), ("margin_l1", 8, 2.0, 0.03),
             ("u2", 8, 1.5, 0.03), ("flat", 8, 1.5, 0.03), ("edge", 8, 1.5, 0.03), ("far", 8, 1.5, 0.03), ("holes", 8, 1.5, 0.03)]
