"""Bundle-adjustment windows of hard landmark shapes for the Schur-kernel layout tests (tests/test_gpu_ba_layouts.py).

synth.ba_window (which bench.py uses) gives every landmark 2-8 observations anchored at its first observer.  The Schur kernel has
separate code for what that never produces, and this module produces it, rendered from ground truth as ba_window does:
  * track lengths 1, 2, 12, 13 (the DPP / recursive-doubling boundary of seg_allreduce, SEG_DPP_MAX = 12), 16, 17, 22, 23 (the pose spans
    of the small / big LDS window, WIN = 16 / WIN_BIG = 22), 31-33, 63, 64, and wide tracks of 65, 128 and P observations;
  * the anchor at the first, a middle or the last observer; a one-observation track is a landmark with only a self edge;
  * landmarks without any edge;
  * residuals from a small fraction of a pixel to tens of pixels, i.e. on both sides of every Huber delta the tests use;
  * 0, 1 or many pose-pose constraints, some between distant poses and some with pose1 > pose2;
  * optionally a bulk of ordinary 2-8-observation landmarks (vectorised) to reach a given number of wave chunks.
"""
import numpy as np

from scavislam_amd import synth
from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE, BA_EDGE_DTYPE

TRACKS = (1, 2, 12, 13, 16, 17, 22, 23, 31, 32, 33, 63, 64)


def _gt_poses(P):
    gt = []
    for i in range(P):
        R_wc = synth.so3_exp(np.array([0.0, 0.002 * i, 0.0]))
        c = np.array([0.3 * np.sin(0.05 * i), 0.0, 0.05 * i])
        gt.append(synth.pose_inv(synth.pose(R_wc, c)))
    return np.array(gt)


def _render(gt, cam, xw, poses, rng, noise):
    """stereo observations (u_l, v, u_r) of world points xw [n,3] from poses [n] plus per-edge noise [n] (pixels)"""
    R, t = gt[poses, :, :3], gt[poses, :, 3]
    y = np.einsum("nij,nj->ni", R, xw) + t
    assert (y[:, 2] > 1.0).all()
    f, cx, cy, b = cam["f"], cam["cx"], cam["cy"], cam["b"]
    obs = np.stack([f * y[:, 0] / y[:, 2] + cx, f * y[:, 1] / y[:, 2] + cy, f * (y[:, 0] - b) / y[:, 2] + cx], 1)
    return obs + rng.normal(0, 1, (len(poses), 3)) * noise[:, None]


def _landmark(gt, cam, anchor, rng):
    """ground-truth inverse-depth point in the anchor frame and its world position"""
    z = rng.uniform(8.0, 30.0)
    u0, v0 = rng.uniform(0.3 * cam["w"], 0.7 * cam["w"]), rng.uniform(0.3 * cam["h"], 0.7 * cam["h"])
    xa = np.array([(u0 - cam["cx"]) / cam["f"] * z, (v0 - cam["cy"]) / cam["f"] * z, z])
    Tw = synth.pose_inv(gt[anchor])
    return np.array([xa[0] / xa[2], xa[1] / xa[2], 1.0 / xa[2]]), Tw[:, :3] @ xa + Tw[:, 3]


def hard_window(P=130, seed=0, copies=2, n_empty=5, n_bulk=400, cam=synth.CAM_NEWCOLLEGE, wide=True):
    """A window with `copies` landmarks of every TRACKS length per anchor position (first, middle, last observer), the wide tracks
    65, 128 and P once per anchor position (wide=True), n_empty landmarks without edges and n_bulk ordinary landmarks.  Returns the
    dict of synth.ba_window (cons empty: see constraints()) plus "n_obs" per landmark."""
    rng = np.random.default_rng(seed)
    gt = _gt_poses(P)
    tracks = [(k, where) for k in TRACKS for where in ("first", "middle", "last") for _ in range(copies)]
    if wide:
        tracks += [(k, where) for k in (65, 128, P) if k <= P for where in ("first", "middle", "last")]
    rng.shuffle(tracks)
    pts, poses_e, anchors, psi_gt, xws = [], [], [], [], []
    for l, (k, where) in enumerate(tracks):
        first = int(rng.integers(0, P - k + 1))
        anchor = first if where == "first" else (first + k - 1 if where == "last" else first + k // 2)
        pg, xw = _landmark(gt, cam, anchor, rng)
        psi_gt.append(pg)
        for i in range(first, first + k):
            pts.append(l); poses_e.append(i); anchors.append(anchor); xws.append(xw)
    L_hard = len(tracks)
    # landmarks without edges
    for _ in range(n_empty):
        psi_gt.append(_landmark(gt, cam, int(rng.integers(0, P)), rng)[0])
    # bulk: 2-8 observations anchored at the first, vectorised
    if n_bulk:
        k = np.minimum(2 + rng.binomial(6, 0.5, n_bulk), P)
        first = (rng.random(n_bulk) * (P - k + 1)).astype(int)
        z = rng.uniform(8.0, 30.0, n_bulk)
        u0, v0 = rng.uniform(0.3 * cam["w"], 0.7 * cam["w"], n_bulk), rng.uniform(0.3 * cam["h"], 0.7 * cam["h"], n_bulk)
        xa = np.stack([(u0 - cam["cx"]) / cam["f"] * z, (v0 - cam["cy"]) / cam["f"] * z, z], 1)
        Tw = np.array([synth.pose_inv(T) for T in gt])[first]
        xw_b = np.einsum("nij,nj->ni", Tw[:, :, :3], xa) + Tw[:, :, 3]
        base = len(psi_gt)
        psi_gt.extend(np.stack([xa[:, 0] / xa[:, 2], xa[:, 1] / xa[:, 2], 1.0 / xa[:, 2]], 1))
        lm = np.repeat(np.arange(n_bulk), k)
        off = np.arange(len(lm)) - np.repeat(np.cumsum(k) - k, k)
        pts.extend(base + lm); poses_e.extend(first[lm] + off); anchors.extend(first[lm]); xws.extend(xw_b[lm])
    pts, poses_e, anchors, xws = np.array(pts), np.array(poses_e), np.array(anchors), np.array(xws)
    # residuals from 0.05 to 30 pixels (log-uniform): both sides of Huber deltas 0.3 .. 3 at every pyramid-level weight
    noise = np.exp(rng.uniform(np.log(0.05), np.log(30.0), len(pts)))
    obs = _render(gt, cam, xws, poses_e, rng, noise)
    lvl = rng.choice(3, len(pts), p=[0.6, 0.3, 0.1])
    s = 0.25 ** lvl
    e = np.zeros(len(pts), BA_EDGE_DTYPE)
    e["obs"], e["point"], e["pose"], e["anchor"] = obs, pts, poses_e, anchors
    e["info"] = np.stack([s, s, np.full(len(s), 0.333 ** 2)], 1)
    rng.shuffle(e)                                      # the reference iterates hash sets: any input order
    psi_gt = np.array(psi_gt)
    psi = psi_gt.copy()
    psi[:, 2] *= 1.0 + rng.normal(0, 0.02, len(psi))
    poses = []
    for T in gt:
        dx = np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, np.deg2rad(0.5), 3)])
        poses.append(synth.pose_mul(synth.pose(synth.so3_exp(dx[3:]), dx[:3]), T))
    n_obs = np.bincount(e["point"], minlength=len(psi))
    return dict(poses=np.array([T.reshape(12) for T in poses]), psi=psi, edges=e, cons=np.zeros(0, BA_CONSTRAINT_DTYPE), cam=cam,
                poses_gt=gt.reshape(-1, 12), psi_gt=psi_gt, n_obs=n_obs, L_hard=L_hard)


def constraints(prob, n, seed=0):
    """n pose-pose constraints on the window's ground truth with measurement noise: neighbours, distant pairs (loop-closure-like) and
    both orders of pose1 / pose2"""
    rng = np.random.default_rng(seed)
    gt = prob["poses_gt"].reshape(-1, 3, 4)
    P = len(gt)
    c = np.zeros(n, BA_CONSTRAINT_DTYPE)
    for j in range(n):
        i1 = int(rng.integers(0, P))
        i2 = (i1 + 1) % P if j % 3 == 0 else int(rng.integers(0, P))
        if i2 == i1:
            i2 = (i1 + 7) % P
        if j % 2:
            i1, i2 = max(i1, i2), min(i1, i2)       # pose1 > pose2: the transposed off-diagonal block
        T = synth.pose_mul(gt[i2], synth.pose_inv(gt[i1]))
        dn = np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.002, 3)])
        T = synth.pose_mul(synth.pose(synth.so3_exp(dn[3:]), dn[:3]), T)
        Lam = np.eye(6) * 30.0
        Lam[:3, :3] *= (350 * max(np.linalg.norm(T[:, 3]), 0.05) / 8.0) ** 2
        Lam[3:, 3:] *= 100.0 ** 2
        c[j]["T_21"], c[j]["info"], c[j]["pose1"], c[j]["pose2"] = T.reshape(12), Lam.reshape(36), i1, i2
    return c
