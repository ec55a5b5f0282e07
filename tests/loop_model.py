"""NumPy restatement of the loop-closure geometric check (PlaceRecognizer::geometricCheck, placerecognizer.cpp:175-202): the yardstick of
tests/test_loop_cpu.py and tests/test_gpu_loop.py.  Written from the reference's text and from the header's (include/scavislam_hip.h, svs_loop_*), not from
the kernels:

  match()          cv::BFMatcher(NORM_L2).match: f64 squared distances on the differences, first minimum
  draw_triples()   the header's sample generator (splitmix64, mulhi32, the rejection structure of ransac.cpp:68-96, 64 draws)
  fit_svd()        getOrientationAndCentriods / SE3Model::calc_motion (ransac_models.cpp:44-81, :138-169) through numpy.linalg.svd
  fit_horn()       the same rotation from Horn's quaternion form (an independent second opinion)
  ransac()         RanSaC<SE3Model>::compute (ransac.cpp:28-137): scoring, first strict maximum from 0, the final pass, the identity quirk
  make_scene()     the seeded scenes of the GPU test
"""
import numpy as np

M64 = (1 << 64) - 1
MAX_DRAWS = 64
CAM = dict(f=500.0, cx=319.5, cy=239.5, b=0.12, w=640, h=480)


# ---- camera (stereo_camera.cpp:36-52; LinearCamera: map(p) = f p + c, unmap(uv) = (uv - c) / f) ---------------------------------------------------------
def unmap_uvu(cam, uvu):
    uvu = np.asarray(uvu, np.float64)
    sd = (uvu[..., 0] - uvu[..., 2]) / cam["b"]
    z = cam["f"] / sd
    return np.stack([((uvu[..., 0] - cam["cx"]) / cam["f"]) * z, ((uvu[..., 1] - cam["cy"]) / cam["f"]) * z, z], -1)


def map_uvu(cam, xyz):
    xyz = np.asarray(xyz, np.float64)
    with np.errstate(all="ignore"):
        u = cam["f"] * (xyz[..., 0] / xyz[..., 2]) + cam["cx"]
        v = cam["f"] * (xyz[..., 1] / xyz[..., 2]) + cam["cy"]
        ur = ((xyz[..., 0] - cam["b"]) / xyz[..., 2]) * cam["f"] + cam["cx"]
    return np.stack([u, v, ur], -1)


# ---- matching ------------------------------------------------------------------------------------------------------------------------------------------
def sqdist(q, t):
    """[N][M] f64 squared distances, formed on the differences"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    D = np.empty((len(q), len(t)))
    for i in range(len(q)):
        d = t - q[i]
        D[i] = np.einsum("jk,jk->j", d, d)
    return D


def match(q, t):
    """trainIdx (the lowest index of the minimum) and the distance matrix"""
    D = sqdist(q, t)
    return np.argmin(D, axis=1).astype(np.int32), D


def match_bound(q, t):
    """B_i = (K + 4) 2^-23 (|q_i|^2 + max_j |t_j|^2): bounds the error of a K-term f32 chain in either formulation"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    return (q.shape[1] + 4) * 2.0 ** -23 * ((q * q).sum(1) + (t * t).sum(1).max())


# ---- the sample generator (the header's text) --------------------------------------------------------------------------------------------------------------
def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, h, d, n):
    return ((splitmix64((seed ^ ((h << 32) | d)) & M64) >> 32) * n) >> 32


def draw_triple(seed, h, n, train_idx):
    """(r0, r1, r2) or None after 64 draws; every draw counts"""
    d = 0
    if n < 3:
        return None
    while d < MAX_DRAWS:
        r = []
        for i in range(3):
            while True:
                if d >= MAX_DRAWS:
                    return None
                x = draw(seed, h, d, n)
                d += 1
                if x not in r:
                    break
            r.append(x)
        t = [int(train_idx[x]) for x in r]
        if len(set(t)) == 3:
            return tuple(r)
    return None


def draw_triples(seed, n_hyp, n, train_idx):
    out = np.full((n_hyp, 3), -1, np.int32)
    for h in range(n_hyp):
        r = draw_triple(seed, h, n, train_idx)
        if r is not None:
            out[h] = r
    return out


def triple_valid(r, n, train_idx):
    r = [int(x) for x in r]
    return all(0 <= x < n for x in r) and len(set(r)) == 3 and len({int(train_idx[x]) for x in r}) == 3


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------------------
def _centre(p0, p1):
    c0 = (p0[0] + p0[1] + p0[2]) * (1.0 / 3.0)
    c1 = (p1[0] + p1[1] + p1[2]) * (1.0 / 3.0)
    return c0, c1, p0 - c0, p1 - c1


def fit_svd(p0, p1):
    """p0: the three query points (unmap_uvu of the observations), p1: the three train points.  [R | t] with R p1 + t ~ p0"""
    c0, c1, a, b = _centre(np.asarray(p0, np.float64), np.asarray(p1, np.float64))
    H = b.T @ a                                   # sum p1 p0^T
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    R = V @ U.T
    if np.linalg.det(R) < 0.0:
        V[:, 2] *= -1.0
        R = V @ U.T
    return np.hstack([R, (c0 - R @ c1)[:, None]])


def fit_horn(p0, p1):
    c0, c1, a, b = _centre(np.asarray(p0, np.float64), np.asarray(p1, np.float64))
    S = b.T @ a                                   # S[i][j] = sum p1[i] p0[j]
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.hstack([R, (c0 - R @ c1)[:, None]])


# ---- RANSAC ------------------------------------------------------------------------------------------------------------------------------------------------
def residuals(cam, T, xyz, uvu):
    """|uvu - map_uvu(T x)| per match and component; T [..., 3, 4]"""
    T = np.asarray(T, np.float64)
    X = np.einsum("...ij,nj->...ni", T[..., :3], xyz) + T[..., None, :, 3]
    return np.abs(uvu - map_uvu(cam, X))


def below(res, thr):
    with np.errstate(invalid="ignore"):
        return np.all(res * res < thr * thr, axis=-1)          # NaN / inf compare false


def ransac(cam, q_uvu, t_xyz, train_idx, samples, thr=2.5, fit=fit_svd):
    """samples [H][3] (an invalid triple, or -1 -1 -1, scores nothing).  Returns a dict: hyp_inliers [H], valid [H], best (-1: none), T [3][4], inlier [n],
    n_inliers, n_invalid, res [H][n][3] (NaN rows for invalid hypotheses), res_final [n][3]"""
    q_uvu, t_xyz = np.asarray(q_uvu, np.float64), np.asarray(t_xyz, np.float64)
    n, Hn = len(q_uvu), len(samples)
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    out = dict(hyp_inliers=np.zeros(Hn, np.int32), valid=np.zeros(Hn, bool), best=-1, T=I, inlier=np.zeros(n, bool), n_inliers=0, n_invalid=Hn,
               res=np.full((Hn, n, 3), np.nan), res_final=np.full((n, 3), np.nan), poses=np.full((Hn, 3, 4), np.nan))
    if n < 3:
        return out
    x = t_xyz[np.asarray(train_idx)]
    for h in range(Hn):
        if triple_valid(samples[h], n, train_idx):
            r = np.asarray(samples[h])
            out["valid"][h] = True
            out["poses"][h] = fit(unmap_uvu(cam, q_uvu[r]), t_xyz[np.asarray(train_idx)[r]])
    v = out["valid"]
    out["n_invalid"] = int((~v).sum())
    if v.any():
        out["res"][v] = residuals(cam, out["poses"][v], x, q_uvu)
        out["hyp_inliers"][v] = below(out["res"][v], thr).sum(1)
    bestinl = 0
    for h in range(Hn):
        if out["hyp_inliers"][h] > bestinl:
            bestinl, out["best"], out["T"] = int(out["hyp_inliers"][h]), h, out["poses"][h]
    out["res_final"] = residuals(cam, out["T"], x, q_uvu)
    out["inlier"] = below(out["res_final"], thr)
    out["n_inliers"] = int(out["inlier"].sum())
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------------------
def so3_exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def _unit_rows(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def make_scene(seed, N, M, K=64, inlier_frac=0.6, cam=CAM):
    """train points at z in [1.5, 6] m seen by the train camera; a planted T_query_from_train (|rotation| 0.09 rad, |translation| 0.5 m); round(inlier_frac N)
    queries are a train descriptor + 0.02 noise per component (renormalised) observed with 0.2 px noise (distinct train points while there are enough, which
    N > M makes impossible); the rest are random descriptors with random observations of positive disparity"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.5, 6.0, M)
    t_xyz_true = np.stack([(rng.uniform(40, cam["w"] - 40, M) - cam["cx"]) / cam["f"] * z, (rng.uniform(40, cam["h"] - 40, M) - cam["cy"]) / cam["f"] * z, z], 1)
    t_uvu = map_uvu(cam, t_xyz_true)
    t_desc = _unit_rows(rng.normal(size=(M, K))).astype(np.float32)
    ax = _unit_rows(rng.normal(size=(1, 3)))[0]
    T = np.hstack([so3_exp(0.09 * ax), (0.5 * _unit_rows(rng.normal(size=(1, 3)))[0])[:, None]])
    n_in = int(round(inlier_frac * N))
    src = rng.permutation(M)[:n_in] if n_in <= M else np.concatenate([rng.permutation(M), rng.integers(0, M, n_in - M)])
    q_desc = _unit_rows(rng.normal(size=(N, K)))
    q_uvu = np.empty((N, 3))
    u = rng.uniform(0, cam["w"], N)
    q_uvu[:] = np.stack([u, rng.uniform(0, cam["h"], N), u - rng.uniform(10.0, 40.0, N)], 1)
    q_desc[:n_in] = _unit_rows(t_desc[src].astype(np.float64) + rng.normal(0, 0.02, (n_in, K)))
    q_uvu[:n_in] = map_uvu(cam, t_xyz_true[src] @ T[:, :3].T + T[:, 3]) + rng.normal(0, 0.2, (n_in, 3))
    truth = np.full(N, -1, np.int32)
    truth[:n_in] = src
    p = rng.permutation(N)
    return dict(cam=cam, q_desc=np.ascontiguousarray(q_desc[p].astype(np.float32)), q_uvu=np.ascontiguousarray(q_uvu[p]), t_desc=t_desc, t_uvu=t_uvu,
                t_xyz=unmap_uvu(cam, t_uvu), T_true=T, truth=truth[p])
