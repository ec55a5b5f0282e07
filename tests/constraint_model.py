"""The pose graph's edges and their constraints, restated in NumPy / plain Python floats -- the yardstick of svs_map_add_edges .. svs_map_compute_constraints and
svs_ba_window_from_map_edges.

compute() is computeConstraint (slam_graph.cpp:787-846) in the operation order include/scavislam_hip.h states:
    common points   the points of kf1's feature_table that are also in kf2's, ascending
    anchor pose     an override of the request, else the map's pose if the anchor is in the window, else the request's cached pose, else MISSING
    depth           || pose_act(T1, pose_act(pose_inv(T_anchor), xyz)) ||, rows ((a0 b0 + a1 b1) + a2 b2) + t, sqrt((x x + y y) + z z)
    median          maths_utils.h:114-136;   T_12 = pose_mul(T1, pose_inv(T2));   norm_dist = || t(T_12) || / median
    info            diag(s a, s a, s a, s b, s b, s b), s = strength, a = Po2((350 * 1.0) * norm_dist), b = Po2(100 * 1.0)
Python floats are IEEE doubles without contraction; NumPy's f64 sqrt and / are correctly rounded.
EdgeTable is the reference's (slam_graph.hpp:197-363) with ONE stored pose T_lo_from_hi and ONE info; constraint_list() is copyContraintsToG2o (:937-981) in the
order the header states.  A map is a dict of flat tables as in ba_map_model: kf_ids, kf_poses [K][12]; point_ids, anchor_ids, xyz [N][3]; obs_point, obs_kf.
"""
import functools
import math

import numpy as np

from register_model import pose_inv, pose_mul

OK, EMPTY, MISSING_ANCHOR = 0, 1, 2
INNER, OUTER = 0, 1


def pose_act(T, x):
    """pose.h: ((t0 x0 + t1 x1) + t2 x2) + t3 per row"""
    T = [float(v) for v in np.asarray(T, np.float64).reshape(12)]
    x = [float(v) for v in x]
    return [T[4 * i] * x[0] + T[4 * i + 1] * x[1] + T[4 * i + 2] * x[2] + T[4 * i + 3] for i in range(3)]


def norm3(v):
    return float(np.sqrt(np.float64((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))


def median(values):
    """maths_utils.h:114-136 over a multiset: the iterator walks the sorted values"""
    s = sorted(float(v) for v in values)
    size = len(s)
    assert size > 0
    if size % 2 == 1:
        return s[size // 2]
    val = s[size // 2 - 1]
    val += s[size // 2]
    return 0.5 * val


def tables(m):
    """-> (feature_table {kf: set(points)}, pose {kf: [12]}, point {id: (anchor, xyz)})"""
    ft = {int(k): set() for k in m["kf_ids"]}
    for p, f in zip(m["obs_point"].tolist(), m["obs_kf"].tolist()):
        ft[f].add(p)
    pose = {int(k): [float(v) for v in T] for k, T in zip(m["kf_ids"], np.asarray(m["kf_poses"]).reshape(-1, 12))}
    point = {int(p): (int(a), [float(v) for v in x]) for p, a, x in zip(m["point_ids"], m["anchor_ids"], m["xyz"])}
    return ft, pose, point


def compute(m, window, kf1, kf2, overrides=(), cached=None, _tables=None):
    """-> dict(status, strength, n_missing, missing (every missing id, ascending), median, norm_dist, T_12 [12], info [36], depths (ascending point id))"""
    ft, pose, point = _tables or tables(m)
    window = set(int(k) for k in window)
    ov = {int(k): [float(v) for v in np.asarray(T, np.float64).reshape(12)] for k, T in overrides}
    cached = {int(k): [float(v) for v in np.asarray(T, np.float64).reshape(12)] for k, T in (cached or {}).items()}
    T1, T2 = ov.get(kf1, pose[kf1]), ov.get(kf2, pose[kf2])
    T_12 = pose_mul(T1, pose_inv(T2))
    common = sorted(ft[kf1] & ft[kf2])
    depths, missing = [], set()
    for p in common:
        a, xyz = point[p]
        if a in ov:
            Ta = ov[a]
        elif a in window:
            Ta = pose[a]
        elif a in cached:
            Ta = cached[a]
        else:
            missing.add(a)
            continue
        depths.append(norm3(pose_act(T1, pose_act(pose_inv(Ta), xyz))))
    out = dict(status=OK, strength=len(common), n_missing=len(missing), missing=np.array(sorted(missing), np.int32), median=0.0, norm_dist=0.0,
               T_12=np.array(T_12, np.float64), info=np.zeros(36), depths=np.zeros(0))
    if missing:
        out["status"] = MISSING_ANCHOR
        return out
    if not common:
        out["status"] = EMPTY
        return out
    med = median(depths)
    norm_dist = float(np.float64(norm3([T_12[3], T_12[7], T_12[11]])) / np.float64(med))
    s = float(len(common))
    v350, v100 = (350 * 1.0) * norm_dist, 100 * 1.0
    a, b = s * (v350 * v350), s * (v100 * v100)
    info = np.zeros((6, 6))
    info[[0, 1, 2], [0, 1, 2]] = a
    info[[3, 4, 5], [3, 4, 5]] = b
    out.update(median=med, norm_dist=norm_dist, info=info.reshape(36), depths=np.array(depths, np.float64))
    return out


def result_record(o):
    """the model's result as the library's MAP_CONSTRAINT_RESULT_DTYPE record"""
    from scavislam_amd.ctypes_types import MAP_CONSTRAINT_RESULT_DTYPE
    r = np.zeros(1, MAP_CONSTRAINT_RESULT_DTYPE)
    r["status"], r["strength"], r["n_missing"], r["median"], r["norm_dist"], r["T_12"], r["info"] = (o["status"], o["strength"], o["n_missing"], o["median"],
                                                                                                   o["norm_dist"], o["T_12"], o["info"])
    return r[0]


class EdgeTable:
    """slam_graph.hpp:197-363 with ONE pose (T_lo_from_hi) and ONE info per edge"""

    def __init__(self):
        self.e = {}

    @staticmethod
    def key(a, b):
        assert a != b
        return (min(a, b), max(a, b))

    def insert(self, id1, id2, strength, edge_type):
        k = self.key(id1, id2)
        assert k not in self.e
        self.e[k] = dict(strength=int(strength), edge_type=int(edge_type), is_marginalized=0, T=[0.0] * 12, info=np.zeros(36))

    def set_constraint(self, id1, id2, T_1_from_2, info):
        e = self.e[self.key(id1, id2)]
        e["T"] = [float(v) for v in T_1_from_2] if id1 < id2 else pose_inv(T_1_from_2)
        e["info"] = np.array(info, np.float64).reshape(36)
        e["is_marginalized"] = 1

    def un_marginalize(self, id1, id2):
        self.e[self.key(id1, id2)]["is_marginalized"] = 0

    def get_1_from_2(self, id1, id2):
        e = self.e[self.key(id1, id2)]
        return (e["T"] if id1 < id2 else pose_inv(e["T"])), e["info"], e["is_marginalized"]

    def record(self, id1, id2):
        from scavislam_amd.ctypes_types import MAP_EDGE_DTYPE
        k = self.key(id1, id2)
        e = self.e[k]
        r = np.zeros(1, MAP_EDGE_DTYPE)
        r["lo"], r["hi"], r["strength"], r["edge_type"], r["is_marginalized"], r["T_lo_from_hi"], r["info"] = (k[0], k[1], e["strength"], e["edge_type"],
                                                                                                               e["is_marginalized"], e["T"], e["info"])
        return r[0]


def constraint_list(window_ids, window_types, table, by_index=False):
    """copyContraintsToG2o in the header's order -> BA_CONSTRAINT_DTYPE (frame ids, or window indices) ; raises on an edge that is not marginalised (:972)"""
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE
    out = []
    ids = [int(k) for k in window_ids]
    for i, a in enumerate(ids):
        for j, b in enumerate(ids):
            if j == i or table.key(a, b) not in table.e or not (window_types[i] == OUTER or window_types[j] == OUTER):
                continue
            T_21, info, marg = table.get_1_from_2(b, a)
            if not marg:
                raise AssertionError("is_maginalized")
            c = np.zeros(1, BA_CONSTRAINT_DTYPE)
            c["T_21"], c["info"], c["pose1"], c["pose2"] = T_21, info, (i if by_index else a), (j if by_index else b)
            out.append(c[0])
    return np.array(out, BA_CONSTRAINT_DTYPE) if out else np.zeros(0, BA_CONSTRAINT_DTYPE)


# ---- the test map -----------------------------------------------------------------------------------------------------------------------------------------------
# keyframe i has id 100 + 3 i, point j id 5000 + 7 j (both cross bitmap words).  A pool of 1 500 points is seen by nested random subsets, so that the common-point
# count of two observers is the size of the smaller subset; every observer also has private points.  Three more keyframes share a row with tied depths.
POOL = 1500
OBSERVERS = dict(A=(0, 1500), B=(1, 1500), C=(2, 513), D=(3, 512), E=(4, 65), F=(5, 64), G=(6, 3), H=(7, 2), I=(8, 1), J=(9, 0))      # name: (keyframe index, pool share)
ANCHOR_KF = (0, 1, 10, 11, 12, 13, 14, 15)      # the pool's anchors: A, B and six keyframes that observe nothing
TIE_KF = dict(T=16, U=17, V=18)
N_KF = 19
WINDOW_SMALL = (0, 1, 2, 10, 11, 16)            # keyframe indices: with this window the anchors 12 .. 15 need a cached pose


def kf_id(i):
    return 100 + 3 * int(i)


@functools.lru_cache(maxsize=None)
def scene(seed=5):
    """-> dict(map, ids {name: keyframe id}, window_small, window_all).  Shared: treat it as read-only."""
    from scavislam_amd import synth
    rng = np.random.default_rng(seed)
    kf_ids = np.array([kf_id(i) for i in range(N_KF)], np.int32)
    poses = np.stack([synth.pose(synth.so3_exp(rng.normal(0, 0.15, 3)), rng.normal(0, 0.8, 3)).reshape(12) for _ in range(N_KF)])
    xyz, anchor, obs_p, obs_k = [], [], [], []
    # the pool
    order = rng.permutation(POOL)
    for j in range(POOL):
        xyz.append([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(2, 10)])
        anchor.append(ANCHOR_KF[rng.integers(len(ANCHOR_KF))])
    for name, (k, share) in OBSERVERS.items():
        for j in order[:share]:
            obs_p.append(int(j)); obs_k.append(k)
    # private points, anchored where they are seen
    for name, (k, share) in OBSERVERS.items():
        for _ in range(int(rng.integers(15, 40))):
            obs_p.append(len(xyz)); obs_k.append(k)
            xyz.append([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(2, 10)]); anchor.append(k)
    # the tied rows: anchored in T, whose pose is the identity (its inverse too, and x 1 + y 0 + z 0 + 0 = x), so with kf1 = T a point and its mirror image about
    # the camera centre have the same depth bit for bit.  20 + 15 small, 30 equal, 35 + 15 large; U sees 35 | 30 | 35 (both middle ranks inside the tie), V sees
    # 20 | 30 | 50 (the middle ranks straddle the tie's upper end), T sees all
    t = TIE_KF["T"]
    poses[t] = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
    unit = np.array([0.6, -0.48, 0.64])
    groups = [("small", 35, lambda: list(unit * rng.uniform(1.0, 2.0) + rng.normal(0, 0.05, 3))), ("equal", 30, None),
              ("large", 50, lambda: list(unit * rng.uniform(5.0, 9.0) + rng.normal(0, 0.05, 3)))]
    eq = list(unit * 3.25 + np.array([0.125, -0.0625, 0.03125]))
    for gname, count, draw in groups:
        for c in range(count):
            v = draw() if draw else [(-1.0) ** c * x for x in eq]
            p = len(xyz)
            xyz.append(v); anchor.append(t)
            sees = {"T"}
            if gname == "small":
                sees |= {"U"} | ({"V"} if c < 20 else set())
            elif gname == "equal":
                sees |= {"U", "V"}
            else:
                sees |= {"V"} | ({"U"} if c < 35 else set())
            for s in sorted(sees):
                obs_p.append(p); obs_k.append(TIE_KF[s])
    n = len(xyz)
    point_ids = (5000 + 7 * np.arange(n)).astype(np.int32)
    shuffle = rng.permutation(len(obs_p))
    m = dict(kf_ids=kf_ids, kf_poses=poses, point_ids=point_ids, anchor_ids=kf_ids[np.array(anchor)], xyz=np.array(xyz, np.float64),
             obs_point=point_ids[np.array(obs_p)][shuffle], obs_kf=kf_ids[np.array(obs_k)][shuffle])
    ids = {name: kf_id(k) for name, (k, _) in OBSERVERS.items()}
    ids.update({name: kf_id(k) for name, k in TIE_KF.items()})
    return dict(map=m, ids=ids, window_small=[kf_id(i) for i in WINDOW_SMALL], window_all=[int(k) for k in kf_ids],
                outside=[kf_id(i) for i in (12, 13, 14, 15)])
