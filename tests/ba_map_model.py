"""The double window's BA problem built from the back end's map, restated in NumPy -- the yardstick of svs_map_prepare_window / svs_ba_window_from_map /
svs_ba_store_to_map.

A map is a dict of flat tables (scene() makes one): kf_ids, kf_poses [K][12]; point_ids, anchor_ids, xyz [N][3]; obs_point, obs_kf, obs_center [M][3], obs_level.
prepare() applies the rules of include/scavislam_hip.h (computeActivePointsAndExtendOuterWindow, slam_graph.cpp:599-663, as set operations):
    1. p is active iff some INNER keyframe F of W0 has p in its feature_table and either anchor(p) is in W0 or (F, anchor(p)) is among the pairs (symmetric)
    2. extension = the anchors of active points that are not in W0, typed OUTER
    3. final window = W0 in the caller's order, then the extension ascending
    4. active list ascending
problem() is copyDataToG2o on that (slam_graph.cpp:983-1032): psi = invert_depth(xyz_anchor), one edge per observation of an active point in a keyframe of the
final window, info = (s^2, s^2, 0.333^2) with s = 1 / 2^level.
literal() restates :605-662 line by line with Python dicts and sets, for ANY iteration order of the reference's hash containers.
"""
import functools

import numpy as np

INNER, OUTER = 0, 1


def invert_depth(x):
    """maths_utils.h:66-69: unproject2d(x.head<2>()) / x[2] -- three plain divisions"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    return np.stack([x[:, 0] / x[:, 2], x[:, 1] / x[:, 2], 1.0 / x[:, 2]], 1)


def info_from_level(level):
    """slam_graph.cpp:1010-1015: Lambda = diag(Po2(pyrFromZero_d(1, level)), same, Po2(0.333))"""
    s = 1.0 / np.exp2(np.asarray(level, np.float64))
    return np.stack([s * s, s * s, np.full(len(s), 0.333 * 0.333)], 1)


def _pair_set(pairs):
    e = np.asarray(pairs, np.int64).reshape(-1, 2)
    return {(int(a), int(b)) for a, b in e} | {(int(b), int(a)) for a, b in e}


def prepare(m, w0_ids, w0_types, pairs):
    """-> dict(window_ids, window_types, active_ids, n_edges_bound)"""
    w0_ids = np.asarray(w0_ids, np.int64); w0_types = np.asarray(w0_types, np.int64)
    anchor_of = dict(zip(m["point_ids"].tolist(), m["anchor_ids"].tolist()))
    w0 = set(w0_ids.tolist())
    inner = set(w0_ids[w0_types == INNER].tolist())
    ps = _pair_set(pairs)
    active = set()
    for p, f in zip(m["obs_point"].tolist(), m["obs_kf"].tolist()):
        if f in inner and (anchor_of[p] in w0 or (f, anchor_of[p]) in ps):
            active.add(p)                                                                        # rule 1
    ext = sorted({anchor_of[p] for p in active} - w0)                                            # rule 2
    active = np.array(sorted(active), np.int32)                                                  # rule 4
    n_obs = np.isin(m["obs_point"], active).sum()
    return dict(window_ids=np.concatenate([w0_ids, ext]).astype(np.int32), window_types=np.concatenate([w0_types, np.full(len(ext), OUTER)]).astype(np.int32),
                active_ids=active, n_edges_bound=int(n_obs))


def problem(m, window_ids, active_ids):
    """-> dict(pose_ids, poses, point_ids, psi, anchor_ids, edges): edges are BA_EDGE_DTYPE with IDS in point / pose (anchor: the anchor's id), in the order of the
    map's observations -- what svs_ba_window_update takes"""
    from scavislam_amd.ctypes_types import BA_EDGE_DTYPE
    window_ids = np.asarray(window_ids, np.int32); active_ids = np.asarray(active_ids, np.int32)
    kf_row = {int(k): i for i, k in enumerate(m["kf_ids"])}
    pt_row = {int(p): i for i, p in enumerate(m["point_ids"])}
    rows = np.array([pt_row[int(p)] for p in active_ids], np.int64)
    keep = np.isin(m["obs_point"], active_ids) & np.isin(m["obs_kf"], window_ids)                # observers n final window (:1001-1006)
    e = np.zeros(int(keep.sum()), BA_EDGE_DTYPE)
    e["obs"] = m["obs_center"][keep]
    e["info"] = info_from_level(m["obs_level"][keep])
    e["point"] = m["obs_point"][keep]
    e["pose"] = m["obs_kf"][keep]
    e["anchor"] = [m["anchor_ids"][pt_row[int(p)]] for p in e["point"]]
    return dict(pose_ids=window_ids, poses=m["kf_poses"][[kf_row[int(k)] for k in window_ids]].copy(), point_ids=active_ids,
                psi=invert_depth(m["xyz"][rows]) if len(rows) else np.zeros((0, 3)), anchor_ids=m["anchor_ids"][rows].astype(np.int32), edges=e)


def literal(m, w0_ids, w0_types, pairs, rng=None):
    """slam_graph.cpp:605-662 as written; rng (or None) decides the iteration order of double_window_ and of every feature_table -> (double_window_ as a dict,
    active_point_set_)"""
    order = (lambda seq: list(seq)) if rng is None else (lambda seq: [seq[i] for i in rng.permutation(len(seq))])
    double_window = {int(k): int(t) for k, t in zip(w0_ids, w0_types)}
    feature_table = {}
    for p, f in zip(m["obs_point"].tolist(), m["obs_kf"].tolist()):
        feature_table.setdefault(f, []).append(p)
    anchor_of = dict(zip(m["point_ids"].tolist(), m["anchor_ids"].tolist()))
    edge_table = _pair_set(pairs)                                                                # orderd_find is symmetric
    active_point_set, extend_outer_window = set(), {}
    for frame_id in order(list(double_window)):                                                  # :605
        if double_window[frame_id] == INNER:                                                     # :611
            for point_id in order(feature_table.get(frame_id, [])):                              # :616
                if point_id not in active_point_set:                                             # :623
                    anchorframe_id = anchor_of[point_id]
                    if anchorframe_id in double_window:                                          # :627
                        active_point_set.add(point_id)
                    elif (frame_id, anchorframe_id) in edge_table:                               # :636
                        active_point_set.add(point_id)
                        extend_outer_window[anchorframe_id] = OUTER                              # :642
    double_window.update(extend_outer_window)                                                    # :662
    return double_window, active_point_set


# ---- the test scene ---------------------------------------------------------------------------------------------------------------------------------------------
N_KF, N_OUTSIDE, N_OUTER = 14, 3, 3      # keyframes 0-2 outside W0, 3-5 OUTER, 6-13 INNER (a chain in time; points are seen in runs of consecutive keyframes,
                                         # anchored at the first)


@functools.lru_cache(maxsize=None)
def scene(n_points=1700, seed=11):
    """The map, W0 and the pairs of tests/test_ba_map_cpu.py and tests/test_gpu_ba_map.py, from the flat arrays of synth.ba_window shaped as
    test_gpu_hipbranch._graph_tables shapes them (ids 100 + 3 i cross bitmap words).  Returns dict(map, w0_ids, w0_types, pairs, cons (BA_CONSTRAINT_DTYPE, frame
    ids), cam).  Treat it as read-only: it is shared."""
    from scavislam_amd import synth
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE
    rng = np.random.default_rng(seed)
    prob = synth.ba_window(P=N_KF, L=n_points, seed=seed, n_outer=0)
    kf_ids = (100 + 3 * np.arange(N_KF)).astype(np.int32)
    point_ids = (5000 + 7 * np.arange(n_points)).astype(np.int32)
    e = prob["edges"]
    anchor_idx = np.zeros(n_points, np.int64)
    anchor_idx[e["point"]] = e["anchor"]
    level = np.round(np.log(1.0 / e["info"][:, 0]) / np.log(4.0)).astype(np.int32)
    obs_point, obs_kf, obs_center, obs_level = point_ids[e["point"]], kf_ids[e["pose"]], e["obs"].copy(), level
    # rule (g): some points anchored inside W0 are also in the feature_table of keyframe 0, which stays outside the final window
    late = np.nonzero(anchor_idx >= N_OUTSIDE + N_OUTER)[0]
    extra = rng.choice(late, 60, replace=False)
    obs_point = np.concatenate([obs_point, point_ids[extra]]); obs_kf = np.concatenate([obs_kf, np.full(60, kf_ids[0])])
    obs_center = np.concatenate([obs_center, rng.uniform(0, 400, (60, 3))]); obs_level = np.concatenate([obs_level, rng.integers(0, 3, 60).astype(np.int32)])
    shuffle = rng.permutation(len(obs_point))                                                    # the order of arrival is not by point
    m = dict(kf_ids=kf_ids, kf_poses=prob["poses"].copy(), point_ids=point_ids, anchor_ids=kf_ids[anchor_idx], xyz=invert_depth(prob["psi"]),
             obs_point=obs_point[shuffle].astype(np.int32), obs_kf=obs_kf[shuffle].astype(np.int32), obs_center=obs_center[shuffle], obs_level=obs_level[shuffle].astype(np.int32))
    first_in = N_OUTSIDE
    w0_ids = kf_ids[first_in:].copy()
    w0_types = (np.arange(first_in, N_KF) < N_OUTSIDE + N_OUTER).astype(np.int32)
    i0 = N_OUTSIDE + N_OUTER                                                                     # the first INNER keyframe
    # edge_table_ entries with an INNER end: the chain's neighbours; (i0, 2): keyframe 2 enters through the first INNER observer of its points; (i0 + 1, 1): keyframe 1
    # only through the SECOND INNER observer; (13, 0): an INNER keyframe that sees no point anchored in keyframe 0
    pairs = [(kf_ids[i], kf_ids[i - d]) for i in range(i0, N_KF) for d in (1, 2)] + [(kf_ids[2], kf_ids[i0]), (kf_ids[i0 + 1], kf_ids[1]), (kf_ids[N_KF - 1], kf_ids[0])]
    # marginalised constraints along the chain wherever an end is not INNER (ba_window's noise model and information, slam_graph.cpp:842-845)
    gt = prob["poses_gt"].reshape(-1, 3, 4)
    cons = np.zeros(i0 - 1, BA_CONSTRAINT_DTYPE)
    for c, i in enumerate(range(1, i0)):
        T_ji = synth.pose_mul(gt[i + 1], synth.pose_inv(gt[i]))
        dn = np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.002, 3)])
        T_ji = synth.pose_mul(synth.pose(synth.so3_exp(dn[3:]), dn[:3]), T_ji)
        Lam = np.eye(6) * 30.0
        Lam[:3, :3] *= (350 * np.linalg.norm(T_ji[:, 3]) / 8.0) ** 2
        Lam[3:, 3:] *= 100.0 ** 2
        cons[c]["T_21"], cons[c]["info"], cons[c]["pose1"], cons[c]["pose2"] = T_ji.reshape(12), Lam.reshape(36), kf_ids[i], kf_ids[i + 1]
    return dict(map=m, w0_ids=w0_ids, w0_types=w0_types, pairs=np.array(pairs, np.int32), cons=cons, cam=prob["cam"])


def rule_cases(sc):
    """point ids per case (a)-(h) of the issue's list, counted on the model alone"""
    m = sc["map"]
    prep = prepare(m, sc["w0_ids"], sc["w0_types"], sc["pairs"])
    w0 = set(sc["w0_ids"].tolist()); inner = set(sc["w0_ids"][sc["w0_types"] == INNER].tolist()); outer = w0 - inner
    final = set(prep["window_ids"].tolist()); ext = final - w0
    active = set(prep["active_ids"].tolist())
    ps = _pair_set(sc["pairs"])
    anchor_of = dict(zip(m["point_ids"].tolist(), m["anchor_ids"].tolist()))
    observers = {}
    for p, f in zip(m["obs_point"].tolist(), m["obs_kf"].tolist()):
        observers.setdefault(p, set()).add(f)
    case = {k: set() for k in "abcdefgh"}
    for p, obs in observers.items():
        a = anchor_of[p]
        obs_in = sorted(obs & inner)
        if p in active and a in w0:
            case["a"].add(p)
        if p in active and a not in w0:
            case["b"].add(p)
            if len(obs_in) >= 2 and (obs_in[0], a) not in ps:
                case["c"].add(p)
        if p not in active and obs_in and a not in w0 and any((f, a) in ps for f in inner - obs):
            case["d"].add(p)
        if p not in active and obs_in and a in ext:
            case["e"].add(p)
        if p not in active and not obs_in and obs & outer:
            case["f"].add(p)
        if p in active and obs - final:
            case["g"].add(p)
        if p in active and any(f in ext and f != a for f in obs):
            case["h"].add(p)
    return case, prep
