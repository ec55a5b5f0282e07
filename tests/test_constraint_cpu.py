"""CPU tests of the yardstick of the pose graph's edges and constraints (tests/constraint_model.py) and of the host-side pair selection
(scavislam_amd.register): each against a literal restatement of the reference's lines with Python dicts and sets, under shuffled iteration orders of its hash
containers.  What stays unpinned is Sophus' own arithmetic: the restatements use the model's pose helpers."""
import numpy as np
import pytest

import constraint_model as CM
from register_model import pose_inv, pose_mul


def _literal_compute_constraint(m, window, kf1, kf2, absolute_pose, rng):
    """slam_graph.cpp:787-846 as written; rng decides the iteration order of v1.feature_table (v2's is only searched).  absolute_pose: computeAbsolutePose's results"""
    ft, pose, point = CM.tables(m)
    order = lambda seq: [seq[i] for i in rng.permutation(len(seq))]
    cache_poses = {}
    T1, T2 = pose[kf1], pose[kf2]
    T_1_from_2 = pose_mul(T1, pose_inv(T2))                                                      # :793
    depth_set = []
    v2_table = set(order(sorted(ft[kf2])))
    for point_id in order(sorted(ft[kf1])):                                                      # :797
        if point_id not in v2_table:                                                             # :802
            continue
        anchorframe_id, xyz_anchor = point[point_id]
        if anchorframe_id in window:                                                             # :809
            T_anchor_from_w = pose[anchorframe_id]
        elif anchorframe_id in cache_poses:                                                      # :814
            T_anchor_from_w = cache_poses[anchorframe_id]
        else:
            T_anchor_from_w = absolute_pose[anchorframe_id]                                      # :821
            cache_poses[anchorframe_id] = T_anchor_from_w
        xyz_v1 = CM.pose_act(T1, CM.pose_act(pose_inv(T_anchor_from_w), xyz_anchor))             # :827
        depth_set.append(CM.norm3(xyz_v1))                                                       # :829 (a multiset: sorted when read)
    visibility_strength = len(depth_set)
    median_depth = CM.median(depth_set)                                                          # :838
    norm_dist = float(np.float64(CM.norm3([T_1_from_2[3], T_1_from_2[7], T_1_from_2[11]])) / np.float64(median_depth))
    alpha = 1
    Lambda = np.eye(6)                                                                           # :842
    Lambda *= visibility_strength
    Lambda[:3, :3] *= (350 * alpha * norm_dist) * (350 * alpha * norm_dist)
    Lambda[3:, 3:] *= (100 * alpha) * (100 * alpha)
    return T_1_from_2, Lambda, visibility_strength, median_depth


@pytest.mark.parametrize("pair", [("A", "B"), ("B", "A"), ("A", "C"), ("D", "C"), ("F", "A"), ("A", "F"), ("G", "H"), ("I", "A"), ("T", "U"), ("V", "T"), ("U", "V")])
def test_model_equals_the_literal_restatement_for_every_hash_order(pair):
    sc = CM.scene()
    m, ids = sc["map"], sc["ids"]
    kf1, kf2 = ids[pair[0]], ids[pair[1]]
    _, pose, _ = CM.tables(m)
    absolute = {k: [v + 0.015625 for v in pose[k]] for k in sc["outside"]}                       # "computeAbsolutePose" gives something else than the stored pose
    want = CM.compute(m, sc["window_small"], kf1, kf2, cached=absolute)
    assert want["status"] == CM.OK and want["strength"] == len(want["depths"]) > 0
    for seed in range(4):
        T, Lam, strength, med = _literal_compute_constraint(m, set(sc["window_small"]), kf1, kf2, absolute, np.random.default_rng(seed))
        assert strength == want["strength"]
        assert np.float64(med).tobytes() == np.float64(want["median"]).tobytes()
        assert np.array(T).tobytes() == want["T_12"].tobytes()
        assert Lam.reshape(36).tobytes() == want["info"].tobytes()


def test_scene_has_the_prescribed_common_point_counts():
    sc = CM.scene()
    m, ids = sc["map"], sc["ids"]
    t = CM.tables(m)
    n = lambda a, b, **kw: CM.compute(m, sc["window_all"], ids[a], ids[b], _tables=t, **kw)
    assert [n("A", x)["strength"] for x in "BCDEFGHIJ"] == [1500, 513, 512, 65, 64, 3, 2, 1, 0]
    assert n("A", "J")["status"] == CM.EMPTY and n("A", "J")["info"].tobytes() == np.zeros(36).tobytes()
    assert n("T", "U")["strength"] == 100 and n("T", "V")["strength"] == 100 and n("U", "V")["strength"] == 85
    # the ties: with kf1 = T thirty depths are one value, both middle ranks of (T, U) inside them, those of (T, V) astride their upper end
    for other, inside in (("U", True), ("V", False)):
        d = np.sort(n("T", other)["depths"])
        assert (d == d[49]).sum() == 30 and (d[50] == d[49]) == inside
    # missing anchors with the small window: ascending, each once
    o = CM.compute(m, sc["window_small"], ids["A"], ids["B"], _tables=t)
    assert o["status"] == CM.MISSING_ANCHOR and o["missing"].tolist() == sc["outside"] and o["n_missing"] == 4 and o["strength"] == 1500
    # an override moves the depths of the points anchored there and T_12
    T = m["kf_poses"][0].copy(); T[3] += 0.25
    a, b = n("A", "B"), n("A", "B", overrides=[(ids["A"], T)])
    assert a["T_12"].tobytes() != b["T_12"].tobytes() and (a["depths"] != b["depths"]).sum() > 100


def test_median_is_the_reference_s():
    assert CM.median([3.0]) == 3.0
    assert CM.median([4.0, 1.0]) == 0.5 * (1.0 + 4.0)
    assert CM.median([9.0, 1.0, 5.0]) == 5.0
    assert CM.median([7.0, 1.0, 3.0, 5.0]) == 0.5 * (3.0 + 5.0)
    assert CM.median([2.0, 2.0, 2.0, 9.0]) == 2.0 and CM.median([1.0, 2.0, 2.0, 2.0, 9.0]) == 2.0 and CM.median([1.0, 2.0, 2.0, 9.0]) == 2.0
    a, b = 0.1, 0.30000000000000004                                                              # the sum is formed first, then halved
    assert CM.median([b, a]) == 0.5 * (a + b)
    with pytest.raises(AssertionError):
        CM.median([])


class _LiteralEdgeTable:
    """slam_graph.hpp:242-331 as written: T_1_from_2 and both Lambdas per edge, keyed (smaller, larger)"""

    def __init__(self):
        self.t = {}

    def insertEdge(self, id1, id2, strength, edge_type):
        assert id1 != id2
        key = (id1, id2) if id1 < id2 else (id2, id1)
        assert key not in self.t
        self.t[key] = dict(is_marginalized_=False, T_1_from_2=None, Lambda_1_from_2=None, Lambda_2_from_1=None)

    def setConstraint(self, id1, id2, T_1_from_2, Lambda_1_from_2, Lambda_2_from_1):
        assert id1 != id2
        if id1 < id2:
            e = self.t[(id1, id2)]
            e["is_marginalized_"] = True
            e["T_1_from_2"] = list(T_1_from_2); e["Lambda_2_from_1"] = Lambda_2_from_1; e["Lambda_1_from_2"] = Lambda_1_from_2
        else:
            e = self.t[(id2, id1)]
            e["is_marginalized_"] = True
            e["T_1_from_2"] = pose_inv(T_1_from_2); e["Lambda_2_from_1"] = Lambda_1_from_2; e["Lambda_1_from_2"] = Lambda_2_from_1

    def getConstraint_id1_from_id2(self, id1, id2):
        assert id1 != id2
        if id1 < id2:
            e = self.t[(id1, id2)]
            if not e["is_marginalized_"]:
                return False, None, None
            return True, e["T_1_from_2"], e["Lambda_1_from_2"]
        e = self.t[(id2, id1)]
        if not e["is_marginalized_"]:
            return False, None, None
        return True, pose_inv(e["T_1_from_2"]), e["Lambda_2_from_1"]

    def unMarginalize(self, id1, id2):
        self.t[(id1, id2) if id1 < id2 else (id2, id1)]["is_marginalized_"] = False

    def orderd_find(self, id1, id2):
        return ((id1, id2) if id1 < id2 else (id2, id1)) in self.t


def _random_pose(rng):
    from scavislam_amd import synth
    return [float(v) for v in synth.pose(synth.so3_exp(rng.normal(0, 0.3, 3)), rng.normal(0, 1, 3)).reshape(12)]


def _two_tables(rng, ids, n_edges, marginalise=0.8):
    """the model's table and the literal one with the same random edges, set in random orientation"""
    mine, ref = CM.EdgeTable(), _LiteralEdgeTable()
    pairs = set()
    while len(pairs) < n_edges:
        a, b = rng.choice(ids, 2, replace=False)
        pairs.add((int(min(a, b)), int(max(a, b))))
    for a, b in sorted(pairs):
        if rng.random() < 0.5:
            a, b = b, a
        mine.insert(a, b, 7, 1); ref.insertEdge(a, b, 7, 1)
        if rng.random() < marginalise:
            x, y = (a, b) if rng.random() < 0.5 else (b, a)
            T, Lam = _random_pose(rng), np.diag(rng.uniform(1, 9, 6)).reshape(36)
            mine.set_constraint(x, y, T, Lam); ref.setConstraint(x, y, T, Lam, Lam)
    return mine, ref, sorted(pairs)


def test_edge_table_orientation_rules():
    rng = np.random.default_rng(2)
    mine, ref, pairs = _two_tables(rng, np.arange(10, 30), 40)
    assert any(e["is_marginalized"] for e in mine.e.values()) and not all(e["is_marginalized"] for e in mine.e.values())
    for a, b in pairs:
        for id1, id2 in ((a, b), (b, a)):                                                        # set and get with id1 > id2 as well
            ok, T, Lam = ref.getConstraint_id1_from_id2(id1, id2)
            T_m, Lam_m, marg = mine.get_1_from_2(id1, id2)
            assert bool(marg) == ok
            if ok:
                assert np.array(T).tobytes() == np.array(T_m).tobytes() and np.asarray(Lam).tobytes() == Lam_m.tobytes()
    a, b = next(k for k, e in mine.e.items() if e["is_marginalized"])
    before = (list(mine.e[(a, b)]["T"]), mine.e[(a, b)]["info"].copy())
    mine.un_marginalize(b, a); ref.unMarginalize(b, a)
    assert ref.getConstraint_id1_from_id2(a, b)[0] is False and mine.get_1_from_2(a, b)[2] == 0
    assert mine.e[(a, b)]["T"] == before[0] and np.array_equal(mine.e[(a, b)]["info"], before[1])      # T and Lambda stay
    with pytest.raises(AssertionError):
        mine.insert(b, a, 1, 0)
    with pytest.raises(AssertionError):
        mine.insert(a, a, 1, 0)


def _literal_copy_constraints(double_window, ref):
    """slam_graph.cpp:937-981 over double_window (a dict in its iteration order) -> [(pose_id_1, pose_id_2, T_2_from_1, Lambda)]"""
    out = []
    for pose_id_1, wtype_1 in double_window.items():
        for pose_id_2, wtype_2 in double_window.items():
            if pose_id_2 == pose_id_1:
                continue
            if not ref.orderd_find(pose_id_1, pose_id_2):
                continue
            if wtype_1 == CM.OUTER or wtype_2 == CM.OUTER:
                is_marginalized, T_2_from_1, Lambda_2_from_1 = ref.getConstraint_id1_from_id2(pose_id_2, pose_id_1)
                assert is_marginalized
                out.append((pose_id_1, pose_id_2, T_2_from_1, Lambda_2_from_1))
    return out


def test_constraint_list_equals_literal_copy_constraints_as_multisets():
    rng = np.random.default_rng(4)
    ids = np.arange(40, 60)
    mine, ref, pairs = _two_tables(rng, ids, 60, marginalise=1.0)
    win = rng.choice(ids, 12, replace=False)
    types = (rng.random(12) < 0.4).astype(int)
    want = constraint_set = sorted((int(c["pose1"]), int(c["pose2"]), c["T_21"].tobytes(), c["info"].tobytes()) for c in CM.constraint_list(win, types, mine))
    assert len(want) >= 6 and len(want) % 2 == 0                                                 # every edge once per direction
    for seed in range(4):
        order = np.random.default_rng(seed).permutation(12)
        dw = {int(win[i]): int(types[i]) for i in order}
        got = sorted((a, b, np.array(T).tobytes(), np.asarray(L).tobytes()) for a, b, T, L in _literal_copy_constraints(dw, ref))
        assert got == constraint_set
    # the stated order: i over the window, then j
    lst = CM.constraint_list(win, types, mine)
    pos = {int(k): i for i, k in enumerate(win)}
    keys = [(pos[int(c["pose1"])], pos[int(c["pose2"])]) for c in lst]
    assert keys == sorted(keys)
    # by window index the records are the same
    by_idx = CM.constraint_list(win, types, mine, by_index=True)
    assert [(int(c["pose1"]), int(c["pose2"])) for c in by_idx] == keys and by_idx["T_21"].tobytes() == lst["T_21"].tobytes()
    # an edge with an OUTER end that is not marginalised: the reference asserts
    c = lst[0]
    mine.un_marginalize(int(c["pose1"]), int(c["pose2"]))
    with pytest.raises(AssertionError):
        CM.constraint_list(win, types, mine)


def _literal_unmarg(double_window, has_edge):
    """slam_graph.cpp:728-759 -> the unMarginalize calls"""
    calls = []
    for pose_id_1, wtype_1 in double_window.items():
        if wtype_1 == CM.INNER:
            for pose_id_2, wtype_2 in double_window.items():
                if pose_id_2 == pose_id_1:
                    continue
                if wtype_2 == CM.INNER:
                    if has_edge(pose_id_1, pose_id_2):
                        calls.append((pose_id_1, pose_id_2))
    return calls


def _literal_marg(old_window, double_window, has_edge):
    """slam_graph.cpp:848-904 -> the (pose_id_1, pose_id_2) of every computeConstraint + setConstraint"""
    calls = []
    for pose_id_1, wtype_1 in old_window.items():
        if wtype_1 == CM.INNER:
            for pose_id_2, wtype_2 in old_window.items():
                if pose_id_2 == pose_id_1:
                    continue
                if not has_edge(pose_id_1, pose_id_2):
                    continue
                if wtype_2 == CM.INNER:
                    pose_1_is_in_inner_window_now = double_window.get(pose_id_1) == CM.INNER
                    pose_2_is_in_inner_window_now = double_window.get(pose_id_2) == CM.INNER
                    if not pose_1_is_in_inner_window_now or not pose_2_is_in_inner_window_now:
                        calls.append((pose_id_1, pose_id_2))
    return calls


def test_pair_selection_of_update_marginalization():
    from scavislam_amd.register import entering_inner_pairs, left_inner_pairs
    rng = np.random.default_rng(6)
    ids = np.arange(200, 230)
    for trial in range(5):
        keys = set()
        while len(keys) < 90:
            a, b = rng.choice(ids, 2, replace=False)
            keys.add((int(min(a, b)), int(max(a, b))))
        has_edge = lambda a, b: (min(a, b), max(a, b)) in keys
        old_ids = rng.choice(ids, 14, replace=False); old_types = (rng.random(14) < 0.35).astype(int)
        # the new window keeps most of the old one, moves some keyframes to OUTER, drops some and adds new ones
        keep = old_ids[rng.random(14) < 0.75]
        fresh = rng.choice(np.setdiff1d(ids, old_ids), 4, replace=False)
        new_ids = np.concatenate([keep, fresh]); new_types = (rng.random(len(new_ids)) < 0.35).astype(int)
        old_w = {int(k): int(t) for k, t in zip(old_ids, old_types)}
        new_w = {int(k): int(t) for k, t in zip(new_ids, new_types)}
        un = {(min(a, b), max(a, b)) for a, b in _literal_unmarg(new_w, has_edge)}
        left = {(min(a, b), max(a, b)) for a, b in _literal_marg(old_w, new_w, has_edge)}
        got_un, got_left = entering_inner_pairs((new_ids, new_types), keys), left_inner_pairs((old_ids, old_types), (new_ids, new_types), keys)
        assert len(set(got_un)) == len(got_un) and set(got_un) == un and all(a < b for a, b in got_un)
        assert len(set(got_left)) == len(got_left) and set(got_left) == left and all(a < b for a, b in got_left)
        assert not (set(got_left) & set(got_un))      # an edge that is unmarginalised has both ends INNER now
    assert left and un
