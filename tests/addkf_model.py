"""The yardstick of svs_map_compute_strength / svs_map_add_keyframe: SlamGraph::computeStrength (slam_graph.cpp:467-552) as the closed form that
include/scavislam_hip.h states, SlamGraph::addKeyframe (:143-186) behind it on a small host graph, and the twin-map sequence -- the same insertion replayed
through svs_map_add_keyframes, _add_points, _add_measured_observations, _add_edges and one storing _compute_constraints.  tests/test_addkf_cpu.py holds the
closed form to a literal restatement of the reference's loops."""
import numpy as np

I12 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
MAX_NEIGHBORS = 1024


def pose_mul(A, B):
    """csrc/pose.h: rows (a0 b0 + a1 b1) + a2 b2, the translation added last; f64, no contraction"""
    A, B = [float(v) for v in A], [float(v) for v in B]
    C = [0.0] * 12
    for i in range(3):
        for j in range(4):
            C[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]
        C[4 * i + 3] += A[4 * i + 3]
    return C


def strength_closed_form(new_anchors, track, vis, thr, half_width, half_height):
    """new_anchors: anchor_id per new point; track: (global_id, u, v) per entry; vis: {point id: observers} of the map before the insertion.
    -> (keys ascending: [kf, strength, n_left, n_right, n_top, n_bottom], exists per track entry, m)"""
    exists = [g in vis for g, _, _ in track]
    E = [(i, g, u, v) for i, (g, u, v) in enumerate(track) if g in vis]
    keys = set(int(a) for a in new_anchors)
    for _, g, _, _ in E:
        keys |= set(vis[g])
    out = []
    h = max(int(thr) // 2, 1)
    for f in sorted(keys):
        if not E:
            out.append([f, sum(1 for a in new_anchors if a == f), 0, 0, 0, 0])
            continue
        seen = [(i, u < half_width, v < half_height) for i, g, u, v in E if f in vis[g]]
        cls = [[i for i, l, _ in seen if l], [i for i, l, _ in seen if not l], [i for i, _, t in seen if t], [i for i, _, t in seen if not t]]
        tot = [len(c) for c in cls]
        if min(tot) < h:
            out.append([f, 0] + tot)
            continue
        t_star = max(c[h - 1] for c in cls)
        out.append([f, sum(1 for i, _, _ in seen if i >= t_star)] + tot)
    return out, exists, len(E)


class Graph:
    """what addKeyframe reads and writes: poses, points, vis_set per point, the pair log with its measurements, the edges in slot order"""

    def __init__(self):
        self.pose, self.point, self.vis, self.log, self.edges = {}, {}, {}, [], []

    def add_first_keyframe(self, kf):
        assert not self.pose and not self.point
        self.pose[int(kf)] = list(I12)

    def add_keyframe(self, newkey, oldkey, T_rel, new_points, track_points, thr, half_width, half_height):
        """new_points: dicts point_id, anchor_id, xyz_anchor, anchor_obs_pyr, anchor_level, feat_center, feat_level; track_points: dicts global_id, center, level.
        -> the outcome: pose, keys (after the clamp, with the edge mark), kept, exists, m, over_capacity, points / pairs / edges in the twin's order"""
        newkey, oldkey = int(newkey), int(oldkey)
        assert oldkey in self.pose and newkey not in self.pose
        keys, exists, m = strength_closed_form([p["anchor_id"] for p in new_points], [(t["global_id"], t["center"][0], t["center"][1]) for t in track_points],
                                               self.vis, thr, half_width, half_height)
        if len(keys) > MAX_NEIGHBORS:
            return dict(over_capacity=True, n_keys=len(keys))
        table = {k[0]: k for k in keys}
        assert oldkey in table                                     # (:165)
        table[oldkey][1] = max(table[oldkey][1], thr)
        for k in keys:
            k.append(1 if k[1] >= thr else 0)
        pose = pose_mul(T_rel, self.pose[oldkey])
        kept = [table[p["anchor_id"]][1] >= thr for p in new_points]
        pts = [p for p, c in zip(new_points, kept) if c]
        pairs = []                                                 # (point, keyframe, centre, level)
        for p in pts:
            pairs.append((p["point_id"], newkey, list(p["feat_center"]), p["feat_level"]))
            pairs.append((p["point_id"], p["anchor_id"], [float(c) * float(2 ** p["anchor_level"]) for c in p["anchor_obs_pyr"]], p["anchor_level"]))
        first = set()
        for t, e in zip(track_points, exists):
            if e and t["global_id"] not in first:
                first.add(t["global_id"])
                pairs.append((t["global_id"], newkey, list(t["center"]), t["level"]))
        edges = [(k[0], newkey, k[1]) for k in keys if k[6]]
        # the graph afterwards
        self.pose[newkey] = pose
        for p in pts:
            self.point[p["point_id"]] = p
            self.vis[p["point_id"]] = set()
        for pid, kf, _, _ in pairs:
            self.vis[pid].add(kf)
        self.log += pairs
        self.edges += edges
        return dict(over_capacity=False, n_keys=len(keys), pose=pose, keys=keys, kept=kept, exists=exists, m=m, points=pts, pairs=pairs, edges=edges)


def key_records(keys, dtype, cap=MAX_NEIGHBORS):
    """the model's key table as the library's array: zero behind the keys"""
    out = np.zeros(cap, dtype)
    for r, k in enumerate(keys):
        out[r]["kf_id"], out[r]["strength"], out[r]["n_left"], out[r]["n_right"], out[r]["n_top"], out[r]["n_bottom"] = k[:6]
        out[r]["edge"] = k[6] if len(k) > 6 else 0
    return out


def new_point_records(new_points, dtype):
    out = np.zeros(len(new_points), dtype)
    for o, p in zip(out, new_points):
        o["xyz_anchor"], o["anchor_obs_pyr"], o["feat_center"] = p["xyz_anchor"], p["anchor_obs_pyr"], p["feat_center"]
        o["point_id"], o["anchor_id"], o["anchor_level"], o["feat_level"] = p["point_id"], p["anchor_id"], p["anchor_level"], p["feat_level"]
    return out


def track_point_records(track_points, dtype):
    out = np.zeros(len(track_points), dtype)
    for o, t in zip(out, track_points):
        o["center"], o["global_id"], o["level"] = t["center"], t["global_id"], t["level"]
    return out


def replay_on_twin(twin, newkey, kf_record, disp, fast_thr, outcome, cand_dtype, cached=None, batch=256):
    """the bar of svs_map_add_keyframe: the outcome through the existing calls of a ResidentMap, in the order the header states.  -> the constraint results"""
    kf = np.array(kf_record).reshape(-1)[:1].copy()
    kf["T_anchor_from_w"][0] = outcome["pose"]
    twin.add_keyframes([newkey], kf, [disp], [fast_thr])
    pts = np.zeros(len(outcome["points"]), cand_dtype)
    for o, p in zip(pts, outcome["points"]):
        o["xyz_anchor"], o["anchor_obs_pyr"], o["anchor_level"], o["kf_index"] = p["xyz_anchor"], p["anchor_obs_pyr"], p["anchor_level"], p["anchor_id"]
    if len(pts):
        twin.add_points([p["point_id"] for p in outcome["points"]], pts)
    pr = outcome["pairs"]
    if pr:
        twin.add_measured_observations([q[0] for q in pr], [q[1] for q in pr], [q[2] for q in pr], [q[3] for q in pr])
    ed = outcome["edges"]
    twin.add_edges([(a, b) for a, b, _ in ed], [s for _, _, s in ed], 0)
    res = []
    for at in range(0, len(ed), batch):
        res += twin.compute_constraints([dict(kf1=a, kf2=b, store=True, cached=cached) for a, b, _ in ed[at:at + batch]])
    return res
