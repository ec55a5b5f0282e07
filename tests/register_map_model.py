"""The device-resident map of the back end and the requests its walk builds, restated in plain Python -- the yardstick of svs_map_* / svs_reg_register_map_batch.

MapModel mirrors the map with dicts and a set of (point, keyframe) pairs.  MapModel.request() applies the three rules of include/scavislam_hip.h and returns a
request as tests/register_model.py (and svs_reg_register_batch) take it:
    1. source points: LOCAL -- every point with an observation in a keyframe of `walk` that is neither the root nor in `direct`; LOOP -- every point observed by
       walk[0]; each once, in ascending point id
    2. keyframe table: entry 0 the root; behind it, ascending, the anchors of the source points and the keyframes of `walk`; flags IN_WINDOW from the map,
       DIRECT_NEIGHBOR for the root and `direct`
    3. observer rows (LOCAL): per source point the table entries of its observers, ascending
literal_local() / literal_loop() restate backend.cpp:480-545 / :853-893 line by line with Python sets, for ANY iteration order of the reference's hash sets.
"""
import numpy as np

import register_model as M


class MapModel:
    def __init__(self):
        self.kf = {}          # id -> dict(T [12], window bool, **whatever the caller attaches: images, thresholds)
        self.pt = {}          # id -> CANDIDATE_DTYPE record, kf_index = anchor id, point_id = id
        self.obs = set()      # (point id, keyframe id)

    # ---- the updates, refusing what svs_map_* refuses (ValueError, nothing changed)
    def add_keyframes(self, ids, Ts, **attached):
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids) or any(i < 0 or i in self.kf for i in ids):
            raise ValueError("keyframe id present or repeated")
        for n, i in enumerate(ids):
            self.kf[i] = dict(T=np.asarray(Ts[n], np.float64).reshape(12).copy(), window=False, **{k: v[n] for k, v in attached.items()})

    def add_points(self, ids, pts):
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids) or any(i < 0 or i in self.pt for i in ids) or any(int(p["kf_index"]) not in self.kf for p in pts):
            raise ValueError("point id present or repeated, or anchor not in the map")
        for i, p in zip(ids, pts):
            q = np.array(p)
            q["point_id"], q["pad_"] = i, 0
            self.pt[i] = q

    def add_observations(self, point_ids, kf_ids):
        pairs = [(int(p), int(k)) for p, k in zip(point_ids, kf_ids)]
        if any(p not in self.pt or k not in self.kf for p, k in pairs):
            raise ValueError("unknown point or keyframe")
        self.obs |= set(pairs)

    def set_poses(self, kf_ids, Ts):
        if any(int(k) not in self.kf for k in kf_ids):
            raise ValueError("unknown keyframe")
        for k, T in zip(kf_ids, Ts):
            self.kf[int(k)]["T"] = np.asarray(T, np.float64).reshape(12).copy()

    def set_points(self, point_ids, xyz):
        if any(int(p) not in self.pt for p in point_ids):
            raise ValueError("unknown point")
        for p, x in zip(point_ids, xyz):
            self.pt[int(p)]["xyz_anchor"] = x

    def set_window(self, kf_ids):
        if any(int(k) not in self.kf for k in kf_ids):
            raise ValueError("unknown keyframe")
        for k in self.kf:
            self.kf[k]["window"] = False
        for k in kf_ids:
            self.kf[int(k)]["window"] = True

    def info(self):
        return len(self.kf), len(self.pt), len(self.obs)

    def feature_table(self, kf):
        return [p for p, k in self.obs if k == kf]

    # ---- rules 1-3
    def source_points(self, mode, root, walk, direct):
        if mode == M.LOOP:
            marking = [walk[0]]
        else:
            skip = set(direct) | {root}
            marking = [k for k in walk if k not in skip]
        marking = set(marking)
        return sorted({p for p, k in self.obs if k in marking})

    def request(self, mode, root, T_root, walk, direct):
        from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
        ids = self.source_points(mode, root, walk, direct)
        table = [root] + sorted((set(int(self.pt[p]["kf_index"]) for p in ids) | set(walk)) - {root})
        entry = {k: e for e, k in enumerate(table)}
        src = np.zeros(len(ids), CANDIDATE_DTYPE)
        for i, p in enumerate(ids):
            src[i] = self.pt[p]
            src[i]["kf_index"] = entry[int(self.pt[p]["kf_index"])]
        flags = np.array([(M.IN_WINDOW if self.kf[k]["window"] else 0) | (M.DIRECT_NEIGHBOR if (k == root or k in set(direct)) else 0) for k in table], np.uint8)
        ob, ok = [0], []
        if mode == M.LOCAL:
            observers = {}
            for p, k in self.obs:
                observers.setdefault(p, []).append(k)
            for p in ids:
                ok += sorted(entry[k] for k in observers.get(p, ()) if k in entry)
                ob.append(len(ok))
        else:
            ob = [0] * (len(ids) + 1)
        return dict(mode=mode, T_root=np.asarray(T_root, np.float64).reshape(12), root_kf=0, kf_T=np.array([self.kf[k]["T"] for k in table]), flags=flags, src=src,
                    obs_begin=np.array(ob, np.int32), obs_kf=np.array(ok, np.int32), kf_ids=np.array(table, np.int32), point_ids=np.array(ids, np.int32))


# ---- backend.cpp, line by line -------------------------------------------------------------------------------------------------------------------------------
def _visible(model, T_root, p, cams):
    """:506-526 / :861-878 for one point -> kept"""
    rec = model.pt[p]
    a, lvl = int(rec["kf_index"]), int(rec["anchor_level"])
    if not model.kf[a]["window"]:                                   # IS_IN_SET(p.anchorframe_id, graph_.double_window()) == false
        return False
    u, v = M.project(T_root, model.kf[a]["T"], rec["xyz_anchor"], cams[lvl])
    return M.in_frame_after_cast(u, v, cams[lvl])


def literal_local(model, cam, root, T_root, larger_neighborhood, direct_neighbors, rng=None):
    """pointsVisibleInRoot (:472-546) behind localRegisterFrame's vertex_table.insert(root) (:571).  larger_neighborhood / direct_neighbors: the two unordered
    sets; rng: shuffles every hash-set / hash-map iteration (the reference's order is no function of its input).
    -> (point_set, candidate_point_list as ids in push_back order, vertex_table as a set of ids)"""
    cams = M.level_cams(cam)
    order = lambda xs: list(xs) if rng is None else [list(xs)[i] for i in rng.permutation(len(xs))]
    vertex_table = {root}
    point_set, candidate_point_list = set(), []
    for keyframe_id in order(larger_neighborhood):
        if keyframe_id in direct_neighbors:
            continue
        for point_id in order(model.feature_table(keyframe_id)):
            if point_id in point_set:
                continue
            point_set.add(point_id)
            if not _visible(model, T_root, point_id, cams):
                continue
            candidate_point_list.append(point_id)
            vertex_table.add(int(model.pt[point_id]["kf_index"]))
    return point_set, candidate_point_list, vertex_table


def literal_loop(model, cam, loop_kf, T_loop, query_kf, rng=None):
    """globalLoopClosure's loop (:847-893)"""
    cams = M.level_cams(cam)
    table = model.feature_table(query_kf)
    if rng is not None:
        table = [table[i] for i in rng.permutation(len(table))]
    vertex_table = {loop_kf}
    candidate_point_list = []
    for point_id in table:
        if not _visible(model, T_loop, point_id, cams):
            continue
        candidate_point_list.append(point_id)
        vertex_table.add(int(model.pt[point_id]["kf_index"]))
    return set(table), candidate_point_list, vertex_table


# ---- the scene of tests/register_model.make_scene() as a map ----------------------------------------------------------------------------------------------------
ROOT_ID, ROOT2_ID, OFFWALK_ID, FEW_ID, ALL_ID = 40, 41, 3, 50, 52


def scene_ids(scene):
    """table entry e of the scene -> keyframe id: the root is NOT the smallest id, the others ascend with their entry, so that the request the map builds for the
    scene's own neighbourhood is the scene itself"""
    n = len(scene["kf_T"])
    return [ROOT_ID] + [7 + 6 * k for k in range(n - 1)]


def fill(target, scene, cand_ids_few=(), attach=None):
    """Puts the scene into `target` (a MapModel or anything with its update methods) and returns the update calls made, as (name, args) -- for replaying them in
    another order.  Beyond the scene's own keyframes (ids scene_ids) and points (ids = their point_id, 1000 ..):
        ROOT2_ID     a second root: the root's twin
        OFFWALK_ID   a keyframe no walk names, with points 600 .. only it observes
        500 .. 505   points anchored in the direct neighbour and observed by direct neighbours only (the root and it)
        FEW_ID       observes the points cand_ids_few
        ALL_ID       observes every point of the scene
    attach(entry) -> dict of per-keyframe extras (images) for table entry `entry` of the scene"""
    ids = scene_ids(scene)
    n = len(ids)
    attach = attach or (lambda e: {})
    calls = []
    extra = [(ROOT2_ID, 0), (OFFWALK_ID, 1), (FEW_ID, 1), (ALL_ID, 1)]
    kf_ids = ids + [k for k, _ in extra]
    entries = list(range(n)) + [e for _, e in extra]
    att = [attach(e) for e in entries]
    calls.append(("add_keyframes", (kf_ids, [scene["kf_T"][e] for e in entries]), {k: [a[k] for a in att] for k in (att[0] if att else {})}))
    src = scene["src"]
    pts = np.array(src)
    pts["kf_index"] = [ids[int(e)] for e in src["kf_index"]]
    calls.append(("add_points", ([int(p) for p in src["point_id"]], pts), {}))
    direct_only = np.array(src[:6]); direct_only["kf_index"] = ids[1]
    calls.append(("add_points", (list(range(500, 506)), direct_only), {}))
    off = np.array(src[6:14]); off["kf_index"] = OFFWALK_ID
    calls.append(("add_points", (list(range(600, 608)), off), {}))
    op, ok = [], []
    for i, p in enumerate(src):
        for e in scene["obs_kf"][scene["obs_begin"][i]:scene["obs_begin"][i + 1]]:
            op.append(int(p["point_id"])); ok.append(ids[int(e)])
        op.append(int(p["point_id"])); ok.append(ALL_ID)
    for p in range(500, 506):
        op.append(p); ok.append(ids[1])
        if p & 1:
            op.append(p); ok.append(ids[0])
    for p in range(600, 608):
        op.append(p); ok.append(OFFWALK_ID)
    for p in cand_ids_few:
        op.append(int(p)); ok.append(FEW_ID)
    calls.append(("add_observations", (op, ok), {}))
    window = [ids[e] for e in range(n) if int(scene["flags"][e]) & M.IN_WINDOW] + [ROOT2_ID]
    calls.append(("set_window", (window,), {}))
    for name, args, kw in calls:
        getattr(target, name)(*args, **kw)
    return calls


def scene_request(scene, mode, root=ROOT_ID):
    """the scene's own neighbourhood by ids: LOCAL -- walk = every keyframe of the scene, direct = the root and entry 1; LOOP -- the query keyframe ALL_ID"""
    ids = scene_ids(scene)
    if mode == M.LOCAL:
        return dict(mode=mode, root_kf=root, T_root_from_world=scene["T_root"], walk_kf=[root] + ids[1:], direct_kf=[root, ids[1]])
    return dict(mode=mode, root_kf=root, T_root_from_world=scene["T_root"], walk_kf=[ALL_ID], direct_kf=[])
