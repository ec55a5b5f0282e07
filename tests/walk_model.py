"""The pose graph's walks restated in plain Python -- the yardstick of svs_map_initial_windows, svs_map_frames_in_neighborhood, svs_map_absolute_poses,
svs_map_reinitialize_poses and svs_map_prepare_window_from_root -- over constraint_model.EdgeTable and register_model.pose_mul / pose_inv, the primitives the
byte-for-byte constraint tests rest on.

The reference (slam_graph.cpp:64-140, :555-596, :665-725) runs one breadth-first search with a queue that holds duplicates and a per-vertex multimap
neighbor_ids_ordered_by_strength walked from rbegin() to rend().  The model rests on the two facts include/scavislam_hip.h states:
    1. adjacency comes from the edge table: row(v) = v's edges in DESCENDING (strength, slot), slot = insertion order into the EdgeTable (a dict keeps it);
    2. visited-at-pop equals visited-at-push: the visit order is "frontier in order, each frontier vertex's row in order, first claim wins".
tests/test_walk_cpu.py holds both to a literal restatement of the reference's loops.
"""
import functools

import numpy as np

from constraint_model import EdgeTable, INNER, OUTER, kf_id
from register_model import pose_inv, pose_mul

WALK_OK, WALK_NO_PATH = 0, 1


def adjacency(table):
    """{v: [(neighbour, slot)] in descending (strength, slot)} from an EdgeTable; a vertex without an edge has no entry (use .get(v, ()))"""
    rows = {}
    for slot, ((lo, hi), e) in enumerate(table.e.items()):
        rows.setdefault(lo, []).append((e["strength"], slot, hi))
        rows.setdefault(hi, []).append((e["strength"], slot, lo))
    return {v: [(u, slot) for _, slot, u in sorted(r, reverse=True)] for v, r in rows.items()}


def visits(adj, root, admit=lambda v: True, expand=lambda v: True):
    """yields (vertex, parent or None) in visit order; `admit`: may the vertex be claimed at all, `expand`: is its row walked.  Lazy: the caller stops it"""
    parent = {root: None}
    order = [root]
    i = 0
    while i < len(order):
        f = order[i]
        i += 1
        yield f, parent[f]
        if not expand(f):
            continue
        for u, _ in adj.get(f, ()):
            if u not in parent and admit(u):
                parent[u] = f
                order.append(u)


def initial_window(adj, root, inner_size, double_size):
    """computeInitialDoubleWin -> (ids in visit order, types)"""
    assert inner_size < double_size
    ids = []
    for v, _ in visits(adj, root):
        ids.append(v)
        if len(ids) == double_size:
            break
    return ids, [INNER if i < inner_size else OUTER for i in range(len(ids))]


def frames_in_neighborhood(adj, window, root, size):
    """framesInNeighborhood -> ids in visit order (the reference returns them as a hash set)"""
    window = set(window)
    ids = []
    if root not in window or size < 1:
        return ids
    for v, _ in visits(adj, root, admit=lambda u: u in window):
        ids.append(v)
        if len(ids) == size:
            break
    return ids


def shortest_path_to_window(adj, window, x):
    """shortestPathToWindow -> [x, .., w] or None"""
    window = set(window)
    parent = {}
    for v, p in visits(adj, x, expand=lambda u: u not in window):
        parent[v] = p
        if v in window:
            path = [v]
            while parent[path[-1]] is not None:
                path.append(parent[path[-1]])
            return path[::-1]
    return None


def relative_pose(table, pose, id1, id2):
    """getRelativePose_1_from_2 (:271-286)"""
    T, _, marg = table.get_1_from_2(id1, id2)
    if marg:
        return [float(v) for v in T]
    return pose_mul(pose[id1], pose_inv(pose[id2]))


def absolute_pose(adj, window, table, pose, x):
    """computeAbsolutePose (:762-782) -> (status, path, T [12])"""
    path = shortest_path_to_window(adj, window, x)
    if path is None:
        return WALK_NO_PATH, [], [0.0] * 12
    cur = path[-1]
    T = [float(v) for v in pose[cur]]
    for new in path[-2::-1]:
        T = pose_mul(relative_pose(table, pose, new, cur), T)
        cur = new
    return WALK_OK, path, T


def reinitialize_poses(adj, window, table, pose, root, old_window, loop_id=-1):
    """reinitializePoses (:665-725) on a copy of `pose` -> (changed ids in visit order, the new pose table)"""
    window, old_window = set(window), set(old_window)
    pose = {k: [float(v) for v in T] for k, T in pose.items()}
    changed, mark = [], {}
    if root not in window:
        return changed, pose
    for v, p in visits(adj, root, admit=lambda u: u in window):
        mark[v] = (p is not None and mark[p]) or v == loop_id
        if p is not None and (mark[v] or v not in old_window):
            pose[v] = pose_mul(relative_pose(table, pose, v, p), pose[p])
            changed.append(v)
    return changed, pose


def neighbors_of_root(adj, window, root, max_num_neighbors):
    """findNeighborsOfRoot (backend.cpp:287-309): the row walked FORWARDS (ascending (strength, slot)), in-window only; the count is compared before it is
    incremented, so up to max_num_neighbors + 1 ids come back"""
    window = set(window)
    out, count = [], 0
    for u, _ in reversed(adj.get(root, ())):
        if u in window:
            out.append(u)
            if count >= max_num_neighbors:
                return out
            count += 1
    return out


def inner_pairs(adj, ids, types):
    """the edge_table_ entries with at least one end in an INNER keyframe: the adjacency rows of the INNER keyframes (an edge between two of them comes twice)"""
    return [(v, u) for v, t in zip(ids, types) if t == INNER for u, _ in adj.get(v, ())]


# ---- the test scene ---------------------------------------------------------------------------------------------------------------------------------------------
# keyframe index i has id constraint_model.kf_id(i) = 100 + 3 i.  `names` maps the named keyframes to ids.
CHAIN = 40
HUBS = dict(h65=65, h230=230, h300=300)


def _pose(rng):
    from scavislam_amd import synth
    return [float(v) for v in synth.pose(synth.so3_exp(rng.normal(0, 0.3, 3)), rng.normal(0, 1.5, 3)).reshape(12)]


@functools.lru_cache(maxsize=None)
def scene(seed=11):
    """-> dict(kf_ids, poses {id: [12]}, edges [(a, b, strength, type)] in insertion order, marg [(lo, hi, T_lo_from_hi, info)], names, table).
    Shared: treat it as read-only (table_copy() for a test that changes edges).
      iso                  an isolated keyframe
      t0 t1 t2             a triangle; R hangs on t0
      R                    adjacent to the hubs h300 and h230: the level behind them holds 299 + 229 = 528 keyframes (> 512)
      h65                  a hub of degree 65 on t1 (longer than a wave), h300 (longer than a 256-lane pass)
      c0 .. c39            a chain, c39 on t2; its edges alternate marginalised / not, the ids along it are shuffled so that the walk meets the stored pose as lo
                           and as hi; the stored poses are random, not the product of the vertex poses
      g*                   small gadgets for the path cases (see names)
      s0 .. s4             a second component
    Strengths come in runs of equal values; the insertion order is shuffled, so slot order is not id order."""
    rng = np.random.default_rng(seed)
    n_idx = [0]
    names = {}

    def new(name=None):
        i = n_idx[0]
        n_idx[0] += 1
        if name:
            names[name] = i
        return i

    E = []                                # (index a, index b, strength, type)
    iso = new("iso")
    t = [new("t%d" % k) for k in range(3)]
    E += [(t[0], t[1], 30, 0), (t[1], t[2], 30, 0), (t[2], t[0], 25, 0)]
    R = new("R")
    E.append((t[0], R, 30, 0))
    # the chain gets indices first and a shuffled assignment, so that ids go up and down along it
    chain_idx = [new() for _ in range(CHAIN)]
    chain = [chain_idx[k] for k in rng.permutation(CHAIN)]
    for k, c in enumerate(chain):
        names["c%d" % k] = c
    for k in range(CHAIN - 1):
        E.append((chain[k], chain[k + 1], 20 + (k % 3), 0))
    E.append((chain[-1], t[2], 22, 0))
    hubs = {}
    for name, deg in HUBS.items():
        h = new(name)
        at = R if name != "h65" else t[1]
        E.append((at, h, 28, 1))
        leaves = [new() for _ in range(deg - 1)]
        hubs[name] = leaves
        for j, l in enumerate(leaves):
            E.append((h, l, 15 + (j // 7) % 5, j % 3))       # runs of seven equal strengths, five values
    names["leaf300"], names["leaf230"], names["leaf65"] = hubs["h300"][17], hubs["h230"][100], hubs["h65"][64 - 1]
    # gadgets.  gw: a window keyframe with three non-window neighbours: gm_lo < gw < gm_hi across marginalised edges, gu across an unmarginalised one
    gm_lo, gw, gm_hi, gu = new("gm_lo"), new("gw"), new("gm_hi"), new("gu")
    E += [(gm_lo, gw, 12, 0), (gm_hi, gw, 12, 0), (gu, gw, 12, 0)]
    # gx sees two window keyframes at equal depth across equal strengths: the later slot is reached first
    gx, ga, gb = new("gx"), new("ga"), new("gb")
    E += [(gx, ga, 18, 0), (gx, gb, 18, 0)]
    # gy: a strong edge into a long path (gy - p1 - p2 - pw) and a weak one into a short path (gy - q1 - qw): hops decide, not strength
    gy, p1, p2, pw, q1, qw = new("gy"), new("p1"), new("p2"), new("pw"), new("q1"), new("qw")
    E += [(gy, p1, 90, 0), (p1, p2, 90, 0), (p2, pw, 90, 0), (gy, q1, 11, 0), (q1, qw, 11, 0)]
    # gn: a window keyframe that is reachable from gw only through the non-window gu
    gn = new("gn")
    E.append((gu, gn, 12, 0))
    s = [new("s%d" % k) for k in range(5)]
    E += [(s[0], s[1], 14, 0), (s[1], s[2], 14, 0), (s[1], s[3], 14, 0), (s[3], s[4], 13, 0)]
    n = n_idx[0]
    fixed = len(E)
    E = [E[k] for k in rng.permutation(fixed)]
    kf_ids = [kf_id(i) for i in range(n)]
    poses = {kf_id(i): _pose(rng) for i in range(n)}
    edges = [(kf_id(a), kf_id(b), st, ty) if rng.integers(2) else (kf_id(b), kf_id(a), st, ty) for a, b, st, ty in E]
    table = EdgeTable()
    for a, b, st, ty in edges:
        table.insert(a, b, st, ty)
    marg = []
    cid = [kf_id(c) for c in chain] + [kf_id(t[2])]
    for k in range(0, CHAIN, 2):          # every second chain edge
        marg.append((min(cid[k], cid[k + 1]), max(cid[k], cid[k + 1])))
    marg += [(kf_id(gm_lo), kf_id(gw)), (kf_id(gw), kf_id(gm_hi))]
    marg = [(lo, hi, _pose(rng), np.diag(rng.uniform(1, 9, 6)).reshape(36)) for lo, hi in marg]
    for lo, hi, T, info in marg:
        table.set_constraint(lo, hi, T, info)
    names = {k: kf_id(v) for k, v in names.items()}
    return dict(kf_ids=kf_ids, poses=poses, edges=edges, marg=marg, names=names, table=table, chain=cid, hubs={k: [kf_id(l) for l in v] for k, v in hubs.items()})


def table_copy(sc):
    t = EdgeTable()
    for a, b, st, ty in sc["edges"]:
        t.insert(a, b, st, ty)
    for lo, hi, T, info in sc["marg"]:
        t.set_constraint(lo, hi, T, info)
    return t
