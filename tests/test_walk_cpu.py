"""CPU tests of tests/walk_model.py: the model (adjacency rows from the edge table in descending (strength, slot); an ordinary breadth-first search with
first-claim-wins) against a literal restatement of the reference's loops -- the queue that holds duplicates and drops them at pop, the per-vertex multimap
neighbor_ids_ordered_by_strength walked rbegin() .. rend(), the PathTraversalNode / ReinitializeTraversalNode copies (slam_graph.cpp:64-140, :555-596, :665-725,
:762-782, slam_graph.hpp:501-533, backend.cpp:287-309).  Edges enter through addNewEdges, registerKeyframes and addLoopClosure, with many equal strengths."""
import bisect
from collections import deque

import numpy as np
import pytest

import constraint_model as CM
import walk_model as WM
from register_model import pose_inv, pose_mul

LOCAL, METRIC, APPEARANCE = 0, 1, 2
COVIS_THR = 3


class RefGraph:
    """the reference's SlamGraph as far as the walks read it"""

    def __init__(self):
        self.T = {}                        # vertex_table_[id].T_me_from_world
        self.nbrs = {}                     # vertex_table_[id].neighbor_ids_ordered_by_strength: a multimap as a list kept sorted by key, stable
        self.edge_table = CM.EdgeTable()
        self.double_window = {}            # id -> type, in insertion order

    @staticmethod
    def multimap_insert(mm, key, value):
        """std::multimap::insert: behind every element with an equal key"""
        mm.insert(bisect.bisect_right([k for k, _ in mm], key), (key, value))

    def add_vertex(self, v, T):
        self.T[v] = [float(x) for x in T]
        self.nbrs[v] = []

    def add_new_edges(self, neighborid_to_strength, edge_type, newkey):
        """:423-465, in the table's iteration order"""
        for other, strength in neighborid_to_strength:
            if strength >= COVIS_THR:
                self.multimap_insert(self.nbrs[other], strength, newkey)
                self.multimap_insert(self.nbrs[newkey], strength, other)
                self.edge_table.insert(other, newkey, strength, edge_type)

    def register_keyframes(self, root, neighborid_to_strength):
        """:188-205"""
        self.add_new_edges(neighborid_to_strength, METRIC, root)

    def add_loop_closure(self, root, loop, strength):
        """:207-251"""
        self.multimap_insert(self.nbrs[loop], strength, root)
        self.multimap_insert(self.nbrs[root], strength, loop)
        self.edge_table.insert(root, loop, strength, APPEARANCE)

    def rbegin_to_rend(self, v):
        return [value for _, value in reversed(self.nbrs[v])]

    # ---- the walks, loop by loop
    def shortest_path_to_window(self, root):
        """:64-103 with PathTraversalNode (hpp:501-513): the constructor copies the parent's path and appends own_id"""
        queue = deque([(root, [root])])
        vertex_set = set()
        while queue:
            own, path_to_me = queue.popleft()
            if own in self.double_window:
                return list(path_to_me)
            if own in vertex_set:
                continue
            vertex_set.add(own)
            for nb in self.rbegin_to_rend(own):
                queue.append((nb, list(path_to_me) + [nb]))
        return None

    def frames_in_neighborhood(self, root, size):
        """:105-140; the set is returned with its insertion order"""
        queue = deque([root])
        vertex_set = {}
        while queue and len(vertex_set) < size:
            leaf = queue.popleft()
            if leaf in vertex_set:
                continue
            if leaf not in self.double_window:
                continue
            vertex_set[leaf] = True
            queue.extend(self.rbegin_to_rend(leaf))
        return list(vertex_set)

    def compute_initial_double_win(self, root, inner_size, double_size):
        """:555-596 -> (ids in insertion order, types)"""
        assert inner_size < double_size
        win = {}
        queue = deque([root])
        while len(win) < double_size and queue:
            leaf = queue.popleft()
            if leaf in win:
                continue
            win[leaf] = CM.INNER if len(win) < inner_size else CM.OUTER
            queue.extend(self.rbegin_to_rend(leaf))
        return list(win), list(win.values())

    def get_relative_pose_1_from_2(self, id1, id2):
        """:271-286"""
        T, _, marg = self.edge_table.get_1_from_2(id1, id2)
        if marg:
            return [float(v) for v in T]
        return pose_mul(self.T[id1], pose_inv(self.T[id2]))

    def compute_absolute_pose(self, x):
        """:762-782"""
        path = self.shortest_path_to_window(x)
        if path is None:
            return None, None
        it = len(path) - 1
        cur = path[it]
        T = list(self.T[cur])
        it -= 1
        while it >= 0:
            new = path[it]
            T = pose_mul(self.get_relative_pose_1_from_2(new, cur), T)
            cur = new
            it -= 1
        return path, T

    def reinitialize_poses(self, root, old_window, loop_id):
        """:665-725 with ReinitializeTraversalNode (hpp:515-533): the node carries a COPY of the parent's pose; changes self.T; -> the changed ids in order"""
        queue = deque([(root, -1, [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], False)])
        cycle_check = set()
        changed = []
        while queue:
            own, parent, T_parent_from_world, mark_reinitialize = queue.popleft()
            if own in cycle_check:
                continue
            if own not in self.double_window:
                continue
            cycle_check.add(own)
            reinitialize_me_and_my_childs = bool(mark_reinitialize or own == loop_id)
            if parent > -1 and (reinitialize_me_and_my_childs or own not in old_window):
                self.T[own] = pose_mul(self.get_relative_pose_1_from_2(own, parent), T_parent_from_world)
                changed.append(own)
            for nb in self.rbegin_to_rend(own):
                queue.append((nb, own, list(self.T[own]), reinitialize_me_and_my_childs))
        return changed

    def find_neighbors_of_root(self, root, max_num_neighbors):
        """backend.cpp:287-309: forwards, and the count is compared before it is incremented"""
        out, count = [], 0
        for _, frame in self.nbrs[root]:
            if frame in self.double_window:
                out.append(frame)
                if count >= max_num_neighbors:
                    return out
                count += 1
        return out


def _pose(rng):
    from scavislam_amd import synth
    return [float(v) for v in synth.pose(synth.so3_exp(rng.normal(0, 0.3, 3)), rng.normal(0, 1, 3)).reshape(12)]


def _random_graph(seed):
    """a graph grown as the back end grows it: keyframes by addNewEdges (LOCAL), then registerKeyframes and addLoopClosure between existing ones; strengths from
    a handful of values, some below covis_thr; ids are not contiguous; some edges marginalised with a pose that is not the product of the vertex poses"""
    rng = np.random.default_rng(seed)
    g = RefGraph()
    n = int(rng.integers(4, 28))
    ids = [int(v) for v in rng.permutation(3 * n)[:n] + 7]
    components = int(rng.integers(1, 3))
    for k, v in enumerate(ids):
        g.add_vertex(v, _pose(rng))
        if k < components:
            continue                                       # a vertex without edges starts a component (or stays alone)
        others = [int(o) for o in rng.permutation(ids[:k])[:int(rng.integers(1, 5))]]
        g.add_new_edges([(o, int(rng.integers(2, 6))) for o in others], LOCAL, v)
    for _ in range(int(rng.integers(0, n))):
        a, b = (int(v) for v in rng.permutation(ids)[:2])
        if CM.EdgeTable.key(a, b) in g.edge_table.e:
            continue
        if rng.integers(2):
            g.register_keyframes(a, [(b, int(rng.integers(2, 6)))])
        else:
            g.add_loop_closure(a, b, int(rng.integers(COVIS_THR, 6)))
    for (lo, hi) in list(g.edge_table.e):
        if rng.integers(3) == 0:
            g.edge_table.set_constraint(lo, hi, _pose(rng), np.eye(6).reshape(36))
    share = (0.1, 0.3, 0.7)[seed % 3]                      # sparse windows give long paths and components without a window keyframe
    window = [v for v in ids if rng.uniform() < share]
    g.double_window = {v: 0 for v in window}
    return g, ids, rng


def _compare(g, ids, rng, adj):
    """every walk of the model (over `adj`) against the literal loops; returns the first difference as a string, or None"""
    window = list(g.double_window)
    pose0 = {k: list(v) for k, v in g.T.items()}
    for root in ids:
        for inner, double in ((1, 2), (2, 5), (3, len(ids)), (len(ids), len(ids) + 3)):
            if g.compute_initial_double_win(root, inner, double) != WM.initial_window(adj, root, inner, double):
                return "initial window %d %d %d" % (root, inner, double)
        for size in (1, 3, len(ids) + 1):
            if g.frames_in_neighborhood(root, size) != WM.frames_in_neighborhood(adj, window, root, size):
                return "neighbourhood %d %d" % (root, size)
        path, T = g.compute_absolute_pose(root)
        status, mpath, mT = WM.absolute_pose(adj, window, g.edge_table, pose0, root)
        if path is None:
            if status != WM.WALK_NO_PATH:
                return "path %d: none expected" % root
        elif status != WM.WALK_OK or mpath != path or np.array(mT).tobytes() != np.array(T).tobytes():
            return "path %d" % root
        for mx in (0, 1, 3):
            if g.find_neighbors_of_root(root, mx) != WM.neighbors_of_root(adj, window, root, mx):
                return "neighbours of root %d %d" % (root, mx)
    for _ in range(3):
        root = int(rng.choice(ids))
        old = [v for v in window if rng.integers(2)]
        loop_id = int(rng.choice(ids)) if rng.integers(2) else -1
        changed_m, pose_m = WM.reinitialize_poses(adj, window, g.edge_table, pose0, root, old, loop_id)
        changed = g.reinitialize_poses(root, set(old), loop_id)
        same = changed == changed_m and all(np.array(g.T[k]).tobytes() == np.array(pose_m[k]).tobytes() for k in ids)
        g.T = {k: list(v) for k, v in pose0.items()}
        if not same:
            return "reinitialise %d %d" % (root, loop_id)
    return None


SEEDS = range(300)


def test_model_equals_the_literal_loops_on_random_graphs():
    seen = dict(paths=0, no_path=0, long=0, ties=0)
    for seed in SEEDS:
        g, ids, rng = _random_graph(seed)
        adj = WM.adjacency(g.edge_table)
        # fact 1: the rows are the multimaps walked backwards
        for v in ids:
            assert [u for u, _ in adj.get(v, ())] == g.rbegin_to_rend(v), (seed, v)
            strengths = [k for k, _ in g.nbrs[v]]
            seen["ties"] += len(strengths) - len(set(strengths))
        assert _compare(g, ids, rng, adj) is None, seed
        for v in ids:
            p = g.shortest_path_to_window(v)
            seen["no_path" if p is None else "paths"] += 1
            seen["long"] += p is not None and len(p) >= 3
    assert seen["paths"] > 1000 and seen["no_path"] > 50 and seen["long"] > 100 and seen["ties"] > 1000, seen


def _adjacency_variant(table, tie_by_id=False, ascending=False):
    rows = {}
    for slot, ((lo, hi), e) in enumerate(table.e.items()):
        rows.setdefault(lo, []).append((e["strength"], hi if tie_by_id else slot, slot, hi))
        rows.setdefault(hi, []).append((e["strength"], lo if tie_by_id else slot, slot, lo))
    return {v: [(u, slot) for _, _, slot, u in sorted(r, reverse=not ascending)] for v, r in rows.items()}


@pytest.mark.parametrize("variant", [dict(tie_by_id=True), dict(ascending=True)])
def test_a_wrong_row_order_is_noticed(variant):
    """ties ordered by id instead of by slot, or ascending rows: the comparison must fail on a good share of the graphs"""
    wrong = 0
    for seed in range(60):
        g, ids, rng = _random_graph(seed)
        wrong += _compare(g, ids, rng, _adjacency_variant(g.edge_table, **variant)) is not None
    assert wrong >= 20, wrong


def test_model_equals_the_literal_loops_on_the_scene():
    sc = WM.scene()
    nm = sc["names"]
    g = RefGraph()
    for k in sc["kf_ids"]:
        g.add_vertex(k, sc["poses"][k])
    for a, b, st, ty in sc["edges"]:       # one edge per addNewEdges call: the insertion order is the list's
        g.add_new_edges([(a, st)], ty, b)
    for lo, hi, T, info in sc["marg"]:
        g.edge_table.set_constraint(lo, hi, T, info)
    assert list(g.edge_table.e) == list(sc["table"].e)
    adj = WM.adjacency(sc["table"])
    assert len(adj[nm["h300"]]) == 300 and len(adj[nm["h230"]]) == 230 and len(adj[nm["h65"]]) == 65 and nm["iso"] not in adj
    window = [nm[k] for k in ("t0", "t1", "t2", "R", "gw", "ga", "gb", "pw", "qw", "gn", "h65")]
    g.double_window = {v: 0 for v in window}
    for root in (nm["R"], nm["iso"], nm["h300"], nm["t0"], nm["s0"]):
        for inner, double in ((1, 2), (3, 7), (25, 200), (100, 600), (700, 900)):
            assert g.compute_initial_double_win(root, inner, double) == WM.initial_window(adj, root, inner, double), (root, inner, double)
    # the level behind the two hubs
    ids, _ = WM.initial_window(adj, nm["R"], 1, 900)
    assert len(ids) == len(sc["kf_ids"]) - 1 - 5 - 14      # all but iso, the second component and the gadgets (5 + 3 + 6 keyframes of their own)
    for x in (nm["c0"], nm["c17"], nm["gm_lo"], nm["gm_hi"], nm["gu"], nm["gx"], nm["gy"], nm["leaf300"], nm["s4"], nm["iso"], nm["R"]):
        path, T = g.compute_absolute_pose(x)
        status, mpath, mT = WM.absolute_pose(adj, window, sc["table"], sc["poses"], x)
        assert (path is None and status == WM.WALK_NO_PATH) or (mpath == path and np.array(mT).tobytes() == np.array(T).tobytes()), x
    assert WM.shortest_path_to_window(adj, window, nm["c0"]) == sc["chain"] and len(sc["chain"]) == 41
    assert WM.shortest_path_to_window(adj, window, nm["gy"]) == [nm["gy"], nm["q1"], nm["qw"]]
    assert WM.shortest_path_to_window(adj, window, nm["s4"]) is None
    for root in window + [nm["gu"]]:
        for size in (1, 4, 40):
            assert g.frames_in_neighborhood(root, size) == WM.frames_in_neighborhood(adj, window, root, size)
        for mx in (0, 2, 40):
            assert g.find_neighbors_of_root(root, mx) == WM.neighbors_of_root(adj, window, root, mx)
    assert nm["gn"] not in WM.frames_in_neighborhood(adj, window, nm["gw"], 40)
    big = [k for k in sc["kf_ids"]]
    g.double_window = {v: 0 for v in big}
    pose0 = {k: list(v) for k, v in g.T.items()}
    for loop_id in (-1, nm["h300"], nm["R"], nm["c20"]):
        old = big[::2]
        changed_m, pose_m = WM.reinitialize_poses(adj, big, sc["table"], pose0, nm["R"], old, loop_id)
        changed = g.reinitialize_poses(nm["R"], set(old), loop_id)
        assert changed == changed_m and all(np.array(g.T[k]).tobytes() == np.array(pose_m[k]).tobytes() for k in big), loop_id
        g.T = {k: list(v) for k, v in pose0.items()}
