"""GPU tests of the pose graph's walks on the device-resident map: svs_map_initial_windows, svs_map_frames_in_neighborhood, svs_map_absolute_poses,
svs_map_reinitialize_poses, svs_map_prepare_window_from_root against tests/walk_model.py, byte for byte (tests/test_walk_cpu.py holds the model to the
reference's loops).  The map is walk_model.scene(): about 660 keyframes with non-contiguous ids -- the level behind the hubs h300 and h230 has to exceed 512
keyframes, which about 400 could not hold -- hubs of degree 65, 230 and 300, a chain of 40 with marginalised edges in both orientations, runs of equal strengths,
a second component, an isolated keyframe."""
import os
import subprocess

import numpy as np
import pytest

import constraint_model as CM
import walk_model as WM

CAPS = dict(max_keyframes=2304, max_points=8192, max_observations=256)
WINDOW_A = ("t0", "t1", "t2", "R", "gw", "ga", "gb", "pw", "qw", "gn", "h65")


@pytest.fixture(scope="module")
def sc():
    return WM.scene()


@pytest.fixture(scope="module")
def adj(sc):
    return WM.adjacency(sc["table"])


@pytest.fixture(scope="module")
def blank(gpu_ctx):
    """one blank pyramid and disparity for every keyframe: the walks never read them"""
    import torch
    ctx, stream = gpu_ctx
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((48 >> l, 64 >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((48, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    return pyr, disp


def _build(ctx, blank, sc, spare_edges=8):
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE, CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    pyr, disp = blank
    d = ResidentMap(ctx, **CAPS)
    ids = sc["kf_ids"]
    kfs = keyframe_table([([t.data_ptr() for t in pyr], [t.shape[1] for t in pyr], sc["poses"][k]) for k in ids])
    d.add_keyframes(ids, kfs, [(disp.data_ptr(), disp.shape[1])] * len(ids), [[[25], [25], [25]]] * len(ids))
    pts = np.zeros(8, CANDIDATE_DTYPE)                           # a handful of points
    pts["xyz_anchor"], pts["kf_index"] = [[0.1 * j, -0.2, 3.0 + j] for j in range(8)], [ids[j] for j in range(8)]
    d.add_points(5000 + 7 * np.arange(8), pts)
    d.add_observations(5000 + 7 * np.arange(8), ids[:8])
    d.reserve_edges(len(sc["edges"]) + spare_edges)
    d.add_edges([(a, b) for a, b, _, _ in sc["edges"]], [s for _, _, s, _ in sc["edges"]], [t for _, _, _, t in sc["edges"]])
    cons = np.zeros(len(sc["marg"]), BA_CONSTRAINT_DTYPE)
    for c, (lo, hi, T, info) in zip(cons, sc["marg"]):         # pose1 > pose2: T_21 is T_lo_from_hi as it is stored
        c["T_21"], c["info"], c["pose1"], c["pose2"] = T, info, hi, lo
    d.set_constraints(cons)
    return d


@pytest.fixture(scope="module")
def dmap(gpu_ctx, blank, sc):
    d = _build(gpu_ctx[0], blank, sc)
    yield d
    d.close()


def _poses_bytes(pose, ids):
    return np.array([pose[k] for k in ids], np.float64).tobytes()


def _row(ids, cap):
    r = np.full(cap, -1, np.int32)
    r[:min(len(ids), cap)] = ids[:cap]
    return r


@pytest.mark.gpu
def test_the_map_holds_the_model_s_edges(dmap, sc):
    keys = list(sc["table"].e)
    assert dmap.get_edges(keys).tobytes() == np.array([sc["table"].record(a, b) for a, b in keys]).tobytes()
    assert dmap.get_poses(sc["kf_ids"]).tobytes() == _poses_bytes(sc["poses"], sc["kf_ids"])


@pytest.mark.gpu
def test_initial_windows(dmap, sc, adj):
    nm = sc["names"]
    roots = [nm[k] for k in ("R", "iso", "h300", "t0", "s0", "c0", "leaf65")]
    leaves = set(sc["hubs"]["h300"]) | set(sc["hubs"]["h230"])
    for inner, double in ((1, 2), (3, 7), (25, 200), (100, 600), (700, 900)):
        got = dmap.initial_windows(roots, inner, double)
        raw = {k: v.copy() for k, v in dmap.raw.items()}
        for i, root in enumerate(roots):
            ids, types = WM.initial_window(adj, root, inner, double)
            assert got[i][0].tolist() == ids and got[i][1].tolist() == types, (root, inner, double)
            assert np.array_equal(raw["ids"][i], _row(ids, double)) and np.array_equal(raw["types"][i], _row(types, double)), (root, inner, double)
        for i in (0, 2, 5):                                        # each alone gives the bytes it has in the batch
            dmap.initial_windows([roots[i]], inner, double)
            assert dmap.raw["ids"][0].tobytes() == raw["ids"][i].tobytes() and dmap.raw["types"][0].tobytes() == raw["types"][i].tobytes()
    # R: 3 neighbours, then the level of 528 behind the hubs -- 200 ends inside a hub's row and inside that level, and the INNER boundary at 25 too
    (ids, types), (iso_ids, _), (hub_ids, _) = dmap.initial_windows([nm["R"], nm["iso"], nm["h300"]], 25, 200)
    assert len(ids) == 200 and set(ids[6:].tolist()) <= leaves and types.tolist() == [0] * 25 + [1] * 175
    assert iso_ids.tolist() == [nm["iso"]] and hub_ids[0] == nm["h300"] and len(hub_ids) == 200
    # a double window larger than the component: the whole component, once
    (ids, _), = dmap.initial_windows([nm["s0"]], 2, 64, window_cap=80)
    assert sorted(ids.tolist()) == sorted(nm["s%d" % k] for k in range(5)) and dmap.raw["ids"].shape == (1, 80)


@pytest.mark.gpu
def test_frames_in_neighborhood(dmap, sc, adj):
    nm = sc["names"]
    window = [nm[k] for k in WINDOW_A]
    dmap.set_window(window)
    roots = [nm[k] for k in ("gu", "gw", "t0", "R", "h65", "t1", "iso")]
    for size in (1, 4, 40):
        got = dmap.frames_in_neighborhood(roots, size)
        raw = dmap.raw["ids"].copy()
        for i, root in enumerate(roots):
            want = WM.frames_in_neighborhood(adj, window, root, size)
            assert got[i].tolist() == want and np.array_equal(raw[i], _row(want, size)), (root, size)
        for i in (1, 2):
            dmap.frames_in_neighborhood([roots[i]], size)
            assert dmap.raw["ids"][0].tobytes() == raw[i].tobytes()
    got = dmap.frames_in_neighborhood(roots, 40)
    assert len(got[0]) == 0 and len(got[6]) == 0                   # roots outside the window
    assert got[1].tolist() == [nm["gw"]]                           # gn is in the window, but reachable only through gu, which is not
    assert set(got[2].tolist()) == {nm[k] for k in ("t0", "t1", "t2", "R", "h65")}      # size beyond the reachable set
    # the same window through a larger one: every keyframe
    dmap.set_window(sc["kf_ids"])
    (ids,), want = dmap.frames_in_neighborhood([nm["R"]], 600), WM.frames_in_neighborhood(adj, sc["kf_ids"], nm["R"], 600)
    assert ids.tolist() == want and len(want) == 600


@pytest.mark.gpu
def test_absolute_poses(dmap, sc, adj):
    nm = sc["names"]
    window = [nm[k] for k in WINDOW_A]
    dmap.set_window(window)
    xs = [nm[k] for k in ("t0", "gm_lo", "gm_hi", "gu", "c0", "c17", "gx", "gy", "s4", "iso", "leaf300", "leaf65", "R", "h300")]
    want = [WM.absolute_pose(adj, window, sc["table"], sc["poses"], x) for x in xs]
    for cap in (64, 3, 0):
        got = dmap.absolute_poses(xs, path_cap=cap)
        raw = {k: v.copy() for k, v in dmap.raw.items()}
        for i, (x, (status, path, T)) in enumerate(zip(xs, want)):
            assert got[i]["status"] == status and got[i]["path_len"] == len(path), (x, cap)
            assert raw["T"][i].tobytes() == np.array(T, np.float64).tobytes(), (x, cap, raw["T"][i], T)
            if cap:
                assert np.array_equal(raw["path"][i], _row(path, cap)), (x, cap)
        for i in (1, 4, 7, 8):
            dmap.absolute_poses([xs[i]], path_cap=cap)
            assert all(dmap.raw[k][0].tobytes() == raw[k][i].tobytes() for k in raw), (xs[i], cap)
    got = dict(zip(("t0", "gm_lo", "gm_hi", "gu", "c0", "c17", "gx", "gy", "s4", "iso", "leaf300", "leaf65", "R", "h300"), dmap.absolute_poses(xs, path_cap=64)))
    # in the window: the stored bytes
    assert got["t0"]["path"].tolist() == [nm["t0"]] and got["t0"]["T"].tobytes() == np.array(sc["poses"][nm["t0"]]).tobytes()
    # one hop across a marginalised edge as lo and as hi, and across an unmarginalised one
    lo_hi = {(lo, hi): T for lo, hi, T, _ in sc["marg"]}
    assert nm["gm_lo"] < nm["gw"] < nm["gm_hi"]
    assert got["gm_lo"]["T"].tobytes() == np.array(CM.pose_mul(lo_hi[(nm["gm_lo"], nm["gw"])], sc["poses"][nm["gw"]])).tobytes()
    assert got["gm_hi"]["T"].tobytes() == np.array(CM.pose_mul(CM.pose_inv(lo_hi[(nm["gw"], nm["gm_hi"])]), sc["poses"][nm["gw"]])).tobytes()
    assert got["gu"]["path"].tolist() == [nm["gu"], nm["gw"]] or got["gu"]["path"].tolist() == [nm["gu"], nm["gn"]]
    # the chain: 41 keyframes, marginalised edges met from both sides
    assert got["c0"]["path"].tolist() == sc["chain"] and got["c0"]["path_len"] == 41
    sides = {a < b for a, b in zip(sc["chain"][0:-1:2], sc["chain"][1::2])}
    assert sides == {True, False}
    # two window keyframes at equal depth behind equal strengths: the later slot is reached first
    keys = list(sc["table"].e)
    later = max((nm["ga"], nm["gb"]), key=lambda k: keys.index(CM.EdgeTable.key(nm["gx"], k)))
    assert got["gx"]["path"].tolist() == [nm["gx"], later]
    # hops decide, not strength
    assert got["gy"]["path"].tolist() == [nm["gy"], nm["q1"], nm["qw"]]
    # no window keyframe in the component: status, zeros
    for k in ("s4", "iso"):
        assert got[k]["status"] == WM.WALK_NO_PATH and got[k]["path_len"] == 0 and not got[k]["T"].any() and len(got[k]["path"]) == 0
    assert got["leaf300"]["path"].tolist() == [nm["leaf300"], nm["h300"], nm["R"]]


@pytest.mark.gpu
def test_reinitialize_poses(gpu_ctx, blank, sc, adj):
    nm, ids = sc["names"], sc["kf_ids"]
    d = _build(gpu_ctx[0], blank, sc)
    start = _poses_bytes(sc["poses"], ids)
    h300, h230 = set(sc["hubs"]["h300"]), set(sc["hubs"]["h230"])
    small = list(dict.fromkeys([nm[k] for k in WINDOW_A] + sc["hubs"]["h65"][:40] + sc["chain"][30:]))      # (t2 ends the chain: once)
    cases = [("all, no loop", ids, ids[::2], nm["R"], -1), ("loop in the window", ids, ids, nm["R"], nm["h300"]), ("loop = root", ids, ids, nm["R"], nm["R"]),
             ("loop on the chain", ids, ids[::3], nm["t0"], nm["c20"]), ("a window with holes", small, small[::2], nm["t1"], -1),
             ("root outside the window", small, small, nm["c0"], -1)]
    for what, window, old, root, loop_id in cases:
        d.set_window(window)
        changed_m, pose_m = WM.reinitialize_poses(adj, window, sc["table"], sc["poses"], root, old, loop_id)
        changed, n = d.reinitialize_poses(root, old, loop_id)
        assert n == len(changed_m) and changed.tolist() == changed_m, what
        got = d.get_poses(ids)
        assert got.tobytes() == _poses_bytes(pose_m, ids), what
        keep = [i for i, k in enumerate(ids) if k not in set(changed_m)]
        assert got[keep].tobytes() == np.frombuffer(start, np.float64).reshape(-1, 12)[keep].tobytes(), what      # the untouched ones: the bytes they had
        assert root not in changed_m
        if what == "all, no loop":
            assert not set(changed_m) & set(old) and len(changed_m) > 250          # only keyframes outside the old window move
        if what == "loop in the window":
            assert set(changed_m) == h300 | {nm["h300"]} and not set(changed_m) & h230      # the whole subtree, no sibling
        if what == "loop = root":
            assert len(changed_m) == len(WM.initial_window(adj, root, 1, 4000)[0]) - 1      # everything reachable but the root
        if what == "root outside the window":
            assert n == 0
        # a short list of changed ids: the count is still the total
        d.set_poses(ids, np.frombuffer(start, np.float64).reshape(-1, 12))
        few, n2 = d.reinitialize_poses(root, old, loop_id, changed_cap=5)
        assert n2 == n and few.tolist() == changed_m[:5] and d.get_poses(ids).tobytes() == _poses_bytes(pose_m, ids), what
        d.set_poses(ids, np.frombuffer(start, np.float64).reshape(-1, 12))
    d.close()


@pytest.mark.gpu
def test_rebuild_after_add_edges(gpu_ctx, blank, sc):
    nm = sc["names"]
    d = _build(gpu_ctx[0], blank, sc)
    table = WM.table_copy(sc)
    d.set_window([nm["t0"]])
    assert d.initial_windows([nm["iso"]], 1, 5)[0][0].tolist() == [nm["iso"]] and d.absolute_poses([nm["iso"]])[0]["status"] == WM.WALK_NO_PATH
    new = [(nm["iso"], nm["t0"], 40, 2), (nm["s0"], nm["iso"], 40, 1), (nm["R"], nm["iso"], 7, 0)]
    d.add_edges([(a, b) for a, b, _, _ in new], [s for _, _, s, _ in new], [t for _, _, _, t in new])
    for a, b, s, t in new:
        table.insert(a, b, s, t)
    adj2 = WM.adjacency(table)
    (ids, types), = d.initial_windows([nm["iso"]], 2, 9)
    assert (ids.tolist(), types.tolist()) == WM.initial_window(adj2, nm["iso"], 2, 9) and ids[:3].tolist() == [nm["iso"], nm["s0"], nm["t0"]]
    status, path, T = WM.absolute_pose(adj2, [nm["t0"]], table, sc["poses"], nm["s4"])
    got = d.absolute_poses([nm["s4"]], path_cap=8)[0]
    assert status == WM.WALK_OK and got["path"].tolist() == path and got["T"].tobytes() == np.array(T).tobytes() and path[-2:] == [nm["iso"], nm["t0"]]
    assert d.neighbors_of_root(nm["iso"], 5).tolist() == WM.neighbors_of_root(adj2, [nm["t0"]], nm["iso"], 5) == [nm["t0"]]
    d.set_window(sc["kf_ids"])
    for mx in (0, 1, 5):
        assert d.neighbors_of_root(nm["iso"], mx).tolist() == WM.neighbors_of_root(adj2, sc["kf_ids"], nm["iso"], mx)
    assert len(d.neighbors_of_root(nm["iso"], 1)) == 2 and d.neighbors_of_root(nm["iso"], 5)[0] == nm["R"]      # the reference's off-by-one; ascending strength
    assert d.neighbors_of_root(nm["h300"], 400).tolist() == WM.neighbors_of_root(adj2, sc["kf_ids"], nm["h300"], 400)
    d.close()


@pytest.mark.gpu
def test_refusals_leave_the_map_unchanged(gpu_ctx, blank, sc, adj):
    from scavislam_amd.capi import SvsError
    nm, ids = sc["names"], sc["kf_ids"]
    d = _build(gpu_ctx[0], blank, sc)
    d.set_window([nm[k] for k in WINDOW_A])
    keys = list(sc["table"].e)
    unknown = ids[0] + 1

    def snapshot():
        return (d.get_poses(ids).tobytes(), d.get_edges(keys).tobytes(), d.edge_info(), d.info(), d.initial_windows([nm["R"]], 5, 40)[0][0].tobytes(),
                np.concatenate(d.frames_in_neighborhood([nm["t0"], nm["gu"]], 9)).tobytes())

    before = snapshot()
    INVALID, CAPACITY = 1, 4
    calls = [
        ("initial window: unknown root", lambda: d.initial_windows([nm["R"], unknown], 2, 5), INVALID),
        ("initial window: inner_size >= double_size", lambda: d.initial_windows([nm["R"]], 5, 5), INVALID),
        ("initial window: double_size above window_cap", lambda: d.initial_windows([nm["R"]], 2, 9, window_cap=8), CAPACITY),
        ("initial window: too many requests", lambda: d.initial_windows([nm["R"]] * 257, 2, 5), CAPACITY),
        ("neighbourhood: unknown root", lambda: d.frames_in_neighborhood([unknown], 4), INVALID),
        ("neighbourhood: size 0", lambda: d.frames_in_neighborhood([nm["R"]], 0), INVALID),
        ("neighbourhood: too many requests", lambda: d.frames_in_neighborhood([nm["R"]] * 257, 4), CAPACITY),
        ("absolute poses: unknown id", lambda: d.absolute_poses([nm["c0"], -1]), INVALID),
        ("absolute poses: too many requests", lambda: d.absolute_poses([nm["c0"]] * 257), CAPACITY),
        ("reinitialise: unknown root", lambda: d.reinitialize_poses(unknown, []), INVALID),
        ("reinitialise: unknown loop id", lambda: d.reinitialize_poses(nm["R"], [], loop_id=unknown), INVALID),
        ("reinitialise: unknown id in the old window", lambda: d.reinitialize_poses(nm["R"], [nm["t0"], unknown]), INVALID),
        ("reinitialise: an id twice in the old window", lambda: d.reinitialize_poses(nm["R"], [nm["t0"], nm["t0"]]), INVALID),
        ("window from root: unknown root", lambda: d.prepare_window_from_root(unknown, 2, 5), INVALID),
        ("window from root: inner_size >= double_size", lambda: d.prepare_window_from_root(nm["R"], 5, 4), INVALID),
        ("window from root: above the solve's limit", lambda: d.prepare_window_from_root(nm["R"], 5, 300, window_cap=300), CAPACITY),
        ("window from root: observations without a measurement", lambda: d.prepare_window_from_root(nm["R"], 2, 5), INVALID),
    ]
    for what, call, status in calls:
        with pytest.raises(SvsError, match="status %d" % status):
            call()
        assert snapshot() == before, what
    d.close()


@pytest.mark.gpu
def test_prepare_window_from_root_equals_prepare_window(gpu_ctx):
    """on constraint_model.scene()'s map, with a measurement for every observation: result, window lists, flags, and the BA window windowFromMap builds"""
    import torch
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE, CANDIDATE_DTYPE, Cam
    from scavislam_amd.register import ResidentMap, keyframe_table
    ctx, stream = gpu_ctx
    m = dict(CM.scene()["map"])
    rng = np.random.default_rng(3)
    m["obs_center"] = rng.uniform(20, 300, (len(m["obs_point"]), 3))
    m["obs_level"] = rng.integers(0, 3, len(m["obs_point"])).astype(np.int32)
    kf = [int(k) for k in m["kf_ids"]]
    table = CM.EdgeTable()
    edges = [(kf[i], kf[i + 1], 20 + i % 3) for i in range(len(kf) - 1)] + [(kf[0], kf[j], 21) for j in (2, 5, 9, 12, 16)] + [(kf[1], kf[j], 22) for j in (10, 13, 15)]
    edges = [edges[k] for k in rng.permutation(len(edges))]
    for a, b, s in edges:
        table.insert(a, b, s, 0)
    adj = WM.adjacency(table)
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((48 >> l, 64 >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((48, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    maps = []
    for _ in range(2):
        d = ResidentMap(ctx, max_keyframes=256, max_points=20000, max_observations=16384)
        kfs = keyframe_table([([t.data_ptr() for t in pyr], [t.shape[1] for t in pyr], T) for T in m["kf_poses"]])
        d.add_keyframes(m["kf_ids"], kfs, [(disp.data_ptr(), disp.shape[1])] * len(kfs), [[[25], [25], [25]]] * len(kfs))
        pts = np.zeros(len(m["point_ids"]), CANDIDATE_DTYPE)
        pts["xyz_anchor"], pts["kf_index"] = m["xyz"], m["anchor_ids"]
        d.add_points(m["point_ids"], pts)
        d.add_measured_observations(m["obs_point"], m["obs_kf"], m["obs_center"], m["obs_level"])
        d.reserve_edges(len(edges))
        d.add_edges([(a, b) for a, b, _ in edges], [s for _, _, s in edges], 0)
        maps.append(d)
    by_hand, from_root = maps
    cam = Cam(285.0, 160.0, 120.0, 0.075, 320, 240)
    in_window = lambda d: [len(w) for w in d.frames_in_neighborhood(kf, 1)]
    state = lambda o: tuple(x.tobytes() for x in o.restoreDataFromG2o()) + (o.window_edges().tobytes(),)
    extended = 0
    for root, inner, double in ((kf[0], 3, 6), (kf[1], 2, 4), (kf[9], 1, 2), (kf[4], 6, 19), (kf[16], 4, 40)):
        ids, types = WM.initial_window(adj, root, inner, double)
        pairs = WM.inner_pairs(adj, ids, types)
        r1, wid1, wtype1 = by_hand.prepare_window(ids, types, pairs)
        r2, wid2, wtype2 = from_root.prepare_window_from_root(root, inner, double)
        assert bytes(r1) == bytes(r2) and wid1.tobytes() == wid2.tobytes() and wtype1.tobytes() == wtype2.tobytes(), (root, inner, double)
        assert r2.n_initial == len(ids) and wid2[:len(ids)].tolist() == ids and in_window(by_hand) == in_window(from_root)
        assert sum(in_window(from_root)) == r2.n_window
        extended += r2.n_window > r2.n_initial
        a, b = SlamGraphOptimizer(ctx, stream), SlamGraphOptimizer(ctx, stream)
        a.windowFromMap(by_hand, np.zeros(0, BA_CONSTRAINT_DTYPE), cam)
        b.windowFromMap(from_root, np.zeros(0, BA_CONSTRAINT_DTYPE), cam)
        assert (a.P, a.L) == (b.P, b.L) == (r2.n_window, r2.n_active) and state(a) == state(b), (root, inner, double)
        a.close(); b.close()
    assert extended >= 1                                           # some window grew by an anchor behind an INNER keyframe's edge
    # without the flags: the window is prepared, the flags stay
    flags = in_window(from_root)
    r3, wid3, _ = from_root.prepare_window_from_root(kf[0], 3, 6, set_window_flags=False)
    assert in_window(from_root) == flags and r3.n_window == len(wid3) >= 6
    for d in maps:
        d.close()


@pytest.mark.gpu
def test_update_marginalization_resolves_missing_anchors(gpu_ctx):
    """resolve_missing=True: the anchors outside the window get their pose from absolute_poses, the stored constraint is the model's with those poses cached"""
    import torch
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    ctx, stream = gpu_ctx
    sc = CM.scene()
    m, ids = sc["map"], sc["ids"]
    kf = [int(k) for k in m["kf_ids"]]
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((48 >> l, 64 >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((48, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    d = ResidentMap(ctx, max_keyframes=256, max_points=20000, max_observations=16384)
    kfs = keyframe_table([([t.data_ptr() for t in pyr], [t.shape[1] for t in pyr], T) for T in m["kf_poses"]])
    d.add_keyframes(m["kf_ids"], kfs, [(disp.data_ptr(), disp.shape[1])] * len(kfs), [[[25], [25], [25]]] * len(kfs))
    pts = np.zeros(len(m["point_ids"]), CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = m["xyz"], m["anchor_ids"]
    d.add_points(m["point_ids"], pts)
    d.add_observations(m["obs_point"], m["obs_kf"])
    table = CM.EdgeTable()
    edges = [(kf[i], kf[i + 1], 30) for i in range(len(kf) - 1)]
    d.reserve_edges(len(edges))
    d.add_edges([(a, b) for a, b, _ in edges], 30, 0)
    for a, b, s in edges:
        table.insert(a, b, s, 0)
    adj = WM.adjacency(table)
    A, B = ids["A"], ids["B"]
    old = ([A, B], [0, 0])
    new = (sc["window_small"], [1 if k == A else 0 for k in sc["window_small"]])
    d.set_window(new[0])
    tabs = CM.tables(m)
    plain, missing = d.update_marginalization(old, new)
    assert sorted(missing) == sorted(sc["outside"]) and plain[0]["status"] == CM.MISSING_ANCHOR
    res, missing = d.update_marginalization(old, new, resolve_missing=True)
    cached = {k: WM.absolute_pose(adj, new[0], table, tabs[1], k)[2] for k in sc["outside"]}
    want = CM.compute(m, new[0], A, B, _tables=tabs, cached=cached)
    assert missing == [] and len(res) == 1 and res[0]["status"] == CM.OK == want["status"]
    assert d.raw["results"][0].tobytes() == CM.result_record(want).tobytes()
    table.set_constraint(A, B, want["T_12"], want["info"])
    assert d.get_edges([(A, B)])[0].tobytes() == table.record(A, B).tobytes()
    d.close()


@pytest.mark.gpu
def test_cpp_adaptor_walks(gpu_ctx, tmp_path):
    """tests/cpp/walk_smoke.cpp: BackendMap::computeInitialDoubleWin / framesInNeighborhood / computeAbsolutePose / prepareForOptimization(root_id, loop_id)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "walk_smoke"
    libdir = os.path.join(root, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "walk_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("WALK ")]
    assert tok and tok[0].split()[1:4] == ["ok", "3", "1"] and int(tok[0].split()[4]) >= 40, out
