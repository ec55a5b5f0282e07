"""GPU tests of inserting a keyframe into the device-resident map: svs_map_compute_strength against the closed form of tests/addkf_model.py, byte for byte, and
svs_map_add_keyframe / svs_map_add_first_keyframe against a twin map built through svs_map_add_keyframes, _add_points, _add_measured_observations, _add_edges
and a storing _compute_constraints (tests/test_addkf_cpu.py holds the model to the reference's loops).  Blank 64 x 48 pyramids; 80 keyframes with non-contiguous
ids on both sides of 8192, so that high words of the keyframe bitmap are used.

One case one might look for cannot occur: an edge that add_keyframe makes always has a common point (a key anchors a kept new point, or observes a track point that
the new keyframe now observes too), so SVS_CONS_EMPTY is not reachable through this call; the zero, unmarginalised edge is shown with SVS_CONS_MISSING_ANCHOR."""
import os
import subprocess

import numpy as np
import pytest

import addkf_model as AM

HW, HH = 320, 240
KF_IDS = list(range(3, 3 + 40 * 7, 7)) + [8190, 8191, 8192, 8193] + list(range(9000, 9000 + 36 * 13, 13))
X_KF, X2_KF = 8192, 8193                                          # keyframes that observe only their own points
ORDINARY = [k for k in KF_IDS if k not in (X_KF, X2_KF)]
US, VS = [5.0, 319.0, 319.999, 320.0, 320.5, 630.0], [7.0, 239.5, 240.0, 240.25, 470.0]


@pytest.fixture(scope="module")
def blank(gpu_ctx):
    import torch
    ctx, stream = gpu_ctx
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((48 >> l, 64 >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((48, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    return pyr, disp


def _kf_records(blank, poses):
    from scavislam_amd.register import keyframe_table
    pyr, _ = blank
    return keyframe_table([([t.data_ptr() for t in pyr], [t.shape[1] for t in pyr], T) for T in poses])


def _disp(blank):
    return (blank[1].data_ptr(), blank[1].shape[1])


THR = [[25], [25], [25]]


def _fill(d, blank, kf_ids, vis):
    """keyframes with identity poses, the points of `vis` anchored in their smallest observer, their rows as measured pairs"""
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    d.add_keyframes(kf_ids, _kf_records(blank, [AM.I12] * len(kf_ids)), [_disp(blank)] * len(kf_ids), [THR] * len(kf_ids))
    ids = sorted(vis)
    pts = np.zeros(len(ids), CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = [0.0, 0.0, 4.0], [min(vis[p]) for p in ids]
    d.add_points(ids, pts)
    pp = [p for p in ids for _ in vis[p]]
    kk = [k for p in ids for k in sorted(vis[p])]
    d.add_measured_observations(pp, kk, np.zeros((len(pp), 3)), np.zeros(len(pp), np.int32))


@pytest.fixture(scope="module")
def smap(gpu_ctx, blank):
    """the map of the strength tests: rows of 1, 2, 63, 64, 65 and 70 observers, 1400 rows of 1 .. 6, 24 points of X_KF (with the first ordinary keyframe) and 12
    of X2_KF alone"""
    from scavislam_amd.register import ResidentMap
    rng = np.random.default_rng(11)
    vis = {}
    for j, n in enumerate((1, 2, 63, 64, 65, 70)):
        vis[100 + j] = set(int(k) for k in rng.choice(ORDINARY, n, replace=False))
    for j in range(1400):
        vis[200 + 2 * j] = set(int(k) for k in rng.choice(ORDINARY, int(rng.integers(1, 7)), replace=False))
    for j in range(24):
        vis[4000 + j] = {X_KF, ORDINARY[0]}
    for j in range(12):
        vis[4100 + j] = {X2_KF}
    d = ResidentMap(gpu_ctx[0], max_keyframes=16384, max_points=8192, max_observations=1 << 15)
    _fill(d, blank, KF_IDS, vis)
    yield d, vis
    d.close()


def _track(entries):
    """(global_id, u, v) -> dicts"""
    return [dict(global_id=int(g), center=[float(u), float(v), 1.0], level=0) for g, u, v in entries]


def _random_track(rng, vis, n):
    ids = [p for p in vis if p < 4000] + [7000, 7001, 8191]      # with unknown ids; sampled with replacement: duplicates
    return _track([(rng.choice(ids), rng.choice(US), rng.choice(VS)) for _ in range(n)])


def _strength(d, vis, track, thr, anchors=()):
    """one compute_strength against the model, byte for byte -> (the call's output, the raw bytes)"""
    from scavislam_amd.ctypes_types import MAP_KEY_DTYPE, MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE
    new = np.zeros(len(anchors), MAP_NEW_POINT_DTYPE)
    new["anchor_id"] = list(anchors)
    out = d.compute_strength(new, AM.track_point_records(track, MAP_TRACK_POINT_DTYPE), thr, HW, HH)
    keys, exists, m = AM.strength_closed_form(list(anchors), [(t["global_id"], t["center"][0], t["center"][1]) for t in track], vis, thr, HW, HH)
    raw = d.raw["keys"].tobytes() + d.raw["track_exists"].tobytes()
    assert (out["n_keys"], out["m"], out["over_capacity"]) == (len(keys), m, False)
    assert d.raw["keys"].tobytes() == AM.key_records(keys, MAP_KEY_DTYPE).tobytes(), [(list(a), b) for a, b in zip(out["keys"], keys) if list(a)[:6] != b][:5]
    assert out["track_exists"].tolist() == exists
    return out, raw


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0, 6, 15])
def test_strength_equals_the_model_at_every_list_length(smap, thr):
    d, vis = smap
    h = max(thr // 2, 1)
    rng = np.random.default_rng(thr)
    nonzero = 0
    for n in (0, 1, 4 * h - 1, 4 * h, 511, 512, 513, 1100):
        anchors = [int(k) for k in rng.choice(ORDINARY, 10)]
        out, _ = _strength(d, vis, _random_track(rng, vis, n), thr, anchors)
        nonzero += sum(1 for k in out["keys"] if k["strength"] > 0)
        if n == 0:
            assert out["m"] == 0 and sum(out["neighborid_to_strength"].values()) == 10
    assert _strength(d, vis, [], thr)[0]["n_keys"] == 0           # both lists empty: no key
    assert nonzero > 0
    # the long rows alone, and one of each length
    for p in (100, 101, 102, 103, 104, 105):
        out, _ = _strength(d, vis, _track([(p, 5.0, 7.0), (p, 630.0, 470.0)]), 2)
        assert out["n_keys"] == len(vis[p]) and all(k["strength"] == 1 for k in out["keys"])
    _strength(d, vis, _track([(100 + j, 5.0, 7.0) for j in range(6)] + [(100 + j, 630.0, 470.0) for j in range(6)]), 2)


@pytest.mark.gpu
def test_crossings_in_four_chunks_at_the_last_entry_and_under_rotation(smap):
    d, vis = smap
    rng = np.random.default_rng(3)
    filler = [p for p in vis if 200 <= p < 4000]
    L, R, T, B = 5.0, 630.0, 7.0, 470.0
    # thr 6, h 3.  X_KF observes the points 4000 ..: LEFT crosses in chunk 0, TOP in chunk 1, RIGHT in chunk 2, BOTTOM in chunk 3; X2_KF crosses at the last entry
    mine = {10: (4000, L, T), 20: (4001, L, T), 300: (4002, L, B), 600: (4003, L, T), 1030: (4004, R, T), 1100: (4005, R, T), 1500: (4006, R, T), 1540: (4007, L, B),
            1700: (4008, L, B), 1800: (4009, R, B), 2000: (4010, L, T)}
    x2 = {40: (4100, L, T), 50: (4101, L, T), 60: (4102, L, T), 70: (4103, R, T), 80: (4104, R, T), 90: (4105, R, B), 95: (4106, R, B), 2047: (4107, L, B)}
    n = 2048
    entries = [mine.get(i) or x2.get(i) or (rng.choice(filler), rng.choice(US), rng.choice(VS)) for i in range(n)]
    out, _ = _strength(d, vis, _track(entries), 6)
    s = out["neighborid_to_strength"]
    assert s[X_KF] == 3 and s[X2_KF] == 1                          # 1700, 1800, 2000; the last entry itself
    rows = {int(k["kf_id"]): k for k in out["keys"]}
    assert [int(rows[X_KF][f]) for f in ("n_left", "n_right", "n_top", "n_bottom")] == [7, 4, 7, 4]
    # the same list rotated: the strengths change as the model says
    for rot in (1, 512, 1701):
        o2, _ = _strength(d, vis, _track(entries[rot:] + entries[:rot]), 6)
        assert [int(rows[X_KF][f]) for f in ("n_left", "n_right", "n_top", "n_bottom")] == [int(k[f]) for k in o2["keys"] if k["kf_id"] == X_KF for f in ("n_left", "n_right", "n_top", "n_bottom")]
    o3, _ = _strength(d, vis, _track(entries[1701:] + entries[:1701]), 6)
    assert o3["neighborid_to_strength"][X_KF] != s[X_KF]


@pytest.mark.gpu
def test_1024_keys_fit_and_1025_are_only_counted(gpu_ctx, blank):
    from scavislam_amd.ctypes_types import MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE
    from scavislam_amd.register import ResidentMap
    kf_ids = [5 + 15 * j for j in range(1030)]                     # up to 15440
    vis = {50 + j: {kf_ids[j]} for j in range(1030)}
    d = ResidentMap(gpu_ctx[0], max_keyframes=16384, max_points=2048, max_observations=4096)
    try:
        _fill(d, blank, kf_ids, vis)
        out, _ = _strength(d, vis, _track([(50 + j, 5.0, 7.0) for j in range(1024)]), 0)
        assert out["n_keys"] == 1024 and not out["over_capacity"]
        out, _ = _strength(d, vis, _track([(50 + j, 5.0, 7.0) for j in range(1000)]), 0, anchors=kf_ids[1000:1024])
        assert out["n_keys"] == 1024
        new = np.zeros(1, MAP_NEW_POINT_DTYPE)
        new["anchor_id"] = kf_ids[1029]
        over = d.compute_strength(new, AM.track_point_records(_track([(50 + j, 5.0, 7.0) for j in range(1024)]), MAP_TRACK_POINT_DTYPE), 0, HW, HH)
        assert over["over_capacity"] and over["n_keys"] == 1025 and over["m"] == 0 and len(over["keys"]) == 0
        assert not d.raw["keys"].view(np.uint8).any() and not d.raw["track_exists"].any()      # the count and the mark, nothing else
    finally:
        d.close()


@pytest.mark.gpu
def test_a_request_gives_the_same_bytes_after_unrelated_growth(smap, blank):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    d, vis = smap
    rng = np.random.default_rng(8)
    track = _random_track(rng, vis, 700)
    anchors = [int(k) for k in rng.choice(ORDINARY, 6)]
    _, before = _strength(d, vis, track, 6, anchors)
    # keyframes, points and pairs that no tracked point has anything to do with
    more_kf = [16001, 16002, 2]
    d.add_keyframes(more_kf, _kf_records(blank, [AM.I12] * 3), [_disp(blank)] * 3, [THR] * 3)
    pts = np.zeros(3, CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = [0.0, 0.0, 4.0], ORDINARY[3]
    d.add_points([6000, 6001, 1], pts)
    d.add_measured_observations([6000, 6001, 1, 6000, 6001], [ORDINARY[3], ORDINARY[4], ORDINARY[5], X2_KF, 16001], np.zeros((5, 3)), np.zeros(5, np.int32))
    vis.update({6000: {ORDINARY[3], X2_KF}, 6001: {ORDINARY[4], 16001}, 1: {ORDINARY[5]}})
    _, after = _strength(d, vis, track, 6, anchors)
    assert before == after


# ---- add_keyframe against the twin map ----------------------------------------------------------------------------------------------------------------------------
FIRST, NEWKEYS = 2, [9, 8195, 31, 8300, 64, 9001, 120, 121, 12000, 300, 16383, 500]
CHAIN_THR = 4
CAPS = dict(max_keyframes=16384, max_points=4096, max_observations=1 << 14)


def _rel_pose(rng):
    a = float(rng.uniform(-0.05, 0.05))
    c, s = float(np.cos(a)), float(np.sin(a))
    t = rng.uniform(-0.2, 0.2, 3)
    return [c, -s, 0.0, float(t[0]), s, c, 0.0, float(t[1]), 0.0, 0.0, 1.0, float(t[2])]


def chain_inputs():
    """the 12 insertions: (newkey, oldkey, T_rel, new points, track points), generated against a model graph that is advanced alongside"""
    rng = np.random.default_rng(21)
    g = AM.Graph()
    g.add_first_keyframe(FIRST)
    keys, next_pid, steps = [FIRST], 1000, []
    for i, newkey in enumerate(NEWKEYS):
        oldkey = keys[-1]
        anchors = [oldkey] * 10 + [keys[0]] * 2 + [keys[-2] if len(keys) > 1 else oldkey] * 2
        new = []
        for a in anchors:
            new.append(dict(point_id=next_pid, anchor_id=a, xyz_anchor=[float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), float(rng.uniform(3, 9))],
                            anchor_obs_pyr=rng.uniform(1, 150, 3).tolist(), anchor_level=int(rng.integers(3)), feat_center=rng.uniform(1, 600, 3).tolist(),
                            feat_level=int(rng.integers(3))))
            next_pid += 3
        known = sorted(g.vis)
        track = []
        if known:
            recent = [p for p in known if g.vis[p] & set(keys[-3:])]
            for _ in range(2 if i == 6 else 45):                     # (two track points cannot fill four classes twice: the oldkey needs the clamp)
                gid = int(rng.choice(recent if rng.random() < 0.8 else known))
                track.append(dict(global_id=gid, center=[float(rng.choice([rng.uniform(0, 640), 320.0])), float(rng.choice([rng.uniform(0, 480), 240.0])), float(rng.uniform(0, 600))],
                                  level=int(rng.integers(3))))
            track.insert(5, dict(global_id=3999, center=[1.0, 1.0, 1.0], level=0))      # no point of the map
            track.append(dict(track[0]))                                                 # twice: counted twice, the first feature wins
        T_rel = _rel_pose(rng)
        out = g.add_keyframe(newkey, oldkey, T_rel, new, track, CHAIN_THR, HW, HH)
        steps.append((newkey, oldkey, T_rel, new, track, out))
        keys.append(newkey)
    return steps, g


def test_the_chain_drops_points_and_needs_the_clamp():
    """on the model alone: the cases the GPU chain is there for exist in it"""
    steps, g = chain_inputs()
    assert any(not all(o["kept"]) for *_, o in steps) and all(any(o["kept"]) for *_, o in steps)
    assert any(len(o["edges"]) >= 3 for *_, o in steps) and any(len(o["keys"]) > len(o["edges"]) for *_, o in steps)
    newkey, oldkey, _, _, _, o = steps[6]
    assert o["edges"] == [(oldkey, newkey, CHAIN_THR)] and len(o["keys"]) >= 2 and o["m"] >= 2      # strength(oldkey) was below the threshold
    assert any(t["global_id"] == 3999 for t in steps[3][4]) and len(g.log) == len(set((p, k) for p, k, _, _ in g.log))


def _new_map(ctx):
    from scavislam_amd.register import ResidentMap
    d = ResidentMap(ctx, **CAPS)
    d.reserve_edges(4096)
    return d


def _insert(d, blank, step, **kw):
    from scavislam_amd.ctypes_types import MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE
    newkey, oldkey, T_rel, new, track, _ = step
    return d.add_keyframe(newkey, oldkey, T_rel, _kf_records(blank, [AM.I12])[0], _disp(blank), THR, AM.new_point_records(new, MAP_NEW_POINT_DTYPE),
                          AM.track_point_records(track, MAP_TRACK_POINT_DTYPE), CHAIN_THR, HW, HH, **kw)


def _same_maps(d, t, g):
    assert d.info() == t.info() == (len(g.pose), len(g.point), len(g.log)) and d.edge_info() == t.edge_info() and d.measured_info() == t.measured_info()
    kfs, pts, edges = sorted(g.pose), sorted(g.point), [(a, b) for a, b, _ in g.edges]
    assert d.get_edges(edges).tobytes() == t.get_edges(edges).tobytes()
    assert d.get_poses(kfs).tobytes() == t.get_poses(kfs).tobytes() == np.array([g.pose[k] for k in kfs], np.float64).tobytes()
    assert d.get_points(pts).tobytes() == t.get_points(pts).tobytes()
    assert d.edge_keys == t.edge_keys and d.edge_log == t.edge_log
    for k in kfs:
        a, b = d.get_feature_table(k), t.get_feature_table(k)
        want = sorted(p for p, kf, _, _ in g.log if kf == k)
        assert a[0].tolist() == b[0].tolist() == want and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == len(want), k
    return kfs, pts


@pytest.mark.gpu
def test_a_chain_of_insertions_equals_the_twin_map(gpu_ctx, blank):
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE, CANDIDATE_DTYPE, CONS_MISSING_ANCHOR, CONS_OK, MAP_KEY_DTYPE, Cam
    from scavislam_amd.frontend import StereoFrontend
    import register_model as RM
    ctx = gpu_ctx[0]
    steps, g = chain_inputs()
    d, t = _new_map(ctx), _new_map(ctx)
    fe = None
    try:
        d.add_first_keyframe(FIRST, _kf_records(blank, [[9.0] * 12]), _disp(blank), THR)      # (the record's pose is ignored)
        t.add_keyframes([FIRST], _kf_records(blank, [AM.I12]), [_disp(blank)], [THR])
        with pytest.raises(Exception):
            d.add_first_keyframe(7, _kf_records(blank, [AM.I12]), _disp(blank), THR)         # the map is not empty
        keys, statuses, poses = [FIRST], [], {FIRST: list(AM.I12)}
        for i, step in enumerate(steps):
            newkey, oldkey, _, new, track, want = step
            window = keys[-3:]
            d.set_window(window)
            t.set_window(window)
            cached = dict(poses) if i == 5 else None               # one insertion with cached anchor poses, one that resolves its missing anchors itself
            out = _insert(d, blank, step, cached=cached, resolve_missing=(i == 8))
            assert d.raw["keys"].tobytes() == AM.key_records(want["keys"], MAP_KEY_DTYPE).tobytes(), i
            assert out["new_kept"].tolist() == want["kept"] and out["track_exists"].tolist() == want["exists"] and out["m"] == want["m"]
            assert out["edges"] == [(a, b) for a, b, _ in want["edges"]] and out["exclude_set"] == {newkey} | {a for a, _, _ in want["edges"]}
            assert out["do_loop_detection"] == (len(out["exclude_set"]) < len(keys) + 1)
            first = [dict(zip(("status", "n_missing"), (int(r["status"]), int(r["n_missing"])))) for r in d.raw["results"][:len(out["edges"])]]
            raw = d.raw["results"][:len(out["edges"])].tobytes(), d.raw["missing"][:len(out["edges"])].tobytes()
            assert not d.raw["results"][len(out["edges"]):].view(np.uint8).any() and (d.raw["missing"][len(out["edges"]):] == -1).all()
            res = AM.replay_on_twin(t, newkey, _kf_records(blank, [AM.I12]), _disp(blank), THR, want, CANDIDATE_DTYPE, cached=cached)
            assert raw == (t.raw["results"].tobytes(), t.raw["missing"].tobytes()), i
            if i == 8:
                res, miss = t.complete_constraints(out["edges"], res)
                assert miss == out["missing"] and any(f["status"] == CONS_MISSING_ANCHOR for f in first)
            assert [(o["status"], o["strength"], o["T_12"].tobytes(), o["info"].tobytes()) for o in out["edge_results"]] == \
                   [(o["status"], o["strength"], o["T_12"].tobytes(), o["info"].tobytes()) for o in res], i
            statuses.append([o["status"] for o in out["edge_results"]])
            keys.append(newkey)
            poses[newkey] = want["pose"]
            if i in (0, 4, 8):
                _same_maps(d, t, _graph_up_to(steps, i))
        print("statuses", statuses)
        assert all(s == CONS_OK for s in statuses[5]) and all(s == CONS_OK for s in statuses[8]) and statuses[0] == [CONS_OK]
        assert any(CONS_MISSING_ANCHOR in s for s in statuses)     # such an edge exists, zero and not marginalised: the edge bytes below
        kfs, pts = _same_maps(d, t, g)
        missing_edges = [e for e in d.get_edges([(a, b) for a, b, _ in g.edges]) if not e["is_marginalized"]]
        assert missing_edges and all(not e["T_lo_from_hi"].any() and not e["info"].any() for e in missing_edges)
        # what reads the map afterwards: the window from the root (with the measured store's log order behind window_edges), the neighbourhood, a stream's list
        cam = Cam(500.0, 320.0, 240.0, 0.1, 640, 480)
        got = []
        for m in (d, t):
            res, wid, wtype = m.prepare_window_from_root(keys[-1], 3, 6)
            opt = SlamGraphOptimizer(ctx)
            opt.windowFromMap(m, np.zeros(0, BA_CONSTRAINT_DTYPE), cam)
            nb = m.frames_in_neighborhood([keys[-1], keys[3]], 5)
            got.append((bytes(res), wid.tobytes(), wtype.tobytes(), opt.window_edges().tobytes(), [x.tolist() for x in nb]))
            opt.close()
        assert got[0] == got[1] and len(got[0][3]) > 0
        fe = StereoFrontend(ctx, RM.SMALL_CAM, max_points=2048, max_keyframes=4)
        lists = [fe.setCandidatesFromMap(m, [dict(stream=0, vertex_kf=[keys[-1], keys[-2], keys[2]], slot_kf=[-1] * 4)], refresh_poses=False)[0] for m in (d, t)]
        assert lists[0]["raw"] == lists[1]["raw"] and lists[0]["n_points"] > 20 and not lists[0]["over_capacity"]
    finally:
        if fe is not None:
            fe.close()
        d.close()
        t.close()


def _graph_up_to(steps, i):
    """the model graph after insertion i"""
    g = AM.Graph()
    g.add_first_keyframe(FIRST)
    for newkey, oldkey, T_rel, new, track, _ in steps[:i + 1]:
        g.add_keyframe(newkey, oldkey, T_rel, new, track, CHAIN_THR, HW, HH)
    return g


@pytest.mark.gpu
def test_every_refusal_leaves_the_map_unchanged(gpu_ctx, blank):
    from scavislam_amd.capi import SvsError
    from scavislam_amd.register import ResidentMap
    ctx = gpu_ctx[0]
    steps, _ = chain_inputs()
    d = _new_map(ctx)
    small = ResidentMap(ctx, max_keyframes=64, max_points=4096, max_observations=40)      # room for the first insertion's 28 pairs, not for the second's
    no_edges = ResidentMap(ctx, max_keyframes=64, max_points=4096, max_observations=4096)
    try:
        for m in (d, small, no_edges):
            m.add_first_keyframe(FIRST, _kf_records(blank, [AM.I12]), _disp(blank), THR)
        small.reserve_edges(8)
        _insert(d, blank, steps[0])
        _insert(d, blank, steps[1])
        _insert(small, blank, steps[0])
        before = d.info(), d.edge_info(), d.measured_info()
        newkey, oldkey, T_rel, new, track, _ = steps[2]

        def refused(**change):
            s = dict(newkey=newkey, oldkey=oldkey, new=[dict(p) for p in new], track=[dict(q) for q in track])
            for k, v in change.items():
                if callable(v):
                    v(s)
                else:
                    s[k] = v
            with pytest.raises(SvsError) as e:
                _insert(d, blank, (s["newkey"], s["oldkey"], T_rel, s["new"], s["track"], None))
            assert (d.info(), d.edge_info(), d.measured_info()) == before, change
            return str(e.value)

        assert "status 1" in refused(oldkey=777)                                            # unknown oldkey
        assert "status 1" in refused(newkey=FIRST)                                          # newkey present
        assert "status 4" in refused(newkey=16384)                                          # beyond the capacity
        assert "status 1" in refused(new=lambda s: s["new"][3].update(anchor_id=778))       # unknown anchor
        assert "status 1" in refused(new=lambda s: s["new"][3].update(point_id=steps[0][3][0]["point_id"]))      # a point of the map
        assert "status 1" in refused(new=lambda s: s["new"][3].update(point_id=s["new"][4]["point_id"]))         # twice in the list
        assert "status 1" in refused(track=lambda s: s["track"][2].update(global_id=s["new"][0]["point_id"]))    # equal to a track id
        assert "status 4" in refused(new=lambda s: s["new"][3].update(point_id=4096))
        for field in ("anchor_level", "feat_level"):
            for bad in (-1, 3):
                assert "status 1" in refused(new=lambda s, f=field, b=bad: s["new"][0].update({f: b}))
        assert "status 1" in refused(track=lambda s: s["track"][5].update(level=3))         # also on an entry that names no point of the map
        # oldkey no key of the table: no new point anchored there, no track point it observes
        far = lambda s: (s.update(new=[p for p in s["new"] if p["anchor_id"] != oldkey], track=[q for q in s["track"] if q["global_id"] == 3999]))
        assert "status 1" in refused(new=far)
        with pytest.raises(SvsError) as e:
            _insert(small, blank, steps[1])
        assert "status 4" in str(e.value) and small.info() == (2, sum(steps[0][5]["kept"]), len(steps[0][5]["pairs"]))
        with pytest.raises(SvsError) as e:
            _insert(no_edges, blank, steps[0])
        assert "status 4" in str(e.value) and no_edges.info() == (1, 0, 0)
        # the map still takes the insertion it refused in pieces
        out = _insert(d, blank, steps[2])
        assert out["edges"] == [(a, b) for a, b, _ in steps[2][5]["edges"]]
    finally:
        for m in (d, small, no_edges):
            m.close()


@pytest.mark.gpu
def test_feature_table_at_the_edges_of_the_bitmap_words_and_of_the_compaction_block(gpu_ctx, blank):
    """The read-back lists a bitmap over point ids, one trip per 512 words of 32 ids: its second trip starts at point id 16384.  A few dozen points with ids on
    both sides of every word edge and of that block edge, measured and unmeasured pairs mixed; the whole table, and every capacity below its length (the entries
    at or behind it are counted, not written), against the pairs as they were given (records: slam_graph.cpp:1010-1015 through ba_map_model.info_from_level)"""
    import ba_map_model as BM
    from scavislam_amd.ctypes_types import BA_EDGE_DTYPE, CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap
    MAXP, KF, OTHER = 20000, 40, 3
    pt_ids = [0, 31, 32, 63, 64, 16383, 16384, 16385, MAXP - 1] + list(range(100, 124))
    rng = np.random.default_rng(5)
    d = ResidentMap(gpu_ctx[0], max_keyframes=64, max_points=MAXP, max_observations=256)
    try:
        d.add_keyframes([OTHER, KF], _kf_records(blank, [AM.I12] * 2), [_disp(blank)] * 2, [THR] * 2)
        pts = np.zeros(len(pt_ids), CANDIDATE_DTYPE)
        pts["xyz_anchor"], pts["kf_index"] = [0.0, 0.0, 4.0], OTHER
        d.add_points(pt_ids, pts)
        mine = [p for i, p in enumerate(pt_ids) if i < 9 or i % 3]                       # every edge id, two thirds of the rest
        measured = [p for i, p in enumerate(mine) if i % 4 != 1]
        center, level = rng.uniform(1, 600, (len(measured), 3)), rng.integers(0, 3, len(measured)).astype(np.int32)
        order = rng.permutation(len(measured))
        d.add_measured_observations([measured[i] for i in order], [KF] * len(measured), center[order], level[order])
        d.add_observations([p for p in mine if p not in measured], [KF] * (len(mine) - len(measured)))
        d.add_measured_observations(pt_ids[::2], [OTHER] * len(pt_ids[::2]), np.ones((len(pt_ids[::2]), 3)), np.zeros(len(pt_ids[::2]), np.int32))
        want = np.zeros(len(mine), BA_EDGE_DTYPE)
        want["point"], want["pose"], want["anchor"] = sorted(mine), KF, -1
        for p, c, l in zip(measured, center, level):
            i = sorted(mine).index(p)
            want["obs"][i], want["info"][i], want["anchor"][i] = c, BM.info_from_level([l])[0], 0
        at = sorted(mine).index(16384)                                                    # the first id of the lister's second trip
        assert max(mine) == MAXP - 1 and {16383, 16385} <= set(mine) and set(measured) & {16384, 16385, MAXP - 1}
        for cap in (None, len(mine), len(mine) - 1, at + 1, at, at - 1, 1, 0):
            ids, rec, n = d.get_feature_table(KF, cap)
            k = len(mine) if cap is None else cap
            assert n == len(mine) and ids.tolist() == sorted(mine)[:k] and rec.tobytes() == want[:k].tobytes(), cap
    finally:
        d.close()


@pytest.mark.gpu
def test_cpp_adaptor_add_keyframe(gpu_ctx, tmp_path):
    """tests/cpp/addkf_smoke.cpp: BackendMap::addFirstKeyframe / addKeyframe"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "addkf_smoke"
    libdir = os.path.join(root, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "addkf_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("ADDKF ")]
    assert tok and tok[0].split() == ["ADDKF", "ok", "3", "2", "60", "16"], out
