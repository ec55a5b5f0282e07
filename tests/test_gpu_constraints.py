"""GPU tests of the pose graph's edges in the device-resident map and of computeConstraint on the device: svs_map_add_edges / _set_constraints / _unmarginalize /
_get_edges / _edge_info, svs_map_compute_constraints, svs_ba_window_from_map_edges and svs_ba_window_constraints against the NumPy model
(tests/constraint_model.py), byte for byte.  The map is constraint_model.scene(): 19 keyframes, about 1 900 points, common-point counts 0 .. 1 500."""
import numpy as np
import pytest

import ba_map_model as BM
import constraint_model as CM

CAPS = dict(max_keyframes=256, max_points=20000, max_observations=16384)
PAIRS = [("A", "J"), ("A", "I"), ("A", "H"), ("A", "G"), ("A", "F"), ("A", "E"), ("A", "D"), ("A", "C"), ("A", "B"), ("B", "A"), ("F", "A"), ("I", "B"), ("D", "C"),
         ("T", "U"), ("T", "V"), ("U", "V"), ("V", "T")]      # 0, 1, 2, 3, 64, 65, 512, 513, 1 500 common points; short against long rows; tied depths
DEPTH_CAP = 1600


@pytest.fixture(scope="module")
def sc():
    return CM.scene()


@pytest.fixture(scope="module")
def tabs(sc):
    return CM.tables(sc["map"])


@pytest.fixture(scope="module")
def blank(gpu_ctx):
    """one blank pyramid and disparity for every keyframe: the constraint walks never read them"""
    import torch
    ctx, stream = gpu_ctx
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((48 >> l, 64 >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((48, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    return pyr, disp


def _fill(ctx, blank, m, measured=False, caps=CAPS):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    pyr, disp = blank
    d = ResidentMap(ctx, **caps)
    kfs = keyframe_table([([t.data_ptr() for t in pyr], [t.shape[1] for t in pyr], T) for T in m["kf_poses"]])
    d.add_keyframes(m["kf_ids"], kfs, [(disp.data_ptr(), disp.shape[1])] * len(kfs), [[[25], [25], [25]]] * len(kfs))
    pts = np.zeros(len(m["point_ids"]), CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = m["xyz"], m["anchor_ids"]
    d.add_points(m["point_ids"], pts)
    if measured:
        d.add_measured_observations(m["obs_point"], m["obs_kf"], m["obs_center"], m["obs_level"])
    else:
        d.add_observations(m["obs_point"], m["obs_kf"])
    return d


@pytest.fixture(scope="module")
def dmap(gpu_ctx, blank, sc):
    d = _fill(gpu_ctx[0], blank, sc["map"])
    yield d
    d.close()


def _absolute(sc, tabs, which=None):
    """the caller's computeAbsolutePose results for the keyframes outside the small window: something else than the stored pose"""
    return {k: [v + 0.015625 for v in tabs[1][k]] for k in (sc["outside"] if which is None else which)}


def _check(dmap, i, want, missing_cap, what):
    """request i of the last call against the model: the result record, the missing ids and the depth row as bytes"""
    raw = dmap.raw
    got = raw["results"][i]
    for f in ("status", "strength", "n_missing", "median", "norm_dist", "T_12", "info"):
        assert np.asarray(got[f]).tobytes() == np.asarray(CM.result_record(want)[f]).tobytes(), (what, f, got[f], want[f])
    assert got.tobytes() == CM.result_record(want).tobytes(), what
    row = np.full(missing_cap, -1, np.int32)
    k = min(len(want["missing"]), missing_cap)
    row[:k] = want["missing"][:k]
    assert np.array_equal(raw["missing"][i], row), (what, raw["missing"][i], want["missing"])
    if raw["depths"].shape[1]:
        drow = np.zeros(raw["depths"].shape[1])
        drow[:len(want["depths"])] = want["depths"]
        bad = np.nonzero(raw["depths"][i].view(np.uint64) != drow.view(np.uint64))[0]
        assert len(bad) == 0, (what, "depths differ at", bad[:8], raw["depths"][i][bad[:8]].tolist(), drow[bad[:8]].tolist())


@pytest.mark.gpu
def test_every_common_point_count_with_all_anchors_in_the_window(gpu_ctx, dmap, sc, tabs):
    m, ids = sc["map"], sc["ids"]
    dmap.set_window(sc["window_all"])
    reqs = [dict(kf1=ids[a], kf2=ids[b]) for a, b in PAIRS]
    out = dmap.compute_constraints(reqs, missing_cap=4, depth_cap=DEPTH_CAP)
    counts = []
    for i, (a, b) in enumerate(PAIRS):
        want = CM.compute(m, sc["window_all"], ids[a], ids[b], _tables=tabs)
        _check(dmap, i, want, 4, (a, b))
        counts.append(out[i]["strength"])
    assert counts[:9] == [0, 1, 2, 3, 64, 65, 512, 513, 1500] and out[0]["status"] == CM.EMPTY and all(o["status"] == CM.OK for o in out[1:])
    # each alone gives the same bytes as in the batch
    whole = {k: v.copy() for k, v in dmap.raw.items()}
    for i in (0, 1, 5, 8, 13):
        dmap.compute_constraints([reqs[i]], missing_cap=4, depth_cap=DEPTH_CAP)
        assert dmap.raw["results"][0].tobytes() == whole["results"][i].tobytes() and dmap.raw["depths"][0].tobytes() == whole["depths"][i].tobytes()


@pytest.mark.gpu
def test_cached_missing_and_overridden_anchor_poses(gpu_ctx, dmap, sc, tabs):
    m, ids = sc["map"], sc["ids"]
    A, B, C_ = ids["A"], ids["B"], ids["C"]
    out4 = sc["outside"]
    dmap.set_window(sc["window_small"])
    cached = _absolute(sc, tabs)
    half = _absolute(sc, tabs, out4[1:3])
    T_a = m["kf_poses"][0].copy(); T_a[3] += 0.25; T_a[7] -= 0.125                               # A "brought temporarily" elsewhere; A anchors an eighth of the pool
    T_o = np.array(tabs[1][out4[0]]); T_o[11] += 0.5                                               # an override of a keyframe that is neither kf1 nor kf2 nor in the window
    cases = [
        ("cached", dict(kf1=A, kf2=B, cached=cached), dict(cached=cached)),
        ("cached, reverse", dict(kf1=B, kf2=A, cached=cached), dict(cached=cached)),
        ("all missing", dict(kf1=A, kf2=B), dict()),
        ("two of four missing", dict(kf1=A, kf2=C_, cached=half), dict(cached=half)),
        ("override on kf1, an anchor", dict(kf1=A, kf2=B, cached=cached, overrides=[(A, T_a)]), dict(cached=cached, overrides=[(A, T_a)])),
        ("override on kf2 and on an outside anchor", dict(kf1=A, kf2=B, cached=half, overrides=[(B, T_a), (out4[0], T_o)]), dict(cached=half, overrides=[(B, T_a), (out4[0], T_o)])),
        ("an override stands in for a cached pose", dict(kf1=C_, kf2=A, cached=_absolute(sc, tabs, out4[1:]), overrides=[(out4[0], T_o)]),
         dict(cached=_absolute(sc, tabs, out4[1:]), overrides=[(out4[0], T_o)])),
    ]
    for cap in (8, 1):                                                                           # a count above the cap: n_missing says how many there are
        out = dmap.compute_constraints([q for _, q, _ in cases], missing_cap=cap, depth_cap=DEPTH_CAP)
        for i, (what, q, kw) in enumerate(cases):
            want = CM.compute(m, sc["window_small"], q["kf1"], q["kf2"], _tables=tabs, **kw)
            _check(dmap, i, want, cap, (what, cap))
        assert [o["status"] for o in out] == [CM.OK, CM.OK, CM.MISSING_ANCHOR, CM.MISSING_ANCHOR, CM.OK, CM.MISSING_ANCHOR, CM.OK]
        assert out[2]["n_missing"] == 4 and out[3]["n_missing"] == 2 and out[5]["n_missing"] == 1
    assert out[2]["missing"].tolist() == out4[:1] and out[3]["missing"].tolist() == [out4[0]]
    # the cached pose decides the depths: different from the run with every anchor in the window
    dmap.set_window(sc["window_all"])
    inside = dmap.compute_constraints([dict(kf1=A, kf2=B)], depth_cap=DEPTH_CAP)[0]
    assert (inside["depths"] != CM.compute(m, sc["window_small"], A, B, _tables=tabs, cached=cached)["depths"]).sum() > 500


@pytest.mark.gpu
def test_same_bytes_alone_in_a_batch_of_16_and_repeated(gpu_ctx, dmap, sc, tabs):
    ids = sc["ids"]
    dmap.set_window(sc["window_small"])
    cached = _absolute(sc, tabs)
    q = dict(kf1=ids["A"], kf2=ids["B"], cached=cached)
    fill = [dict(kf1=ids[a], kf2=ids[b], cached=cached) for a, b in (PAIRS * 2)[:15]]
    dmap.compute_constraints([q], depth_cap=DEPTH_CAP)
    alone = (dmap.raw["results"][0].tobytes(), dmap.raw["depths"][0].tobytes(), dmap.raw["missing"][0].tobytes())
    for pos in (0, 7, 15, 7):
        dmap.compute_constraints(fill[:pos] + [q] + fill[pos:], depth_cap=DEPTH_CAP)
        assert (dmap.raw["results"][pos].tobytes(), dmap.raw["depths"][pos].tobytes(), dmap.raw["missing"][pos].tobytes()) == alone, pos


def _edge_scene(ctx, blank, sc):
    ids = sc["ids"]
    d = _fill(ctx, blank, sc["map"])
    d.reserve_edges(32)
    edges = [(ids["A"], ids["B"]), (ids["C"], ids["A"]), (ids["D"], ids["C"]), (ids["B"], ids["F"]), (ids["U"], ids["T"]), (ids["A"], ids["J"])]
    d.add_edges(edges, [10, 20, 30, 40, 50, 60], [0, 1, 2, 0, 1, 2])
    table = CM.EdgeTable()
    for (a, b), s, t in zip(edges, [10, 20, 30, 40, 50, 60], [0, 1, 2, 0, 1, 2]):
        table.insert(a, b, s, t)
    return d, table, edges


def _records(table, edges):
    return np.array([table.record(a, b) for a, b in edges]).tobytes()


@pytest.mark.gpu
def test_storing_requests_set_the_edges_constraint(gpu_ctx, blank, sc, tabs):
    m, ids = sc["map"], sc["ids"]
    d, table, edges = _edge_scene(gpu_ctx[0], blank, sc)
    assert d.edge_info() == (6, 0)
    assert d.get_edges(edges).tobytes() == _records(table, edges)                                # new edges: keys, strength, type, nothing else
    assert d.get_edges([(b, a) for a, b in edges]).tobytes() == _records(table, edges)           # either orientation names the edge
    d.set_window(sc["window_all"])
    # one request per orientation against storage (A < B: T_12 is stored as it is; C > A: its inverse), one that does not store, one that is EMPTY
    reqs = [dict(kf1=ids["A"], kf2=ids["B"], store=True), dict(kf1=ids["C"], kf2=ids["A"], store=True), dict(kf1=ids["D"], kf2=ids["C"], store=False),
            dict(kf1=ids["F"], kf2=ids["B"], store=True), dict(kf1=ids["A"], kf2=ids["J"], store=True)]
    out = d.compute_constraints(reqs)
    for q, o in zip(reqs, out):
        want = CM.compute(m, sc["window_all"], q["kf1"], q["kf2"], _tables=tabs)
        assert o["status"] == want["status"] and o["info"].tobytes() == want["info"].tobytes()
        if q["store"] and want["status"] == CM.OK:
            table.set_constraint(q["kf1"], q["kf2"], want["T_12"], want["info"])
    assert out[4]["status"] == CM.EMPTY
    got = d.get_edges(edges)
    assert got.tobytes() == _records(table, edges)
    assert got["is_marginalized"].tolist() == [1, 1, 0, 1, 0, 0] and d.edge_info() == (6, 3)
    assert got[0]["T_lo_from_hi"].tobytes() == out[0]["T_12"].tobytes() and got[1]["T_lo_from_hi"].tobytes() != out[1]["T_12"].tobytes()
    # a missing anchor stores nothing
    d.set_window(sc["window_small"])
    o = d.compute_constraints([dict(kf1=ids["D"], kf2=ids["C"], store=True)])[0]
    assert o["status"] == CM.MISSING_ANCHOR and d.get_edges(edges).tobytes() == got.tobytes() and d.edge_info() == (6, 3)
    # unmarginalize clears the flag only
    d.unmarginalize([(ids["B"], ids["A"])])
    table.un_marginalize(ids["A"], ids["B"])
    after = d.get_edges(edges)
    assert after.tobytes() == _records(table, edges) and after[0]["T_lo_from_hi"].tobytes() == got[0]["T_lo_from_hi"].tobytes() and d.edge_info() == (6, 2)
    # setConstraint with the caller's own values, in both orientations
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE
    rng = np.random.default_rng(8)
    cons = np.zeros(2, BA_CONSTRAINT_DTYPE)
    for c, (p1, p2) in zip(cons, ((ids["T"], ids["U"]), (ids["F"], ids["B"]))):                  # pose1 < pose2: T_21 is T_hi_from_lo; pose1 > pose2: T_lo_from_hi
        T_21 = CM.pose_mul(tabs[1][p2], CM.pose_inv(tabs[1][p1]))
        c["T_21"], c["info"], c["pose1"], c["pose2"] = T_21, np.diag(rng.uniform(1, 9, 6)).reshape(36), p1, p2
        table.set_constraint(p2, p1, T_21, c["info"])
    d.set_constraints(cons)
    assert d.get_edges(edges).tobytes() == _records(table, edges) and d.edge_info() == (6, 3)
    d.close()


def _raw_compute(d, reqs, missing_cap=4, depth_cap=0, n=None):
    """the C call itself (the Python wrapper sorts the cached ids): reqs are MapConstraintRequest structures"""
    from scavislam_amd.ctypes_types import MAP_CONSTRAINT_RESULT_DTYPE, MapConstraintRequest
    n = len(reqs) if n is None else n
    arr = (MapConstraintRequest * max(len(reqs), 1))(*reqs)
    res = np.zeros(max(n, 1), MAP_CONSTRAINT_RESULT_DTYPE)
    missing = np.zeros((max(n, 1), max(missing_cap, 1)), np.int32)
    depths = np.zeros((max(n, 1), max(depth_cap, 1)))
    return d.ctx.lib.svs_map_compute_constraints(d.h, n, arr, missing_cap, res.ctypes.data, missing.ctypes.data, depth_cap, depths.ctypes.data if depth_cap else None)


def _req(kf1, kf2, store=0, cached_ids=None, cached_T=None):
    from scavislam_amd.ctypes_types import MapConstraintRequest
    r = MapConstraintRequest()
    r.kf1, r.kf2, r.store = kf1, kf2, store
    if cached_ids is not None:
        r.n_cached, r.cached_ids, r.cached_T = len(cached_ids), cached_ids.ctypes.data, cached_T.ctypes.data
    return r


@pytest.mark.gpu
def test_refusals_leave_the_edge_table_as_it_was(gpu_ctx, blank, sc, tabs):
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE, MAP_CONS_MAX_REQUESTS
    ctx = gpu_ctx[0]
    ids = sc["ids"]
    INVALID, CAPACITY = 1, 4
    # without svs_map_reserve_edges every edge call is a capacity refusal
    bare = _fill(ctx, blank, sc["map"])
    for call in (lambda: bare.add_edges([(ids["A"], ids["B"])], 1, 0), lambda: bare.unmarginalize([(ids["A"], ids["B"])]), lambda: bare.get_edges([(ids["A"], ids["B"])]),
                 lambda: bare.set_constraints(np.zeros(1, BA_CONSTRAINT_DTYPE)), lambda: bare.compute_constraints([dict(kf1=ids["A"], kf2=ids["B"], store=True)])):
        with pytest.raises(SvsError, match="status 4"):
            call()
    assert bare.edge_info() == (0, 0)
    bare.close()
    d, table, edges = _edge_scene(ctx, blank, sc)
    d.set_window(sc["window_all"])
    d.compute_constraints([dict(kf1=ids["A"], kf2=ids["B"], store=True)])
    snap, info = d.get_edges(edges).tobytes(), d.edge_info()
    assert info == (6, 1)
    A, B, unknown = ids["A"], ids["B"], 101
    asc = np.array([CM.kf_id(12), CM.kf_id(13)], np.int32)
    T2 = np.zeros((2, 12))
    cases = [
        ("unknown kf1", lambda: _raw_compute(d, [_req(unknown, B)]), INVALID),
        ("unknown kf2", lambda: _raw_compute(d, [_req(A, 7000)]), INVALID),
        ("kf1 == kf2", lambda: _raw_compute(d, [_req(A, A)]), INVALID),
        ("cached list descending", lambda: _raw_compute(d, [_req(A, B, cached_ids=asc[::-1].copy(), cached_T=T2)]), INVALID),
        ("cached id twice", lambda: _raw_compute(d, [_req(A, B, cached_ids=asc[[0, 0]].copy(), cached_T=T2)]), INVALID),
        ("a bad request behind a storing one", lambda: _raw_compute(d, [_req(ids["C"], A, store=1), _req(A, A)]), INVALID),
        ("store without the edge", lambda: _raw_compute(d, [_req(A, ids["D"], store=1)]), INVALID),
        ("two storing requests for one edge", lambda: _raw_compute(d, [_req(ids["C"], A, store=1), _req(A, ids["C"], store=1)]), INVALID),
        ("more requests than the capacity", lambda: _raw_compute(d, [_req(A, B)] * (MAP_CONS_MAX_REQUESTS + 1)), CAPACITY),
        ("more cached poses than keyframes fit", lambda: _raw_compute(d, [_req(A, B, cached_ids=np.arange(CAPS["max_keyframes"] + 1, dtype=np.int32),
                                                                              cached_T=np.zeros((CAPS["max_keyframes"] + 1, 12)))]), CAPACITY),
        ("a depth row shorter than kf1's feature_table", lambda: _raw_compute(d, [_req(A, B)], depth_cap=1500), CAPACITY),
    ]
    for what, call, status in cases:
        assert call() == status, what
        assert d.get_edges(edges).tobytes() == snap and d.edge_info() == info, what
    wrapped = [
        ("id1 == id2", lambda: d.add_edges([(A, A)], 1, 0), 1),
        ("an edge already present", lambda: d.add_edges([(ids["G"], ids["H"]), (B, A)], 1, 0), 1),
        ("an edge twice in the call", lambda: d.add_edges([(ids["G"], ids["H"]), (ids["H"], ids["G"])], 1, 0), 1),
        ("an unknown keyframe", lambda: d.add_edges([(ids["G"], unknown)], 1, 0), 1),
        ("a type outside 0 .. 2", lambda: d.add_edges([(ids["G"], ids["H"])], 1, 3), 1),
        ("more edges than reserved", lambda: d.add_edges([(ids["G"], CM.kf_id(i)) for i in range(7, 19)] + [(ids["H"], CM.kf_id(i)) for i in range(8, 19)]
                                                         + [(ids["I"], CM.kf_id(i)) for i in range(9, 19)], 1, 0), 4),
        ("unmarginalize: no such edge", lambda: d.unmarginalize([(A, B), (ids["G"], ids["H"])]), 1),
        ("unmarginalize: an edge twice", lambda: d.unmarginalize([(A, B), (B, A)]), 1),
        ("get: no such edge", lambda: d.get_edges([(ids["G"], ids["H"])]), 1),
    ]
    for what, call, status in wrapped:
        with pytest.raises(SvsError, match=f"status {status}"):
            call()
        assert d.get_edges(edges).tobytes() == snap and d.edge_info() == info, what
    bad = np.zeros(2, BA_CONSTRAINT_DTYPE)
    bad["pose1"], bad["pose2"] = [A, ids["G"]], [B, ids["H"]]
    with pytest.raises(SvsError, match="status 1"):
        d.set_constraints(bad)                                                                   # the second edge does not exist: the first is not set either
    assert d.get_edges(edges).tobytes() == snap and d.edge_info() == info
    # and the table still works
    d.add_edges([(ids["G"], ids["H"])], 5, 1)
    assert d.edge_info() == (7, 1) and d.get_edges(edges).tobytes() == snap
    d.close()


@pytest.mark.gpu
def test_update_marginalization_follows_the_reference_s_two_loops(gpu_ctx, blank, sc, tabs):
    m, ids = sc["map"], sc["ids"]
    d, table, edges = _edge_scene(gpu_ctx[0], blank, sc)
    names = lambda s: [ids[c] for c in s]
    old = (names("ABCDF"), [0, 0, 0, 0, 1])
    new = (names("BCDFT") + sc["outside"][:2], [0, 0, 1, 1, 0, 1, 1])                            # A leaves the window, D moves to OUTER
    d.set_window(new[0])
    # (A, B), (A, C), (C, D) were INNER pairs and are not any more; two of their anchors are neither in the window nor cached yet
    res, missing = d.update_marginalization(old, new)
    first = [CM.compute(m, new[0], a, b, _tables=tabs) for a, b in ((ids["A"], ids["B"]), (ids["A"], ids["C"]), (ids["C"], ids["D"]))]
    assert [o["status"] for o in res] == [o["status"] for o in first] == [CM.MISSING_ANCHOR] * 3
    assert missing == sorted({int(k) for o in first for k in o["missing"]}) and ids["A"] in missing and len(missing) >= 3      # A left the window: its pose is the graph's to give
    assert d.edge_info() == (6, 0)
    cached = {k: [v - 0.03125 for v in tabs[1][k]] for k in missing}
    res, missing = d.update_marginalization(old, new, cached=cached)
    assert missing == [] and [o["status"] for o in res] == [CM.OK] * 3
    for a, b in ((ids["A"], ids["B"]), (ids["A"], ids["C"]), (ids["C"], ids["D"])):
        want = CM.compute(m, new[0], a, b, _tables=tabs, cached=cached)
        table.set_constraint(a, b, want["T_12"], want["info"])
    assert d.get_edges(edges).tobytes() == _records(table, edges) and d.edge_info() == (6, 3)
    # the next window takes A and C back into the inner window: their edge is unmarginalised, (C, D) stays
    d.set_window(names("ABCD"))
    res, missing = d.update_marginalization(new, (names("ABCD"), [0, 1, 0, 1]))
    table.un_marginalize(ids["A"], ids["C"])
    assert res == [] and d.get_edges(edges).tobytes() == _records(table, edges) and d.edge_info() == (6, 2)
    d.close()


# ---- end to end: the window's constraints from the edge table -------------------------------------------------------------------------------------------------
def _rel_update_err(new, ref, start):      # the bar of tests/test_gpu_ba.py and tests/test_gpu_ba_map.py
    upd = np.abs(ref - start).max()
    return np.abs(new - ref).max() / max(upd, 1e-300)


@pytest.mark.gpu
def test_window_from_map_edges_equals_from_map_fed_the_model_s_list(gpu_ctx, sc):
    import torch
    import oracle as O
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import BaParams, Cam
    ctx, stream = gpu_ctx
    bsc = BM.scene()
    m = bsc["map"]
    w, h = int(bsc["cam"]["w"]), int(bsc["cam"]["h"])
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((h >> l, w >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    ctx.sync()
    d = _fill(ctx, (pyr, disp), m, measured=True)
    c = bsc["cam"]
    cam = Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"])
    res, wid, wtype = d.prepare_window(bsc["w0_ids"], bsc["w0_types"], bsc["pairs"])
    prep = BM.prepare(m, bsc["w0_ids"], bsc["w0_types"], bsc["pairs"])
    assert np.array_equal(wid, prep["window_ids"]) and (wtype == 1).sum() >= 4 and len(wid) > len(bsc["w0_ids"])
    # the edge table: the scene's pairs and the chain between every two consecutive keyframes; marginalised (by computeConstraint on the device, every keyframe
    # outside the window with a cached pose) wherever an end is OUTER in the final window
    kf = [int(k) for k in m["kf_ids"]]
    keys = sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in bsc["pairs"]} | {(kf[i], kf[i + 1]) for i in range(len(kf) - 1)})
    d.reserve_edges(len(keys) + 4)
    d.add_edges(keys, 30, 0)
    table = CM.EdgeTable()
    for a, b in keys:
        table.insert(a, b, 30, 0)
    types = dict(zip(wid.tolist(), wtype.tolist()))
    outer_edges = [(a, b) for a, b in keys if a in types and b in types and (types[a] == 1 or types[b] == 1)]
    assert len(outer_edges) >= 4
    tabs = CM.tables(m)
    cached = {k: tabs[1][k] for k in kf if k not in types}
    reqs = [dict(kf1=(a if i % 2 == 0 else b), kf2=(b if i % 2 == 0 else a), store=True, cached=cached) for i, (a, b) in enumerate(outer_edges)]
    out = d.compute_constraints(reqs)
    for q, o in zip(reqs, out):
        want = CM.compute(m, wid.tolist(), q["kf1"], q["kf2"], _tables=tabs, cached=cached)
        assert o["status"] == want["status"] == CM.OK and o["T_12"].tobytes() == want["T_12"].tobytes() and o["info"].tobytes() == want["info"].tobytes(), (q["kf1"], q["kf2"])
        table.set_constraint(q["kf1"], q["kf2"], want["T_12"], want["info"])
    assert d.get_edges(keys).tobytes() == _records(table, keys)
    cons = CM.constraint_list(wid, wtype, table)
    assert len(cons) == 2 * len(outer_edges)
    a, b = SlamGraphOptimizer(ctx, stream), SlamGraphOptimizer(ctx, stream)
    a.windowFromMap(d, None, cam)                                                                # the constraints come from the edge table
    b.windowFromMap(d, cons, cam)
    state = lambda o: tuple(x.tobytes() for x in o.restoreDataFromG2o()) + (o.window_edges().tobytes(),)
    info = lambda o: tuple(o.info()[k] for k in ("solve_kernel", "envelope_rows", "wave_chunks", "wide_landmarks"))
    assert (a.P, a.L) == (b.P, b.L) == (len(wid), len(prep["active_ids"]))
    assert state(a) == state(b) and info(a) == info(b)
    ca, cb = a.window_constraints(), b.window_constraints()
    assert len(ca) == len(cons) and ca.tobytes() == cb.tobytes() == CM.constraint_list(wid, wtype, table, by_index=True).tobytes()
    # an edge with an OUTER end that is not marginalised: refused, the handle keeps its problem
    before = state(a), a.window_constraints().tobytes()
    d.unmarginalize([outer_edges[0]])
    with pytest.raises(SvsError, match="status 1"):
        a.windowFromMap(d, None, cam)
    assert (state(a), a.window_constraints().tobytes()) == before
    d.compute_constraints([reqs[0]])                                                             # marginalised again, the same bytes
    assert d.get_edges(keys).tobytes() == _records(table, keys)
    # optimize on both handles: the comparison tests/test_gpu_ba_map.py holds its two paths to
    prob = BM.problem(m, prep["window_ids"], prep["active_ids"])
    prm = BaParams.reference_defaults()
    poses_ref, psi_ref, st_ref = O.ba_optimize(prob["poses"], prob["psi"], a.window_edges(), ca, cam, prm)
    assert st_ref.accepted >= 1 and st_ref.chi2_final < st_ref.chi2_init
    for name, opt in (("from the edge table", a), ("from the model's list", b)):
        st = opt.optimize()
        poses, psi = opt.restoreDataFromG2o()
        assert (st.iterations, st.trials, st.accepted, st.terminated) == (st_ref.iterations, st_ref.trials, st_ref.accepted, st_ref.terminated), name
        ep, el = _rel_update_err(poses, poses_ref, prob["poses"]), _rel_update_err(psi, psi_ref, prob["psi"])
        print(f"{name}: pose update rel err {ep:.2e}, psi {el:.2e}")
        assert ep < 1e-6 and el < 1e-6, name
    a.storeToMap(d)                                                                              # the handle's problem is the map's prepared window
    for o in (a, b):
        o.close()
    d.close()


@pytest.mark.gpu
def test_cpp_adaptor_edges_and_constraints(gpu_ctx, tmp_path):
    """tests/cpp/constraints_smoke.cpp: BackendMap::reserveEdges / addEdges / computeConstraints / updateMarginalization and SlamGraphBA::copyDataFromMap without
    constraints of include/scavislam_hip.hpp, against the depths, median and Lambda the program forms on the host"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "constraints_smoke"
    libdir = os.path.join(root, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "constraints_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("CONSTRAINTS ")]
    assert tok and tok[0].split()[1] == "ok" and int(tok[0].split()[2]) >= 60 and tok[0].split()[3] == "4", out
