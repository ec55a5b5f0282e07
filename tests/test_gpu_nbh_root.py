"""GPU tests of svs_frontend_set_neighborhood_from_root: a stream's whole neighbourhood from a root id, built on the device from the resident map.  Every output
is held, byte for byte, against tests/nbh_root_model.py on a host mirror of the same map, and against a TWIN front end that is fed through the four calls the
feature joins -- ResidentMap.neighbors_of_root, absolute_poses (put into a twin map by set_poses), setCandidatesFromMap and setVertexTable, its head ordered by the
model; after one step the decideKeyframes records of the two are the same bytes.  Scene: register_model.make_scene() at SMALL_CAM put into a map by
register_map_model.fill(), extended by nbh_root_model.extend() and its edge table (21 keyframes, 20 edges)."""
import os
import subprocess

import numpy as np
import pytest

import nbh_root_model as RM
import register_map_model as MM
import register_model as M
from test_gpu_neighborhood import device_scene, scene      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = M.SMALL_CAM
K, VCAP, MAXP = 16, 16, 640
SLOT_IDS = [7, 13, 19, 25, 40, RM.HUB, RM.LONE, 52]
INVALID, CAPACITY = "status 1", "status 4"
HUB, LONE = RM.HUB, RM.LONE


def slots(missing=()):
    return [(-1 if k in missing else k) for k in SLOT_IDS] + [-1] * (K - len(SLOT_IDS))


def _fill(m):
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE
    if hasattr(m, "reserve_edges"):
        m.reserve_edges(len(RM.EDGES) + 4)
        m.add_edges([(a, b) for a, b, _, _ in RM.EDGES], [s for _, _, s, _ in RM.EDGES], [t for _, _, _, t in RM.EDGES])
        marg = RM.new_poses()[1]
        cons = np.zeros(len(marg), BA_CONSTRAINT_DTYPE)
        for c, ((lo, hi), (T, info)) in zip(cons, marg.items()):      # pose1 > pose2: T_21 is T_lo_from_hi as it is stored
            c["T_21"], c["info"], c["pose1"], c["pose2"] = T, info, hi, lo
        m.set_constraints(cons)


def _device_map(ctx, dev, scene):
    from test_gpu_register_map import DeviceMap
    d = DeviceMap(ctx, dev, scene, max_keyframes=128, max_points=2048, max_observations=8192)
    MM.fill(d, scene, cand_ids_few=scene["src"]["point_id"][:10], attach=lambda e: dict(entry=e))
    RM.extend(d)
    _fill(d)
    return d


@pytest.fixture(scope="module")
def both(gpu_ctx, device_scene, scene):
    model = MM.MapModel()
    MM.fill(model, scene, cand_ids_few=scene["src"]["point_id"][:10], attach=lambda e: dict(entry=e))
    RM.extend(model)
    dmap = _device_map(gpu_ctx[0], device_scene, scene)
    yield model, RM.edge_table(), dmap
    dmap.close()


@pytest.fixture(scope="module")
def host_frames(scene):
    """the scene's keyframes 1 .. 4 rendered as make_scene renders them, a frame at the root's stored pose (the active keyframe), the root's own image (current)"""
    from scavislam_amd import synth
    sc = synth.Scene(2011)
    n_other = len(scene["kf_T"]) - 1
    traj = synth.trajectory(2 * n_other + 2)
    order = [k for k in range(2 * n_other + 1) if k != n_other][:n_other]
    host = [sc.render(CAM, traj[k], seed=k) for k in order]
    host.append(sc.render(CAM, scene["T_root"].reshape(3, 4), seed=41))
    host.append((scene["root_pyr"][0], scene["root_disp"]))
    return host


@pytest.fixture(scope="module")
def frames_of(gpu_ctx, host_frames):
    """B -> device frames [B][h][w] (every stream sees the same camera)"""
    import torch
    ctx, stream = gpu_ctx
    cache = {}

    def get(B):
        if B not in cache:
            with torch.cuda.stream(stream):
                out = [dict(left=torch.as_tensor(np.stack([img] * B)).cuda(), disp=torch.as_tensor(np.stack([disp] * B).astype(np.float32)).cuda())
                       for img, disp in host_frames]
            stream.synchronize()
            cache[B] = dict(kf=out[:-2], act=out[-2], cur=out[-1])
        return cache[B]
    return get


def _off(T, d):
    T = np.array(T, np.float64).reshape(12).copy()
    T[3] += d; T[7] -= 0.5 * d
    return T


def _make_fe(ctx, frames_of, model, B=2, max_points=MAXP, stale=0.05):
    """B streams with the scene's keyframes in slots 0 .. 3, the active keyframe's frame in slots 4 .. 7 (ids SLOT_IDS), every pose `stale` metres off the map's"""
    from scavislam_amd.frontend import StereoFrontend
    fr = frames_of(B)
    fe = StereoFrontend(ctx, CAM, max_points=max_points, max_keyframes=K, n_streams=B)
    for s, k in enumerate(SLOT_IDS):
        fe.processFirstFrames(**(fr["kf"][s] if s < len(fr["kf"]) else fr["act"]))
        fe.keepKeyframes(s, np.stack([_off(model.kf[k]["T"], stale)] * B))
    return fe


def _step(fe, frames_of, scene):
    B = fe.n_streams
    fe.processFrames(np.stack([np.array(M.I12)] * B), np.stack([scene["T_root"].reshape(12)] * B), **frames_of(B)["cur"])
    out = []
    for b in range(B):
        res, m, g = fe.results(b)
        out.append((bytes(res), m.tobytes(), g.tobytes(), int(res.n_matched)))
    return out


def _head(scene, sizes, first_id=3000):
    n = sum(sizes)
    head = np.array(scene["src"][:n])
    head["kf_index"] = np.arange(n) % 4
    head["point_id"] = first_id + np.arange(n)
    return head, [int(e) for e in np.cumsum(sizes)]


def _q(stream, root, act, max_nn=10, slot_kf=None, head=None, ge=None, n_fixed=None, keys=None):
    q = dict(stream=stream, root_id=root, act_id=act, max_num_neighbors=max_nn, slot_kf=slots() if slot_kf is None else slot_kf)
    if head is not None:
        q.update(head=head, head_group_end=ge, n_fixed_groups=len(ge) if n_fixed is None else n_fixed, head_group_kf=[-1] * len(ge) if keys is None else keys)
    return q


def _keyed(scene, stream, root, act, max_nn=10, **kw):
    """two fixed groups, then groups keyed by 13, 7 (never a neighbour of the active keyframe: dropped), 19, HUB and an empty one keyed by 41"""
    head, ge = _head(scene, [3, 2, 4, 5, 1, 6, 0])
    return _q(stream, root, act, max_nn, head=head, ge=ge, n_fixed=2, keys=[-1, -1, 13, 7, 19, HUB, 41], **kw)


def _state(o, b):
    """everything of stream b the call may write, as it lies on the device behind the call"""
    return o["table"][b].tobytes(), o["kf_table"].tobytes(), o["kf_vertex"].tobytes()


def _check(fe, dmap, model, table, reqs, refresh=True, vertex_cap=VCAP):
    """the call's outputs against the model -> (outputs, the model's)"""
    outs = fe.setNeighborhoodFromMap(dmap.map, reqs, refresh_poses=refresh, vertex_cap=vertex_cap, want_records=True, want_tables=True)
    wants = []
    for o, q in zip(outs, reqs):
        w = RM.build(model, table, q, max_points=fe.max_points, vertex_cap=vertex_cap)
        wants.append(w)
        got = tuple(o[f] for f in RM.FIELDS)
        print("request", q["root_id"], q["act_id"], q["max_num_neighbors"], "->", dict(zip(RM.FIELDS, got)))
        assert got == RM.result_fields(w), (q["root_id"], q["act_id"])
        res, pid, vid, vT, act, strength = o["raw"]
        if w["over_capacity"] or w["root_outside_window"]:
            for row in (pid, vid, act, strength):
                assert (np.frombuffer(row, np.int32) == -1).all()
            assert not np.frombuffer(vT, np.uint8).any() and not o["slot_T"].any()
            continue
        n, nv, na = w["n_points"], w["n_vertex"], w["n_act_neighbors"]
        row = o["table"][q["stream"]]
        assert row[:n].tobytes() == w["records"].tobytes()
        assert (row[n:].view(np.uint8) == 0xff).all()                                   # "no candidate" behind the list
        assert np.array_equal(np.frombuffer(pid, np.int32), np.concatenate([w["point_ids"], np.full(fe.max_points - n, -1, np.int32)]))
        assert np.array_equal(np.frombuffer(vid, np.int32), np.concatenate([w["vertex_ids"], np.full(vertex_cap - nv, -1, np.int32)]))
        assert vT == np.concatenate([w["vertex_T"], np.zeros((vertex_cap - nv, 12))]).tobytes()
        assert np.array_equal(np.frombuffer(act, np.int32), np.concatenate([w["act_neighbors"], np.full(vertex_cap - na, -1, np.int32)]))
        assert strength == w["strength"].tobytes()
        assert o["kf_table"].tobytes() == w["kf_table"].tobytes() and o["kf_vertex"].tobytes() == w["kf_vertex"].tobytes()
        slot_T = np.zeros((K, 12))
        if refresh:
            for s, T in w["slot_T"].items():
                slot_T[s] = T
        assert o["slot_T"].tobytes() == slot_T.tobytes()
        assert fe.n_points[q["stream"]] == n
    return outs, wants


@pytest.fixture(scope="module")
def list_fe(gpu_ctx, frames_of, both):
    fe = _make_fe(gpu_ctx[0], frames_of, both[0])
    yield fe
    fe.close()


# ---- 1. every output against the model ---------------------------------------------------------------------------------------------------------------------------
CASES = [("hub_13_neighbours_cap_10", HUB, 40, 10), ("hub_cap_0", HUB, 40, 0), ("hub_cap_12", HUB, HUB, 12), ("hub_cap_above_the_row", HUB, 19, 20),
         ("ties_by_slot_then_by_id_anchors_outside", 40, 40, 10), ("root_and_act_without_edges", LONE, LONE, 10), ("act_absent", 40, 3, 10),
         ("act_is_an_anchor_outside_the_window", 40, 7, 10), ("cap_1", 40, 13, 1), ("root_13", 13, 40, 10)]


@pytest.mark.parametrize("name,root,act,max_nn", CASES, ids=[c[0] for c in CASES])
def test_outputs_equal_the_model(list_fe, both, scene, name, root, act, max_nn):
    model, table, dmap = both
    for stream, refresh, missing in ((0, True, ()), (1, False, (25, 13))):
        q = _keyed(scene, stream, root, act, max_nn, slot_kf=slots(missing))
        outs, wants = _check(list_fe, dmap, model, table, [q], refresh=refresh)
        assert not outs[0]["over_capacity"] and not outs[0]["root_outside_window"]
    o = outs[0]
    if name == "hub_13_neighbours_cap_10":
        assert o["n_root_neighbors"] == 11 and list(o["vertex_ids"][1:4]) == [78, 77, 76]            # 77 before 76: the slot decides
    if name == "hub_cap_0":
        assert o["n_root_neighbors"] == 1 and list(o["vertex_ids"]) == [HUB, 78] and o["act_index"] == -1
    if name == "hub_cap_above_the_row":
        assert o["n_root_neighbors"] == 13 and 50 not in o["vertex_ids"] and RM.OUT_LEAF not in o["vertex_ids"]
    if name == "ties_by_slot_then_by_id_anchors_outside":
        assert list(o["vertex_ids"]) == [40, 19, 13, HUB, 7, 25] and [int(o["vertex_ids"][j]) for j in o["act_neighbors"]] == [13, 19, HUB]
        assert o["n_no_path"] == 1 and o["n_head_dropped"] == 5 + 0 and o["n_groups"] == 2 + 3 + 1    # keyed by 7 and by 41: dropped
        path = dmap.absolute_poses([7], path_cap=8)[0]
        assert list(path["path"]) == [7, RM.N1, 13] and o["vertex_T"][4].tobytes() == path["T"].tobytes()
    if name == "root_and_act_without_edges":
        assert list(o["vertex_ids"]) == [LONE, 7] and o["n_act_neighbors"] == 0 and o["act_index"] == 0 and o["n_head_kept"] == 5
    if name == "act_absent":
        assert o["act_index"] == -1 and o["kf_table"]["act"] == -1 and o["n_head_kept"] == 5 and o["n_points"] == 5 + o["n_map_points"]


def test_a_root_outside_the_window_leaves_the_stream_untouched(list_fe, both, scene):
    model, table, dmap = both
    before, _ = _check(list_fe, dmap, model, table, [_keyed(scene, 0, 40, 40)])
    n = list(list_fe.n_points)
    outs, _ = _check(list_fe, dmap, model, table, [_keyed(scene, 0, 7, 7), _q(1, LONE, LONE)])
    assert outs[0]["root_outside_window"] == 1 and outs[1]["root_outside_window"] == 0
    assert _state(outs[0], 0) == _state(before[0], 0) and list_fe.n_points[0] == n[0]


# ---- 2. capacity ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_at_the_edge_and_one_past_it(list_fe, both, scene):
    model, table, dmap = both
    fit = RM.build(model, table, _keyed(scene, 0, 40, 40))
    room = MAXP - fit["n_points"]                                     # grow the first fixed group until the list is exactly max_points long

    def grown(extra):
        head, ge = _head(scene, [3 + extra, 2, 4, 5, 1, 6, 0])
        return _q(0, 40, 40, head=head, ge=ge, n_fixed=2, keys=[-1, -1, 13, 7, 19, HUB, 41])

    outs, wants = _check(list_fe, dmap, model, table, [grown(room)])
    assert outs[0]["n_points"] == MAXP and not outs[0]["over_capacity"]
    full = _state(outs[0], 0)
    outs, _ = _check(list_fe, dmap, model, table, [grown(room + 1), _q(1, LONE, LONE)])      # (d): one record more; the other request is answered
    assert outs[0]["over_capacity"] == 1 and outs[0]["n_points"] == MAXP + 1 and outs[0]["n_head_dropped"] == 5 and outs[1]["over_capacity"] == 0
    assert _state(outs[0], 0) == full and list_fe.n_points[0] == MAXP
    outs, _ = _check(list_fe, dmap, model, table, [grown(room + 12)])                        # (b): the fixed groups alone do not fit
    assert outs[0]["over_capacity"] == 1 and outs[0]["n_vertex"] == 0 and _state(outs[0], 0) == full
    nv = fit["n_vertex"]
    outs, _ = _check(list_fe, dmap, model, table, [_keyed(scene, 0, 40, 40)], vertex_cap=nv)
    assert outs[0]["n_vertex"] == nv and not outs[0]["over_capacity"]
    small = _state(outs[0], 0)
    outs, _ = _check(list_fe, dmap, model, table, [_keyed(scene, 0, 40, 40)], vertex_cap=nv - 1)   # (c)
    assert outs[0]["over_capacity"] == 1 and outs[0]["n_vertex"] == nv and _state(outs[0], 0) == small
    outs, _ = _check(list_fe, dmap, model, table, [_keyed(scene, 0, HUB, 40)], vertex_cap=12)      # the root and eleven neighbours fit exactly, the anchors do not: (c)
    assert outs[0]["over_capacity"] == 1 and outs[0]["n_root_neighbors"] == 11 and outs[0]["n_vertex"] == 15 and outs[0]["n_map_points"] > 0
    outs, _ = _check(list_fe, dmap, model, table, [_keyed(scene, 0, HUB, 40)], vertex_cap=11)      # (a)
    assert outs[0]["over_capacity"] == 1 and outs[0]["n_vertex"] == 12 and outs[0]["n_map_points"] == 0


# ---- 3. the twin front end ---------------------------------------------------------------------------------------------------------------------------------------
def test_twin_front_end_fed_through_the_four_calls(gpu_ctx, device_scene, frames_of, scene, both):
    model, table, dmap = both
    reqs = [_keyed(scene, 0, 40, 40), _keyed(scene, 1, HUB, 40, slot_kf=slots((25,)))]
    twin = _device_map(gpu_ctx[0], device_scene, scene)
    fe = _make_fe(gpu_ctx[0], frames_of, model)
    tfe = _make_fe(gpu_ctx[0], frames_of, model)
    try:
        outside = sorted(k for k in model.kf if not model.kf[k]["window"])
        walked = dmap.absolute_poses(outside)
        ok = [i for i, w in enumerate(walked) if w["status"] == 0]
        assert 7 in [outside[i] for i in ok] and 25 not in [outside[i] for i in ok]
        twin.set_poses([outside[i] for i in ok], [walked[i]["T"] for i in ok])
        outs, wants = _check(fe, dmap, model, table, reqs)
        for q, w, o in zip(reqs, wants, outs):
            b = q["stream"]
            vertex = [q["root_id"]] + [int(k) for k in twin.neighbors_of_root(q["root_id"], q["max_num_neighbors"])]
            t = tfe.setCandidatesFromMap(twin.map, [dict(stream=b, vertex_kf=vertex, slot_kf=q["slot_kf"], head=w["records"][:w["n_new"]],
                                                         head_group_end=w["group_end"][:-1])], refresh_poses=True, vertex_cap=VCAP, want_records=True)[0]
            tfe.setVertexTable([dict(stream=b, vertex_kf=t["vertex_ids"], vertex_T=t["vertex_T"], sets=["map"] * len(t["vertex_ids"]), act=w["act_index"],
                                     neighbors=w["act_neighbors"], slot_kf=q["slot_kf"])])
            assert t["table"][b].tobytes() == o["table"][b].tobytes()
            assert t["vertex_T"].tobytes() == o["vertex_T"].tobytes() and list(t["vertex_ids"]) == list(o["vertex_ids"])
        # the twin's resident rows: a request that leaves its stream untouched reads them back
        for q, o in zip(reqs, outs):
            back = tfe.setNeighborhoodFromMap(twin.map, [_q(q["stream"], 7, 7, slot_kf=q["slot_kf"])], want_tables=True)[0]
            assert back["root_outside_window"] == 1
            assert back["kf_table"].tobytes() == o["kf_table"].tobytes() and back["kf_vertex"].tobytes() == o["kf_vertex"].tobytes()
        a, b = _step(fe, frames_of, scene), _step(tfe, frames_of, scene)
        print("n_matched", [s[3] for s in a])
        assert a == b and a[0][3] >= 20                              # the refinement and the gate really ran; the slot poses are the same
        da, db = fe.decideKeyframes(dmap.map, want_lists=2), tfe.decideKeyframes(twin.map, want_lists=2)
        for x, y in zip(da, db):
            assert x["dec"].tobytes() == y["dec"].tobytes() and x["dec"]["valid"] == 1
            for f in ("new", "track", "new_rec", "track_rec"):
                assert x[f].tobytes() == y[f].tobytes()
    finally:
        fe.close(); tfe.close(); twin.close()


# ---- 4. batching, repetition, the map unchanged ------------------------------------------------------------------------------------------------------------------
def _map_bytes(dmap, model):
    kfs, pts = sorted(model.kf), sorted(model.pt)
    tabs = []
    for k in kfs:
        ids, meas = dmap.get_feature_table(k)[:2]
        tabs.append((np.asarray(ids).tobytes(), np.asarray(meas).tobytes()))
    return (dmap.get_points(pts).tobytes(), dmap.get_poses(kfs).tobytes(), dmap.get_edges([(a, b) for a, b, _, _ in RM.EDGES]).tobytes(), tabs, dmap.edge_info(),
            dmap.info())


def test_a_batch_of_33_equals_each_stream_alone_a_repetition_and_leaves_the_map_as_it_was(gpu_ctx, frames_of, scene, both):
    model, table, dmap = both
    B = 33
    roots = [(HUB, 40, 10), (40, 40, 10), (LONE, LONE, 10), (7, 7, 10), (HUB, HUB, 0), (40, 3, 1), (13, 40, 10), (HUB, 19, 20)]
    reqs = [_keyed(scene, b, *roots[b % len(roots)], slot_kf=slots((25,) if b % 3 == 0 else ())) for b in range(B)]
    fe = _make_fe(gpu_ctx[0], frames_of, model, B=B)
    try:
        before = _map_bytes(dmap, model)
        outs, wants = _check(fe, dmap, model, table, reqs)
        batch = [(o["raw"], o["slot_T"].tobytes()) + _state(o, q["stream"]) for o, q in zip(outs, reqs)]
        again = fe.setNeighborhoodFromMap(dmap.map, reqs, vertex_cap=VCAP, want_records=True, want_tables=True)
        assert [(o["raw"], o["slot_T"].tobytes()) + _state(o, q["stream"]) for o, q in zip(again, reqs)] == batch
        for q, want in zip(reqs, batch):
            o = fe.setNeighborhoodFromMap(dmap.map, [q], vertex_cap=VCAP, want_records=True, want_tables=True)[0]
            assert (o["raw"], o["slot_T"].tobytes()) + _state(o, q["stream"]) == want, q["stream"]
        assert _map_bytes(dmap, model) == before
        assert sum(o["n_no_path"] for o in outs) > 0 and sum(o["root_outside_window"] for o in outs) == 4
    finally:
        fe.close()


def _vertex_tables(rng, B):
    """a setVertexTable request per stream: 1 .. 5 vertices, staged sets whose sizes differ from stream to stream"""
    reqs = []
    for b in range(B):
        V = 1 + b % 5
        reqs.append(dict(stream=b, vertex_kf=[int(k) for k in rng.permutation(200)[:V]], vertex_T=rng.standard_normal((V, 12)), act=b % V,
                         sets=[[int(i) for i in rng.permutation(5000)[:int(rng.integers(0, 60))]] for _ in range(V)], neighbors=[v for v in range(V) if v != b % V][:3],
                         slot_kf=slots((25,) if b % 3 == 0 else ())))
    return reqs


def test_a_staging_block_that_grows_in_mid_life(gpu_ctx, frames_of, scene, both):
    """one request, then 33 that ask for every optional output, then one again, on ONE front end: the blocks start at twice the first call's need, so the second
    call outgrows them and the third reuses the bigger ones.  setNeighborhoodFromMap: every call against the model, and its outputs and device rows against a fresh
    front end that makes only that call.  setVertexTable: the resident rows of the streams a call names, read back by a request that leaves its stream untouched,
    against those of a fresh front end that makes only that call"""
    model, table, dmap = both
    B = 33
    roots = [(HUB, 40, 10), (40, 40, 10), (LONE, LONE, 10), (HUB, HUB, 0), (40, 3, 1), (13, 40, 10), (HUB, 19, 20)]
    reqs = [_keyed(scene, b, *roots[b % len(roots)], slot_kf=slots((25,) if b % 3 == 0 else ())) for b in range(B)]
    tabs = _vertex_tables(np.random.default_rng(5), B)
    key = lambda outs, rq: [(o["raw"], o["slot_T"].tobytes()) + _state(o, q["stream"]) for o, q in zip(outs, rq)]

    def rows(fe, rq):
        back = fe.setNeighborhoodFromMap(dmap.map, [_q(q["stream"], 7, 7, slot_kf=q["slot_kf"]) for q in rq], want_tables=True)
        assert all(o["root_outside_window"] == 1 for o in back)
        return [(o["kf_table"].tobytes(), o["kf_vertex"].tobytes()) for o in back]

    nbr_calls, tab_calls = [[reqs[0]], reqs, [reqs[1]]], [[tabs[0]], tabs, [tabs[1]]]
    fe = _make_fe(gpu_ctx[0], frames_of, model, B=B)
    try:
        got = [key(_check(fe, dmap, model, table, rq)[0], rq) for rq in nbr_calls]
        assert got[1][0] == got[0][0] and got[2][0] == got[1][1]
        got_tabs = []
        for rq in tab_calls:
            fe.setVertexTable(rq)
            got_tabs.append(rows(fe, rq))
        assert got_tabs[1][0] == got_tabs[0][0] and got_tabs[2][0] == got_tabs[1][1] and len(set(got_tabs[1])) == B
    finally:
        fe.close()
    for nq, rq, g, gt in zip(nbr_calls, tab_calls, got, got_tabs):      # (the two calls stage through blocks of their own: one fresh front end serves both)
        fresh = _make_fe(gpu_ctx[0], frames_of, model, B=B if len(rq) > 1 else 2)
        try:
            outs = fresh.setNeighborhoodFromMap(dmap.map, nq, refresh_poses=True, vertex_cap=VCAP, want_records=True, want_tables=True)
            assert key(outs, nq) == g, f"setNeighborhoodFromMap, {len(nq)} request(s)"
            fresh.setVertexTable(rq)
            assert rows(fresh, rq) == gt, f"setVertexTable, {len(rq)} request(s)"
        finally:
            fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(gpu_ctx, frames_of, host_frames, scene, both):
    from scavislam_amd import capi
    from scavislam_amd.capi import SvsError
    from scavislam_amd.register import ResidentMap
    model, table, dmap = both
    good = _keyed(scene, 0, 40, 40)
    unkept = slots(); unkept[K - 1] = 41
    twice = slots(); twice[0] = twice[1]
    bad_slot = good["head"].copy(); bad_slot["kf_index"][3] = K - 1
    cases = [(INVALID, [good, dict(good, stream=1), dict(good, stream=1)]), (INVALID, [good, good]), (INVALID, [dict(good, stream=2)]),
             (INVALID, [dict(good, root_id=9)]), (INVALID, [dict(good, act_id=9)]), (INVALID, [dict(good, max_num_neighbors=-1)]),
             (INVALID, [dict(good, slot_kf=unkept)]), (INVALID, [dict(good, slot_kf=twice)]),
             (INVALID, [dict(good, head_group_end=[3, 5, 9, 14, 15, 12, 21])]), (INVALID, [dict(good, head_group_end=[3, 5, 9, 14, 15, 21, 20])]),
             (INVALID, [dict(good, head=bad_slot)]), (INVALID, [dict(good, n_fixed_groups=0)]), (INVALID, [dict(good, n_fixed_groups=8)]),
             (INVALID, [dict(good, head_group_kf=[-1, -1, 13, 7, 13, HUB, 41])]),      # one key on two groups
             (INVALID, [dict(good, head_group_kf=[-1, -1, 13, 7, 19, HUB, 9])]),       # a key that is no keyframe of the map
             (CAPACITY, [dict(good, head_group_end=[0] * 63 + [21], head_group_kf=[-1] * 64, n_fixed_groups=64)])]
    fe = _make_fe(gpu_ctx[0], frames_of, model)
    other = capi.Context(0)
    try:
        foreign = ResidentMap(other, max_keyframes=8, max_points=8, max_observations=8)
        outs, _ = _check(fe, dmap, model, table, [good, _q(1, LONE, LONE)])
        state = [_state(o, b) for b, o in enumerate(outs)]
        for code, reqs in cases:
            with pytest.raises(SvsError, match=code):
                fe.setNeighborhoodFromMap(dmap.map, reqs, vertex_cap=VCAP)
        for cap in (0, 65):
            with pytest.raises(SvsError, match=INVALID):
                fe.setNeighborhoodFromMap(dmap.map, [good], vertex_cap=cap)
        with pytest.raises(SvsError, match=INVALID):                                     # fe and map on different contexts
            fe.setNeighborhoodFromMap(foreign, [good], vertex_cap=VCAP)
        foreign.close()
        back = fe.setNeighborhoodFromMap(dmap.map, [_q(0, 7, 7), _q(1, 7, 7)], vertex_cap=VCAP, want_records=True, want_tables=True)
        assert [_state(o, b) for b, o in enumerate(back)] == state and fe.n_points == [outs[0]["n_points"], outs[1]["n_points"]]
    finally:
        fe.close()
        other.close()
    # between submit_frame and wait_frame the list of the frame in flight is latched
    from scavislam_amd.frontend import StereoFrontend
    one = StereoFrontend(gpu_ctx[0], CAM, max_points=MAXP, max_keyframes=K)
    try:
        (act_img, act_disp), (cur_img, cur_disp) = host_frames[-2], host_frames[-1]
        one.processFirstFrame(act_img, disp=np.asarray(act_disp, np.float32))
        one.keepKeyframe(0, scene["T_root"])
        lone_slots = [LONE] + [-1] * (K - 1)
        want = _check(one, dmap, model, table, [_q(0, LONE, LONE, slot_kf=lone_slots)])[1][0]
        one.submitFrame(cur_img, np.array(M.I12), scene["T_root"], disp=np.asarray(cur_disp, np.float32))
        with pytest.raises(SvsError, match=INVALID):
            one.setNeighborhoodFromMap(dmap.map, [_q(0, 40, 40, slot_kf=lone_slots)], vertex_cap=VCAP)
        res, m, g = one.waitFrame()
        assert len(m) == want["n_points"] == 6
    finally:
        one.close()


# ---- 6. the C++ adaptor --------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_smoke_prints_the_models_counts(gpu_ctx, tmp_path):
    """tests/cpp/nbh_root_smoke.cpp builds a small map of its own through BackendMap -- keyframes 0 .. 4 of which 0 .. 2 are in the window, 40 points (point p is
    observed by keyframe p % 4 and anchored in (p / 4) % 4), edges (0, 1, 9) (2, 0, 7) (1, 2, 7) (3, 1, 5) -- and asks StereoFrontend::setNeighborhoodFromMap for
    root 0 with act 1, one fixed group and groups keyed by 2, 4, 0"""
    from constraint_model import EdgeTable
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    model = MM.MapModel()
    model.add_keyframes([0, 1, 2, 3, 4], [M.I12] * 5)
    pts = np.zeros(40, CANDIDATE_DTYPE)
    pts["kf_index"] = (np.arange(40) // 4) % 4
    model.add_points(list(range(40)), pts)
    model.add_observations(list(range(40)), [p % 4 for p in range(40)])
    model.set_window([0, 1, 2])
    table = EdgeTable()
    for a, b, s in ((0, 1, 9), (2, 0, 7), (1, 2, 7), (3, 1, 5)):
        table.insert(a, b, s, 0)
    head = np.zeros(6, CANDIDATE_DTYPE)
    head["point_id"], head["kf_index"] = 100 + np.arange(6), -1
    want = RM.build(model, table, dict(root_id=0, act_id=1, slot_kf=[0, 2], head=head, head_group_end=[1, 3, 4, 6], n_fixed_groups=1, head_group_kf=[-1, 2, 4, 0]))
    exe = tmp_path / "nbh_root_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "nbh_root_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("NBH_ROOT ")]
    assert tok and tok[0].split()[1] == "ok", out
    n = len(RM.FIELDS)
    assert tuple(int(v) for v in tok[0].split()[2:2 + n]) == RM.result_fields(want)
    rest = [int(v) for v in tok[0].split()[2 + n:]]
    nv, na = want["n_vertex"], want["n_act_neighbors"]
    assert rest == [int(k) for k in want["vertex_ids"]] + [int(k) for k in want["act_neighbors"]] + [int(p) for p in want["point_ids"][:want["n_new"]]]
    assert len(rest) == nv + na + want["n_new"]
