"""GPU tests of committing a registration or a loop closure into the device-resident map: svs_reg_commit, svs_map_register_keyframes and svs_map_add_loop_closure
against a twin map that takes the lists of tests/regcommit_model.py through svs_map_add_measured_observations, svs_map_add_edges and a storing
svs_map_compute_constraints, byte for byte; the constraint records, edge list, track list and T_new against the model itself (tests/test_regcommit_cpu.py holds
the model to the reference's loops).  Scene and capacities of tests/test_gpu_register_map.py; the scene's pairs go in with measurements."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import constraint_model as CM
import regcommit_model as RC
import register_map_model as MM
import register_model as M
import walk_model as WM
from test_gpu_register_map import CAM, EXIT3_ID, MAP_CAPS, DeviceMap, device_scene, exit3_ids, few_ids, model_run, scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVIS = M.PARAMS["covis_thr"]
OUTSIDE_ID = 25                                                   # the scene's keyframe outside the double window: in the walk, anchors points, never qualifies


@pytest.fixture(scope="module")
def registrar(gpu_ctx):
    from scavislam_amd.register import KeyframeRegistrar
    reg = KeyframeRegistrar(gpu_ctx[0], CAM, max_requests=8, max_points=512, max_keyframes=8, max_observers=4096)
    yield reg
    reg.close()


class Env:
    """what every case builds maps from"""

    def __init__(self, ctx, dev, scene, few, exit3):
        self.ctx, self.dev, self.scene, self.few, self.exit3, self.open = ctx, dev, scene, few, exit3, []

    def fill(self, m, through=lambda t: t):
        t = through(RC.measured(m))
        MM.fill(t, self.scene, cand_ids_few=self.few, attach=lambda e: dict(entry=e))
        t.add_keyframes([EXIT3_ID], [M.I12], entry=[1])           # the keyframe of the third exit: observes exactly its 16 points
        t.add_observations(self.exit3, [EXIT3_ID] * len(self.exit3))

    def model(self, **kw):
        m = RC.CommitModel()
        self.fill(m, **kw)
        return m

    def device(self, edges=64, through=lambda t: t, **caps):
        d = DeviceMap(self.ctx, self.dev, self.scene, **caps)
        self.open.append(d)
        if edges:
            d.reserve_edges(edges)
        self.fill(d, through=through)
        return d

    def close(self):
        for d in self.open:
            d.close()


@pytest.fixture(scope="module")
def env(gpu_ctx, device_scene, scene, few_ids, exit3_ids):
    e = Env(gpu_ctx[0], device_scene, scene, few_ids, exit3_ids)
    yield e
    e.close()


def _snapshot(d, model):
    """every read-back of a device map, as bytes"""
    kfs = sorted(model.kf)
    edges = sorted(d.edge_keys)
    tables = []
    for k in kfs:
        ids, rec, n = d.get_feature_table(k)
        tables.append((ids.tobytes(), rec.tobytes(), n))
    return (d.info(), d.measured_info(), d.edge_info(), edges, d.get_edges(edges).tobytes() if edges else b"", d.get_poses(kfs).tobytes(), tables)


def _outputs(o):
    """a RegistrationOutput as regcommit_model takes a registration"""
    st = np.stack([o.kf_stats[f] for f in ("strength", "n_u_hi", "n_u_lo", "n_v_hi", "n_v_lo", "qualifies", "in_vertex_table")], 1)
    return dict(status=o.status, cand_src=o.cand_src, accepted=o.accepted, obs=o.matches["obs"], kf_stats=st, T=o.T_newroot_from_oldroot.reshape(12))


def _outside_poses(model):
    return {k: model.kf[k]["T"] for k in model.kf if not model.kf[k]["window"]}


def _apply_on_twin(t, kf, T_new, track, edges, edge_type, other_first, cached):
    """the parent's composition: the three existing calls with the model's lists -> the constraint call's raw arrays"""
    t.add_measured_observations([g for g, _, _ in track], [kf] * len(track), [c for _, c, _ in track], [l for _, _, l in track])
    t.add_edges([(o, kf) for o, _ in edges], [s for _, s in edges], edge_type)
    t.compute_constraints([dict(kf1=o if other_first else kf, kf2=kf if other_first else o, store=True, overrides=[(kf, T_new)], cached=cached) for o, _ in edges])
    return t.raw["results"].tobytes(), t.raw["missing"].tobytes()


def _model_records(results, cap=16):
    rec = b"".join(CM.result_record(o).tobytes() for o in results)
    miss = np.full((len(results), cap), -1, np.int32)
    for i, o in enumerate(results):
        miss[i, :min(len(o["missing"]), cap)] = o["missing"][:cap]
    return rec, miss.tobytes()


def _commit_raw(reg, n_e):
    r = reg.commit_raw
    return r["results"][:n_e].tobytes(), r["missing"][:n_e].tobytes()


def _register_and_commit(reg, d, model, q, cached, index=0, batch=None, **kw):
    """one registration and its commit on d -> (the request the model builds, the registration as the model takes it, the commit's output)"""
    outs = reg.register_map_batch(d.map, batch or [q])
    req = model.request(q["mode"], q["root_kf"], q["T_root_from_world"], q["walk_kf"], q["direct_kf"])
    return req, _outputs(outs[index]), reg.commit(d.map, index, cached=cached, resolve_missing=False, **kw)


@pytest.fixture(scope="module")
def local_pair(env, registrar, scene):
    """case 1's maps: d took the commit, t the three existing calls; the model took the canonical commit"""
    model, d, t = env.model(), env.device(), env.device()
    q = MM.scene_request(scene, M.LOCAL)
    cached = _outside_poses(model)
    pose_before = d.get_poses([MM.ROOT_ID]).tobytes()
    req, out, got = _register_and_commit(registrar, d, model, q, cached)
    raw = dict(registrar.commit_raw)
    track, edges = RC.track_list(req, out), RC.edge_list(req, out)
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    before = model.content()
    added, pairs, results = RC.commit_local(model, MM.ROOT_ID, T_new, track, edges, cached=cached)
    twin_raw = _apply_on_twin(t, MM.ROOT_ID, T_new, track, edges, RC.METRIC, True, cached)
    return dict(model=model, d=d, t=t, q=q, req=req, out=out, got=got, raw=raw, track=track, edges=edges, T_new=T_new, added=added, pairs=pairs, results=results,
                twin_raw=twin_raw, cached=cached, pose_before=pose_before, content_before=before)


# ---- 1. a LOCAL commit against the twin map and the model ------------------------------------------------------------------------------------------------------------
def test_local_commit_equals_the_twin_map_and_the_model(local_pair):
    p = local_pair
    got, raw, n_e = p["got"], p["raw"], len(p["edges"])
    assert got["committed"] and got["status"] == 0 and got["mode"] == M.LOCAL and got["root_id"] == MM.ROOT_ID and got["other_id"] == -1
    assert n_e == 2 and [k for k, _ in p["edges"]] == [13, 19]
    assert got["T_new"].tobytes() == np.array(p["T_new"], np.float64).tobytes()
    assert got["track_point_ids"].tolist() == [g for g, _, _ in p["track"]] and got["track_added"].tolist() == p["added"]
    assert 0 < got["n_pairs_added"] == sum(p["added"]) < len(p["track"])                      # both sides of the "pair already present" rule
    assert raw["edge_kf"].tolist() == [13, 19] + [-1] * 6 and raw["edge_strength"][:2].tolist() == [s for _, s in p["edges"]] and not raw["edge_strength"][2:].any()
    assert got["edges"] == p["pairs"]
    assert (raw["results"][:n_e].tobytes(), raw["missing"][:n_e].tobytes()) == p["twin_raw"] == _model_records(p["results"])
    assert all(o["status"] == CM.OK for o in p["results"])
    assert _snapshot(p["d"], p["model"]) == _snapshot(p["t"], p["model"])
    d = p["d"]
    assert d.get_poses([MM.ROOT_ID]).tobytes() == p["pose_before"]                             # the override was for the computation only
    assert d.info() == p["model"].info() and d.edge_info() == (2, 2)
    ids, rec, n = d.get_feature_table(MM.ROOT_ID)
    want = sorted(g for g, k in p["model"].obs if k == MM.ROOT_ID)
    assert ids.tolist() == want and n == len(want)
    for g, r in zip(ids.tolist(), rec):                                                         # a pair that was present keeps what it had
        c, l = p["model"].meas[(g, MM.ROOT_ID)]
        assert r["obs"].tolist() == c and r["info"][0] == (1.0 / (1 << l)) ** 2
    e = d.get_edges(p["pairs"])
    for rec_, (k, _), o in zip(e, p["edges"], p["results"]):
        assert rec_.tobytes() == p["model"].edges.record(k, MM.ROOT_ID).tobytes()
        assert rec_["edge_type"] == RC.METRIC and rec_["is_marginalized"] == 1


# ---- 2. a LOOP commit ------------------------------------------------------------------------------------------------------------------------------------------------
def test_loop_commit_equals_the_twin_map_and_the_model(env, registrar, scene):
    model, d, t = env.model(), env.device(), env.device()
    q = MM.scene_request(scene, M.LOOP)
    cached = _outside_poses(model)
    req, out, got = _register_and_commit(registrar, d, model, q, cached)
    track = RC.track_list(req, out)
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    added, pairs, results = RC.commit_loop(model, MM.ALL_ID, MM.ROOT_ID, T_new, track, cached=cached)
    twin_raw = _apply_on_twin(t, MM.ROOT_ID, T_new, track, [(MM.ALL_ID, len(track))], RC.APPEARANCE, False, cached)
    assert got["committed"] and got["mode"] == M.LOOP and (got["root_id"], got["other_id"]) == (MM.ROOT_ID, MM.ALL_ID)
    assert len(track) == int(out["accepted"].sum()) >= COVIS and got["edge_strength"] == [len(track)] and got["edges"] == [(MM.ROOT_ID, MM.ALL_ID)]
    assert got["track_point_ids"].tolist() == [g for g, _, _ in track] and got["track_added"].tolist() == added and 0 < sum(added) < len(track)
    assert got["T_new"].tobytes() == np.array(T_new, np.float64).tobytes()
    assert _commit_raw(registrar, 1) == twin_raw == _model_records(results) and results[0]["status"] == CM.OK
    assert _snapshot(d, model) == _snapshot(t, model)
    e = d.get_edges([(MM.ALL_ID, MM.ROOT_ID)])[0]
    assert e.tobytes() == model.edges.record(MM.ALL_ID, MM.ROOT_ID).tobytes() and e["edge_type"] == RC.APPEARANCE and e["strength"] == len(track)


# ---- 3. the variant map: accepted points no qualifying keyframe observes; an anchor nobody gave a pose for ------------------------------------------------------------
def test_points_without_a_qualifying_observer_stay_out_and_a_missing_anchor_is_resolved(env, registrar, scene, local_pair):
    chosen = set(local_pair["got"]["track_point_ids"][5:105:5].tolist())     # 20 points the plain scene accepts
    assert len(chosen) == 20

    def variant(target):
        """their only observers: the keyframe outside the window (in the walk) and ALL_ID; an edge from that keyframe into the window, for computeAbsolutePose"""
        class V:
            def __getattr__(self, name):
                return getattr(target, name)

            def add_observations(self, point_ids, kf_ids):
                keep = [(int(p), int(k)) for p, k in zip(point_ids, kf_ids) if int(p) not in chosen or int(k) == MM.ALL_ID]
                keep += [(p, OUTSIDE_ID) for p in sorted(chosen) if any(int(q) == p for q in point_ids)]
                target.add_observations([p for p, _ in keep], [k for _, k in keep])
        return V()

    model, d = env.model(through=variant), env.device(through=variant)
    for m in (model, d):
        (m.add_edge(19, OUTSIDE_ID, 20, RC.LOCAL_EDGE) if m is model else m.add_edges([(19, OUTSIDE_ID)], [20], RC.LOCAL_EDGE))
    assert all({k for g, k in model.obs if g == p} == {OUTSIDE_ID, MM.ALL_ID} for p in chosen)
    q = MM.scene_request(scene, M.LOCAL)
    outs = registrar.register_map_batch(d.map, [q])
    req, out = model.request(q["mode"], q["root_kf"], q["T_root_from_world"], q["walk_kf"], q["direct_kf"]), _outputs(outs[0])
    track, edges = RC.track_list(req, out), RC.edge_list(req, out)
    accepted_ids = {int(req["point_ids"][int(out["cand_src"][i])]) for i in np.nonzero(out["accepted"])[0]}
    assert chosen <= accepted_ids and not chosen & {g for g, _, _ in track} and edges      # the model: accepted, and in no qualifying row
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    got = registrar.commit(d.map, 0, resolve_missing=False)
    first = _commit_raw(registrar, len(edges))
    _, pairs, results = RC.commit_local(model, MM.ROOT_ID, T_new, track, edges)
    assert got["track_point_ids"].tolist() == [g for g, _, _ in track] and first == _model_records(results)
    assert not chosen & set(d.get_feature_table(MM.ROOT_ID)[0].tolist())
    missing = [i for i, o in enumerate(results) if o["status"] == CM.MISSING_ANCHOR]
    assert missing and got["missing"] == [OUTSIDE_ID]
    for i in missing:
        e = d.get_edges([pairs[i]])[0]
        assert not e["is_marginalized"] and not e["T_lo_from_hi"].any() and not e["info"].any()
    # resolve_missing on a second map: absolute_poses, then a storing compute_constraints with the same override
    d2 = env.device(through=variant)
    d2.add_edges([(19, OUTSIDE_ID)], [20], RC.LOCAL_EDGE)
    registrar.register_map_batch(d2.map, [q])
    done = registrar.commit(d2.map, 0, resolve_missing=True)
    pose = {k: [float(v) for v in model.kf[k]["T"]] for k in model.kf}
    status, path, T_out = WM.absolute_pose(WM.adjacency(model.edges), model.window(), model.edges, pose, OUTSIDE_ID)
    assert status == WM.WALK_OK and path == [OUTSIDE_ID, 19]
    for (k, r), o in zip(pairs, results):
        if o["status"] == CM.MISSING_ANCHOR:
            o2 = model.constraint(k, r, overrides=[(r, T_new)], cached={OUTSIDE_ID: T_out})
            model.set_constraint(k, r, o2)
    assert done["missing"] == [] and all(o["status"] == CM.OK for o in done["edge_results"])
    for k, r in pairs:
        assert d2.get_edges([(k, r)])[0].tobytes() == model.edges.record(k, r).tobytes()


# ---- 4. the explicit calls against the twin ----------------------------------------------------------------------------------------------------------------------------
def test_explicit_calls_give_the_bytes_of_the_commit(env, registrar, scene, local_pair):
    p = local_pair
    e = env.device()
    dup = [p["track"][3], p["track"][0]]                                                        # repeated ids: taken once, the first feature wins
    dup[0] = (dup[0][0], [1.0, 2.0, 3.0], 2)
    track = p["track"][:10] + [(1999, [5.0, 6.0, 7.0], 1)] + p["track"][10:] + dup             # 1999 is no point of the map: skipped
    n2s = {19: p["edges"][1][1], OUTSIDE_ID: COVIS - 1, 13: p["edges"][0][1]}                   # any order; one neighbour below the threshold: no edge
    got = e.register_keyframes(MM.ROOT_ID, p["T_new"], n2s, RC.track_records(track), COVIS, cached=p["cached"], resolve_missing=False)
    assert got["edges"] == p["pairs"] and got["edge_strength"] == [s for _, s in p["edges"]]
    want_added = p["added"][:10] + [False] + p["added"][10:] + [False, False]
    assert got["track_added"].tolist() == want_added and got["n_pairs_added"] == sum(p["added"])
    assert (e.raw["results"][:2].tobytes(), e.raw["missing"][:2].tobytes()) == p["twin_raw"]
    assert e.raw["edge_kf"].tolist() == [13, 19, -1]
    assert _snapshot(e, p["model"]) == _snapshot(p["t"], p["model"])
    # addLoopClosure with the caller's list, against a commit of the loop request
    model, a, b = env.model(), env.device(), env.device()
    q = MM.scene_request(scene, M.LOOP)
    cached = _outside_poses(model)
    req, out, got = _register_and_commit(registrar, a, model, q, cached)
    first = _commit_raw(registrar, 1)
    track = RC.track_list(req, out)
    exp = b.add_loop_closure(MM.ALL_ID, MM.ROOT_ID, got["T_new"], RC.track_records(track), cached=cached, resolve_missing=False)
    assert (b.raw["results"].tobytes(), b.raw["missing"].tobytes()) == first and exp["track_added"].tolist() == got["track_added"].tolist()
    assert exp["edges"] == got["edges"] and exp["edge_strength"] == [len(track)]
    RC.commit_loop(model, MM.ALL_ID, MM.ROOT_ID, got["T_new"], track, cached=cached)
    assert _snapshot(a, model) == _snapshot(b, model)


# ---- 5. what follows sees the commit --------------------------------------------------------------------------------------------------------------------------------------
def test_a_following_registration_and_walk_see_the_new_pairs_and_edges(env, registrar, scene, local_pair):
    p = local_pair
    fresh = env.device()
    q2 = dict(mode=M.LOOP, root_kf=MM.ROOT2_ID, T_root_from_world=scene["T_root"], walk_kf=[MM.ROOT_ID], direct_kf=[])      # the first root as the query keyframe: its feature_table is the source list

    def after(m):
        registrar.register_map_batch(m.map, [q2], want_pass1=True)
        raw = registrar.raw
        walk = m.frames_in_neighborhood([MM.ROOT_ID, 13], 8)
        return ([raw[k].tobytes() if hasattr(raw[k], "tobytes") else raw[k] for k in ("results", "cand_src", "matches", "accepted", "kf_stats", "point_ids", "kf_ids")],
                [w.tolist() for w in walk])

    on_d, on_t, on_fresh = after(p["d"]), after(p["t"]), after(fresh)
    assert on_d == on_t
    assert on_d[1][0] == WM.frames_in_neighborhood(WM.adjacency(p["model"].edges), p["model"].window(), MM.ROOT_ID, 8) and len(on_d[1][0]) == 3
    assert on_fresh[1][0] == [MM.ROOT_ID] and on_fresh[0] != on_d[0]


# ---- 6. requests that commit nothing; refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw_commit(reg, dmap, index, cached_ids=(), track_cap=None, want_ids=True):
    """svs_reg_commit as the library takes it, so that a test can hand it what the binding would put right"""
    from scavislam_amd.ctypes_types import MAP_CONSTRAINT_RESULT_DTYPE, RegCommitResult
    ids = np.array(cached_ids, np.int32)
    T = np.tile(np.array(M.I12, np.float64), (max(len(ids), 1), 1))
    res = RegCommitResult()
    cons, miss = np.zeros(reg.max_keyframes, MAP_CONSTRAINT_RESULT_DTYPE), np.zeros((reg.max_keyframes, 4), np.int32)
    cap = reg.max_points if track_cap is None else track_cap
    tid = np.zeros(max(cap, 1), np.int32)
    return reg.ctx.lib.svs_reg_commit(reg.h, dmap.map.h, index, len(ids), ids.ctypes.data if len(ids) else None, T.ctypes.data if len(ids) else None, 4, C.byref(res), None,
                                      None, cons.ctypes.data, miss.ctypes.data, cap, tid.ctypes.data if want_ids else None, None), res


def test_requests_that_are_not_ok_commit_nothing_and_refusals_leave_everything_as_it_was(env, registrar, scene, local_pair):
    from scavislam_amd.capi import SvsError
    from scavislam_amd.register import KeyframeRegistrar
    INVALID, CAPACITY = 1, 4
    p = local_pair
    model, d = env.model(), env.device()
    T, ids = scene["T_root"], MM.scene_ids(scene)
    q = MM.scene_request(scene, M.LOCAL)
    batch = [dict(mode=M.LOOP, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[EXIT3_ID], direct_kf=[]),               # exit 3
             dict(mode=M.LOCAL, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[MM.ALL_ID], direct_kf=ids[1:]), q]     # exit 4; the scene's own
    before = _snapshot(d, model)
    outs = registrar.register_map_batch(d.map, batch)
    assert [o.status for o in outs] == [3, 4, 0]
    for i in (0, 1, 0):
        got = registrar.commit(d.map, i)
        assert not got["committed"] and got["status"] == outs[i].status and got["n_track"] == 0 and got["edges"] == [] and len(got["track_point_ids"]) == 0
        assert not registrar.commit_raw["results"].view(np.uint8).any() and (registrar.commit_raw["track_point_ids"] == -1).all()
    assert _snapshot(d, model) == before
    # refusals on this batch: each leaves the map and the registrar's batch as they were
    other = env.device()
    with_edge = env.device()
    with_edge.add_edges([(MM.ROOT_ID, 19)], [30], RC.LOCAL_EDGE)
    n_obs = d.info()[2]
    tight = env.device(max_keyframes=MAP_CAPS["max_keyframes"], max_points=MAP_CAPS["max_points"], max_observations=n_obs + len(p["track"]) - 1)
    one_edge = env.device(edges=1)
    no_edges = env.device(edges=0)
    assert _raw_commit(registrar, other, 2)[0] == INVALID                                     # a map the batch did not run on
    assert _raw_commit(registrar, d, 3)[0] == INVALID and _raw_commit(registrar, d, -1)[0] == INVALID      # outside the batch
    assert _raw_commit(registrar, d, 2, cached_ids=[30, 30])[0] == INVALID and _raw_commit(registrar, d, 2, cached_ids=[31, 30])[0] == INVALID
    assert _raw_commit(registrar, d, 2, track_cap=len(p["track"]) - 1)[0] == CAPACITY
    assert _snapshot(d, model) == before and _snapshot(other, model) == before
    for m, code in ((with_edge, INVALID), (tight, CAPACITY), (one_edge, CAPACITY), (no_edges, CAPACITY)):
        kept = _snapshot(m, model)
        registrar.register_map_batch(m.map, batch[2:])
        assert _raw_commit(registrar, m, 0)[0] == code
        assert _snapshot(m, model) == kept
    registrar.register_map_batch(tight.map, batch[2:])
    rc, res = _raw_commit(registrar, tight, 0, want_ids=False, track_cap=0)                   # still refused for the room, not for the caller's array
    assert rc == CAPACITY
    # a stateless registration ends the batch
    from test_gpu_register_map import _stateless
    registrar.register_map_batch(d.map, batch)
    _stateless(registrar, env.dev, model, scene, [q])
    assert _raw_commit(registrar, d, 2)[0] == INVALID
    # the refused request still commits, to the bytes of case 1; then it is spent
    registrar.register_map_batch(d.map, batch)
    got = registrar.commit(d.map, 2, cached=p["cached"], resolve_missing=False)
    assert got["committed"] and _commit_raw(registrar, 2) == p["twin_raw"]
    assert _snapshot(d, p["model"]) == _snapshot(p["t"], p["model"])
    after = _snapshot(d, p["model"])
    with pytest.raises(SvsError, match="status 1"):
        registrar.commit(d.map, 2)                                                            # already committed
    assert _snapshot(d, p["model"]) == after
    # a registrar that has not registered anything
    idle = KeyframeRegistrar(env.ctx, CAM, max_requests=1, max_points=64, max_keyframes=4, max_observers=64)
    try:
        assert _raw_commit(idle, d, 0)[0] == INVALID
    finally:
        idle.close()
    # the explicit forms
    tr = RC.track_records(p["track"][:3])
    bad_level = tr.copy(); bad_level["level"][1] = 3
    for call in (lambda: other.register_keyframes(9, p["T_new"], {13: 20}, tr, COVIS),                              # unknown root
                 lambda: other.register_keyframes(MM.ROOT_ID, p["T_new"], {9: 20}, tr, COVIS),                      # unknown neighbour
                 lambda: other.register_keyframes(MM.ROOT_ID, p["T_new"], {MM.ROOT_ID: 20}, tr, COVIS),             # the root its own neighbour
                 lambda: other.register_keyframes(MM.ROOT_ID, p["T_new"], {13: 20}, bad_level, COVIS),
                 lambda: other.add_loop_closure(MM.ROOT_ID, MM.ROOT_ID, p["T_new"], tr),                            # root == loop
                 lambda: other.add_loop_closure(9, MM.ROOT_ID, p["T_new"], tr),
                 lambda: with_edge.add_loop_closure(19, MM.ROOT_ID, p["T_new"], tr)):                               # an edge already present
        with pytest.raises(SvsError, match="status 1"):
            call()
    assert _snapshot(other, model) == before


# ---- 7. batch invariance ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_commit_does_not_depend_on_the_batch_or_the_run(env, registrar, scene, local_pair):
    from test_gpu_register_map import _batch_of_8
    p = local_pair
    first = _batch_of_8(scene)                                                                # the scene's LOCAL request at index 0
    second = first[1:6] + [first[0]] + first[6:]                                              # and at index 5
    got = []
    for batch, index in ((first, 0), (second, 5), (first, 0)):
        d = env.device()
        registrar.register_map_batch(d.map, batch)
        out = registrar.commit(d.map, index, cached=p["cached"], resolve_missing=False)
        raw = registrar.commit_raw
        got.append((out["track_point_ids"].tobytes(), out["track_added"].tobytes(), out["T_new"].tobytes(), raw["edge_kf"].tobytes(), raw["edge_strength"].tobytes(),
                    raw["results"].tobytes(), raw["missing"].tobytes(), _snapshot(d, p["model"])))
    assert got[0] == got[1] == got[2]
    assert got[0][5][:2 * 416] == p["twin_raw"][0] and got[0][7] == _snapshot(p["t"], p["model"])
    # several requests of one batch, one after the other, each with what the registration computed
    d = env.device()
    outs = registrar.register_map_batch(d.map, first)
    a = registrar.commit(d.map, 0, cached=p["cached"], resolve_missing=False)
    b = registrar.commit(d.map, 6, cached=p["cached"], resolve_missing=False)
    assert a["committed"] and b["committed"] and b["root_id"] == MM.ROOT2_ID and b["n_pairs_added"] == b["n_track"] > 0
    assert d.edge_info()[0] == len(a["edges"]) + len(b["edges"])


# ---- 8. resources ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_create_commit_destroy_returns_every_counter(gpu_ctx, device_scene, scene, few_ids, exit3_ids):
    from scavislam_amd.register import KeyframeRegistrar
    ctx = gpu_ctx[0]
    names = ("live_device_bytes", "live_pinned_bytes", "live_sync_objects")
    before = [ctx.get_stat(n) for n in names]
    e = Env(ctx, device_scene, scene, few_ids, exit3_ids)
    reg = KeyframeRegistrar(ctx, CAM, max_requests=8, max_points=512, max_keyframes=8, max_observers=4096)
    d = e.device()
    reg.register_map_batch(d.map, [MM.scene_request(scene, M.LOCAL)])
    held = [ctx.get_stat(n) for n in names]
    got = reg.commit(d.map, 0)
    assert got["committed"] and got["missing"] == [OUTSIDE_ID]                                # no edge leads to that anchor: it stays missing, as the reference would assert
    d.register_keyframes(MM.ROOT2_ID, M.I12, {13: 20}, RC.track_records([(1000, [1.0, 2.0, 3.0], 0)]), COVIS)
    e.close()
    reg.close()
    assert held[0] > before[0] and held[1] > before[1]
    assert [ctx.get_stat(n) for n in names] == before


# ---- 9. the C++ adaptor ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_adaptor_registers_and_commits_as_the_c_calls_do(gpu_ctx, tmp_path):
    """tests/cpp/regcommit_smoke.cpp: BackendRegistration::localRegisterFrame(map, root) / globalLoopClosure(map, ..) and BackendMap::registerKeyframes of
    include/scavislam_hip.hpp against svs_reg_register_map_batch + svs_reg_commit called directly on a twin map"""
    exe = tmp_path / "regcommit_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "regcommit_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("REGCOMMIT ")]
    assert tok and tok[0].split()[1] == "ok", out
    n_track, n_added, n_edges, loop_strength = (int(v) for v in tok[0].split()[2:6])
    assert n_track >= 15 and 0 < n_added < n_track and n_edges == 1 and loop_strength >= 15
