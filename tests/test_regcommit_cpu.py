"""CPU tests of tests/regcommit_model.py: the canonical statement of include/scavislam_hip.h (svs_reg_commit, svs_map_register_keyframes, svs_map_add_loop_closure)
against the literal restatement of backend.cpp:615-722, :904-971 and slam_graph.cpp:188-251, :400-465 under shuffled hash orders; and that the scene of
tests/test_gpu_regcommit.py exercises both sides of the "pair already present" rule."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import register_map_model as MM
import register_model as M
import regcommit_model as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = M.SMALL_CAM
COVIS = M.PARAMS["covis_thr"]
NEW_EXPORTS = ["svs_reg_commit", "svs_map_register_keyframes", "svs_map_add_loop_closure"]


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model(scene):
    m = RC.CommitModel()
    MM.fill(RC.measured(m), scene, attach=lambda e: dict(entry=e))
    return m


@pytest.fixture(scope="module")
def local_run(scene, model):
    return RC.registration_of(model, scene, CAM, MM.scene_request(scene, M.LOCAL))


@pytest.fixture(scope="module")
def loop_run(scene, model):
    return RC.registration_of(model, scene, CAM, MM.scene_request(scene, M.LOOP))


def _fork(model):
    m = RC.CommitModel()
    m.kf = {k: dict(v, T=np.array(v["T"])) for k, v in model.kf.items()}
    m.pt = {k: np.array(v) for k, v in model.pt.items()}
    m.obs, m.meas, m.log = set(model.obs), dict(model.meas), list(model.log)
    m.edges.e = copy.deepcopy(model.edges.e)
    m.edge_log = list(model.edge_log)
    return m


def test_the_scene_exercises_both_sides_of_the_pair_rule(scene, model, local_run, loop_run):
    """LOCAL: status 0, the keyframes 13 and 19 qualify, 244 accepted candidates of which 136 already have the pair (point, root) and 108 do not; LOOP (query ALL_ID):
    status 0 and, on this model, the same 244 / 136 (both requests cull the same candidates).  The figures are printed; what is asserted is that both counts are non-zero"""
    req, out = local_run
    assert out["status"] == M.OK
    assert sorted(int(req["kf_ids"][k]) for k in np.nonzero(out["kf_stats"][:, 5])[0]) == [13, 19]
    track = RC.track_list(req, out)
    present = sum((g, MM.ROOT_ID) in model.obs for g, _, _ in track)
    print("LOCAL accepted", int(out["accepted"].sum()), "track", len(track), "present", present, "new", len(track) - present)
    assert len(track) == int(out["accepted"].sum())               # in this scene every accepted point is observed by a qualifying keyframe
    assert present > 0 and len(track) - present > 0
    req, out = loop_run
    assert out["status"] == M.OK
    track = RC.track_list(req, out)
    present = sum((g, MM.ROOT_ID) in model.obs for g, _, _ in track)
    print("LOOP accepted", len(track), "present", present)
    assert len(track) == int(out["accepted"].sum()) and present > 0 and len(track) - present > 0


@pytest.mark.parametrize("seed", range(20))
def test_canonical_local_commit_equals_the_literal_restatement_in_any_hash_order(scene, model, local_run, seed):
    req, out = local_run
    q = MM.scene_request(scene, M.LOCAL)
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    a, b = _fork(model), _fork(model)
    cached = {k: a.kf[k]["T"] for k in a.kf if not a.kf[k]["window"]}      # every anchor's pose is given: the constraints are compared to the last bit
    added, pairs, results = RC.commit_local(a, MM.ROOT_ID, T_new, RC.track_list(req, out), RC.edge_list(req, out), cached=cached)
    rng = np.random.default_rng(seed)
    n2s, tpl = RC.keyframes_to_register(b, CAM, req, out, set(q["direct_kf"]) | {MM.ROOT_ID}, COVIS, rng)
    assert sorted(n2s) == RC.edge_list(req, out)
    assert len(tpl) >= len(added) and {g for g, _, _ in tpl} == {g for g, _, _ in RC.track_list(req, out)}
    RC.register_keyframes(b, MM.ROOT_ID, T_new, n2s, tpl, COVIS, cached=cached)
    assert a.content() == b.content()
    assert all(o["status"] == 0 and o["strength"] >= COVIS for o in results) and len(pairs) == 2
    assert a.content() != model.content() and np.array_equal(a.kf[MM.ROOT_ID]["T"], model.kf[MM.ROOT_ID]["T"])


@pytest.mark.parametrize("seed", range(20))
def test_canonical_loop_commit_equals_the_literal_restatement(scene, model, loop_run, seed):
    req, out = loop_run
    q = MM.scene_request(scene, M.LOOP)
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    a, b = _fork(model), _fork(model)
    cached = {k: a.kf[k]["T"] for k in a.kf if not a.kf[k]["window"]}
    track = RC.track_list(req, out)
    added, pairs, results = RC.commit_loop(a, MM.ALL_ID, MM.ROOT_ID, T_new, track, cached=cached)
    rng = np.random.default_rng(seed)
    tpl = RC.loop_track_list(req, out)
    assert tpl == track
    # the feature tables and point tables of the reference are hash containers, but addLoopClosure iterates none of them: the shuffle moves the map's own tables
    b.obs = set(RC._order(sorted(b.obs), rng))
    RC.add_loop_closure(b, MM.ALL_ID, MM.ROOT_ID, T_new, tpl, cached=cached)
    assert a.content() == b.content()
    e = a.edges.e[(MM.ROOT_ID, MM.ALL_ID)]
    assert (e["strength"], e["edge_type"], e["is_marginalized"]) == (len(track), RC.APPEARANCE, 1) and results[0]["status"] == 0


def test_explicit_and_device_list_formulations_agree(scene, model, local_run):
    """the explicit call takes the reference's list (a point once per qualifying observer, in any order of the keyframes) and every neighbour with its strength;
    the commit takes the canonical list: the same map"""
    req, out = local_run
    q = MM.scene_request(scene, M.LOCAL)
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    a, b = _fork(model), _fork(model)
    RC.commit_local(a, MM.ROOT_ID, T_new, RC.track_list(req, out), RC.edge_list(req, out))
    n2s, tpl = RC.keyframes_to_register(b, CAM, req, out, set(q["direct_kf"]) | {MM.ROOT_ID}, COVIS, np.random.default_rng(3))
    below = [(int(req["kf_ids"][-1]), COVIS - 1)]                   # a neighbour below the threshold gets no edge
    added, pairs, _ = RC.commit_local(b, MM.ROOT_ID, T_new, tpl + [(99999, [1.0, 2.0, 3.0], 0)], n2s + below, covis_thr=COVIS)
    assert a.content() == b.content() and sum(added) == len(a.obs) - len(model.obs) and not added[-1]
    assert len(tpl) > len(RC.track_list(req, out))                 # the reference's list does repeat points


def test_a_missing_anchor_leaves_the_edge_zero_and_unmarginalised(scene, model, local_run):
    req, out = local_run
    q = MM.scene_request(scene, M.LOCAL)
    T_new = RC.pose_mul(out["T"], q["T_root_from_world"])
    a = _fork(model)
    _, pairs, results = RC.commit_local(a, MM.ROOT_ID, T_new, RC.track_list(req, out), RC.edge_list(req, out))
    miss = [o for o in results if o["status"] == 2]
    assert miss, "an anchor of the scene lies outside the window"
    for (k, r), o in zip(pairs, results):
        e = a.edges.e[(min(k, r), max(k, r))]
        assert e["is_marginalized"] == (o["status"] == 0) and (o["status"] == 0 or not np.asarray(e["info"]).any())


def test_header_binding_and_exports_agree():
    from scavislam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in capi.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr), name
    lib = os.path.join(ROOT, "scavislam_amd", "libscavislam_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in NEW_EXPORTS:
        assert re.search(r"\bT %s\b" % name, syms), name
    from scavislam_amd.ctypes_types import RegCommitResult
    import ctypes as C
    assert C.sizeof(RegCommitResult) == 128
