"""CPU tests of the yardstick of svs_frontend_set_neighborhood_from_root (tests/nbh_root_model.py): its rules are held against a literal restatement of
backend.cpp:244-309 / :347-386 and of the loop of stereo_frontend.cpp:1007-1029, with every hash container walked in 20 shuffled orders and equal-strength
multimap entries compared as sets per strength; the header, the ctypes layouts and the exports agree."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nbh_root_model as RM
import neighborhood_model as NM
import register_map_model as MM
import register_model as M
import walk_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model(scene):
    m = MM.MapModel()
    MM.fill(m, scene, cand_ids_few=scene["src"]["point_id"][:10], attach=lambda e: dict(entry=e))
    RM.extend(m)
    return m


@pytest.fixture(scope="module")
def table():
    return RM.edge_table()


def slots(missing=()):
    tab = [7, 13, 19, 25, 40, RM.HUB, RM.LONE, 52]
    return [(-1 if k in missing else k) for k in tab] + [-1] * (K - len(tab))


def _head(scene, sizes, first_id=3000):
    n = sum(sizes)
    head = np.array(scene["src"][100:100 + n])
    head["kf_index"] = np.arange(n) % 4
    head["point_id"] = first_id + np.arange(n)
    return head, [int(e) for e in np.cumsum(sizes)]


CASES = [(40, 10), (40, 0), (40, 1), (RM.HUB, 10), (RM.HUB, 0), (RM.HUB, 12), (RM.HUB, 13), (RM.LONE, 10), (13, 10), (41, 10), (52, 3)]


@pytest.mark.parametrize("root,max_nn", CASES)
def test_model_equals_the_literal_restatement_in_twenty_hash_orders(model, table, root, max_nn):
    adj, window, pose = RM.graph_of(model, table)
    builds = {}                                                 # by act: the model is no function of a hash order
    for seed in range(20):
        rng = np.random.default_rng(seed)
        point_list, vertex_map, found = RM.literal(model, table, root, max_nn, rng)
        for act in sorted(vertex_map) + [3]:
            if act not in builds:
                builds[act] = RM.build(model, table, dict(root_id=root, act_id=act, slot_kf=slots(), max_num_neighbors=max_nn))
            out = builds[act]
            assert not out["over_capacity"] and not out["root_outside_window"]
            vertex = [int(k) for k in out["vertex_ids"]]
            # rule 1: the multimap's order is a function of the insertion order, so the ids compare as a list
            assert vertex[0] == root and vertex[1:1 + len(found)] == found and out["n_root_neighbors"] == len(found) <= max_nn + 1
            assert all(k in window for k in found)
            # rule 2
            assert sorted(point_list) == [int(p) for p in out["point_ids"]] and len(set(point_list)) == len(point_list) == out["n_map_points"]
            assert set(vertex) == set(vertex_map) and len(vertex) == len(vertex_map) == out["n_vertex"]
            assert vertex[1 + len(found):] == sorted(vertex[1 + len(found):])
            # rule 3
            lost = 0
            for k, T in zip(vertex, out["vertex_T"]):
                want = vertex_map[k]["T_me_from_w"]
                if want is None:                                    # the reference asserts; here the stored pose, counted
                    lost += 1
                    want = pose[k]
                    assert k not in window
                assert np.array_equal(T, np.array(want)), k
            assert lost == out["n_no_path"]
            # rules 4 and 5
            if act in vertex_map:
                assert out["act_index"] == vertex.index(act)
                mine = [(int(out["strength"][out["act_index"], j]), vertex[j]) for j in out["act_neighbors"]]
                assert mine == sorted(mine) and RM.per_strength(mine) == RM.per_strength(vertex_map[act]["strength_to_neighbors"])
            else:
                assert out["act_index"] == -1 and out["n_act_neighbors"] == 0
            for i, a in enumerate(vertex):
                row = [(int(s), vertex[j]) for j, s in enumerate(out["strength"][i, :len(vertex)]) if s >= 0]
                assert RM.per_strength(row) == RM.per_strength(vertex_map[a]["strength_to_neighbors"]) and out["strength"][i, i] == -1
            assert (out["strength"][len(vertex):] == -1).all() and (out["strength"][:, len(vertex):] == -1).all()


@pytest.mark.parametrize("root,act", [(40, 40), (RM.HUB, 40), (RM.HUB, RM.HUB), (40, 3)])
def test_head_groups_follow_the_literal_loop(scene, model, table, root, act):
    """newpoint_map: the active keyframe's list (two fixed groups here) and lists keyed by 13, 19, 7 (no neighbour of 40), HUB, an empty one keyed by 41"""
    keys = [13, 7, 19, RM.HUB, 41]
    head, ge = _head(scene, [3, 2, 4, 5, 1, 6, 0])
    q = dict(root_id=root, act_id=act, slot_kf=slots(), head=head, head_group_end=ge, n_fixed_groups=2, head_group_kf=[-1, -1] + keys)
    out = RM.build(model, table, q)
    for seed in range(20):
        _, vertex_map, _ = RM.literal(model, table, root, 10, np.random.default_rng(seed))
        if act not in vertex_map:
            assert out["head_order"] == [0, 1] and out["n_head_dropped"] == 16 and out["act_index"] == -1
            continue
        stn = vertex_map[act]["strength_to_neighbors"]
        visited = RM.literal_group_order(stn, {k: None for k in keys + [act]}, act)
        assert visited[0] == act
        got = [keys[g - 2] for g in out["head_order"][2:]]
        strength_of = dict((k, s) for s, k in stn)
        assert RM.per_strength([(strength_of[k], k) for k in got]) == RM.per_strength([(strength_of[k], k) for k in visited[1:]])
        assert [strength_of[k] for k in got] == sorted(strength_of[k] for k in got)
    kept = [g for g in out["head_order"]]
    begin = lambda g: ge[g - 1] if g else 0
    assert out["records"][:out["n_new"]].tobytes() == b"".join(head[begin(g):ge[g]].tobytes() for g in kept)
    assert out["n_head_kept"] + out["n_head_dropped"] == len(head) and out["n_groups"] == len(kept) + 1 == len(out["group_end"])
    assert out["group_end"][-1] == out["n_points"] == out["n_new"] + out["n_map_points"]


def test_the_scene_has_work_for_every_rule(model, table):
    adj, window, pose = RM.graph_of(model, table)
    a = RM.build(model, table, dict(root_id=40, act_id=40, slot_kf=slots(missing=(25,))))
    print({f: a[f] for f in RM.FIELDS}, list(a["vertex_ids"]), list(a["act_neighbors"]))
    assert list(a["vertex_ids"]) == [40, 19, 13, RM.HUB, 7, 25]                 # the tie at strength 20 goes by slot; 7 and 25 are anchors outside the window
    assert [int(a["vertex_ids"][j]) for j in a["act_neighbors"]] == [13, 19, RM.HUB]      # and by id here
    assert a["n_no_path"] == 1 and a["n_no_slot"] > 0 and a["n_map_points"] > 300
    assert WM.absolute_pose(adj, window, table, pose, 7)[1] == [7, RM.N1, 13]   # a path of three: (7, N1) marginalised, (N1, 13) not
    assert table.e[(7, RM.N1)]["is_marginalized"] == 1 and table.e[(13, RM.N1)]["is_marginalized"] == 0
    assert not np.array_equal(a["vertex_T"][4], pose[7]) and np.array_equal(a["vertex_T"][5], pose[25])
    hub = RM.build(model, table, dict(root_id=RM.HUB, act_id=40, slot_kf=slots()))
    assert hub["n_root_neighbors"] == 11 and RM.build(model, table, dict(root_id=RM.HUB, act_id=40, slot_kf=slots(), max_num_neighbors=0))["n_root_neighbors"] == 1
    assert RM.build(model, table, dict(root_id=RM.HUB, act_id=40, slot_kf=slots(), max_num_neighbors=20))["n_root_neighbors"] == 13
    assert list(hub["vertex_ids"][1:5]) == [78, 77, 76, 52]                      # 77 before 76: the slot decides
    row = [u for u, _ in reversed(adj[RM.HUB])]
    assert row.index(50) < row.index(19) < row.index(RM.OUT_LEAF) < row.index(13)  # keyframes outside the window between those inside
    lone = RM.build(model, table, dict(root_id=RM.LONE, act_id=RM.LONE, slot_kf=slots()))
    assert list(lone["vertex_ids"]) == [RM.LONE, 7] and lone["n_act_neighbors"] == 0 and lone["act_index"] == 0 and lone["n_map_points"] == 6
    assert RM.result_fields(RM.build(model, table, dict(root_id=7, act_id=7, slot_kf=slots()))) == (0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0)


def test_capacity_is_all_or_nothing_in_the_model(scene, model, table):
    head, ge = _head(scene, [3, 4, 5])
    q = dict(root_id=40, act_id=40, slot_kf=slots(), head=head, head_group_end=ge, n_fixed_groups=1, head_group_kf=[-1, 13, 7])
    fit = RM.build(model, table, q)
    assert fit["n_head_kept"] == 7 and fit["n_head_dropped"] == 5 and fit["group_end"] == [3, 7, fit["n_points"]] and fit["n_groups"] == 3
    assert not RM.build(model, table, q, max_points=fit["n_points"], vertex_cap=fit["n_vertex"])["over_capacity"]
    d = RM.build(model, table, q, max_points=fit["n_points"] - 1)                # (d): the kept head does not fit, the fixed one does
    assert d["over_capacity"] and "records" not in d and all(d[f] == fit[f] for f in RM.FIELDS if f != "over_capacity")
    b = RM.build(model, table, q, max_points=fit["n_map_points"] + 2)            # (b): not even the fixed group
    assert RM.result_fields(b) == (3 + fit["n_map_points"], fit["n_map_points"], 0, 0, 1, 0, fit["n_root_neighbors"], 0, 0, 0, 0, 0, 0)
    c = RM.build(model, table, q, vertex_cap=fit["n_vertex"] - 1)                # (c)
    assert RM.result_fields(c) == (3 + fit["n_map_points"], fit["n_map_points"], fit["n_vertex"], fit["n_no_slot"], 1, 0, fit["n_root_neighbors"], 0, 0, 0, 0, 0, 0)
    a = RM.build(model, table, dict(q, root_id=RM.HUB), vertex_cap=11)           # (a): the root and eleven neighbours
    assert RM.result_fields(a) == (3, 0, 12, 0, 1, 0, 11, 0, 0, 0, 0, 0, 0)


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree(tmp_path):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import KF_MAX_VERTICES, NbrRequest, NbrResult
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    lib = capi.load()
    name = "svs_frontend_set_neighborhood_from_root"
    assert name in capi.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr)
    assert hasattr(lib, name)
    assert len(capi._SIGS[name]) == len(re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1).split(","))
    req_fields = [f for f, _ in NbrRequest._fields_]
    res_fields = [f for f, _ in NbrResult._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu %d'
                   + " %zu" * (len(req_fields) + len(res_fields)) + '\\n",sizeof(svs_nbr_request),sizeof(svs_nbr_result),SVS_KF_MAX_VERTICES'
                   + "".join(",offsetof(svs_nbr_request,%s)" % f for f in req_fields) + "".join(",offsetof(svs_nbr_result,%s)" % f for f in res_fields)
                   + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(NbrRequest), C.sizeof(NbrResult), KF_MAX_VERTICES] + [getattr(NbrRequest, f).offset for f in req_fields] + \
        [getattr(NbrResult, f).offset for f in res_fields]
