"""CPU tests of the neighbourhood list's yardstick (tests/neighborhood_model.py) and of the boundary of svs_frontend_set_candidates_from_map: the model's rules are
held against a literal restatement of backend.cpp:311-386 with Python sets, under shuffled hash orders, on the scene of tests/register_model.make_scene() as
register_map_model.fill() puts it into a map; the header, the ctypes layouts and the exports agree."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import neighborhood_model as NM
import register_map_model as MM
import register_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model(scene):
    m = MM.MapModel()
    MM.fill(m, scene, cand_ids_few=scene["src"]["point_id"][:10], attach=lambda e: dict(entry=e))
    return m


def _vertex_lists(scene):
    ids = MM.scene_ids(scene)
    return [[MM.ROOT_ID, ids[2]], [MM.ROOT_ID], ids, [MM.OFFWALK_ID], [MM.ROOT2_ID], [ids[3], MM.ALL_ID, MM.ROOT_ID]]


@pytest.mark.parametrize("seed", [None, 0, 1, 2])
def test_model_equals_the_literal_restatement_as_sets_in_any_hash_order(scene, model, seed):
    rng = None if seed is None else np.random.default_rng(seed)
    slots = NM.slot_table(scene)
    for vertex in _vertex_lists(scene):
        out = NM.build(model, vertex, slots)
        point_list, vertex_map = NM.literal(model, vertex, rng)
        n_map = out["n_map_points"]
        assert len(point_list) == n_map == len({ap["point_id"] for ap in point_list})      # each once
        assert list(out["point_ids"]) == sorted(ap["point_id"] for ap in point_list)         # the model's order is the ascending one
        by_id = {ap["point_id"]: ap for ap in point_list}
        for rec in out["records"]:
            ap = by_id[int(rec["point_id"])]
            assert np.array_equal(rec["xyz_anchor"], ap["xyz_anchor"]) and np.array_equal(rec["anchor_obs_pyr"], ap["anchor_obs_pyr"])
            assert int(rec["anchor_level"]) == ap["anchor_level"] and int(rec["pad_"]) == 0
            assert int(rec["kf_index"]) == (slots.index(ap["anchor_id"]) if ap["anchor_id"] in slots else -1)
        assert set(int(k) for k in out["vertex_ids"]) == set(vertex_map) and len(out["vertex_ids"]) == len(vertex_map) == out["n_vertex"]
        assert list(out["vertex_ids"][:len(vertex)]) == vertex and list(out["vertex_ids"][len(vertex):]) == sorted(out["vertex_ids"][len(vertex):])
        for k, T in zip(out["vertex_ids"], out["vertex_T"]):
            assert np.array_equal(T, vertex_map[int(k)])
        assert out["group_end"] == [0, n_map] and out["n_groups"] == 2 and out["n_new"] == 0


def test_the_scene_has_work_for_every_rule(scene, model):
    """counted on the model alone, at the default seed, for the vertex list [ROOT_ID, scene_ids[2]] and a slot table without the scene's last keyframe"""
    ids = MM.scene_ids(scene)
    vertex = [MM.ROOT_ID, ids[2]]
    out = NM.build(model, vertex, NM.slot_table(scene, missing=(ids[4],)))
    per_point = {}
    for p, k in model.obs:
        per_point.setdefault(p, set()).add(k)
    seen_twice = [p for p, ks in per_point.items() if len(ks & set(vertex)) >= 2]
    added = [int(k) for k in out["vertex_ids"][len(vertex):]]
    empty = NM.build(model, [MM.ROOT2_ID], NM.slot_table(scene))
    off = NM.build(model, [MM.OFFWALK_ID], NM.slot_table(scene))
    everything = NM.build(model, ids, NM.slot_table(scene))
    print("points", out["n_map_points"], "seen twice", len(seen_twice), "anchors added", added, "without a slot", out["n_no_slot"], "ROOT2", empty["n_map_points"],
          "OFFWALK", list(off["point_ids"]), "all keyframes", everything["n_map_points"], everything["n_vertex"])
    assert len(seen_twice) >= 1 and len(added) >= 1 and out["n_no_slot"] >= 1
    assert (out["n_map_points"], len(seen_twice), out["n_vertex"], out["n_no_slot"]) == (399, 182, 5, 124)
    assert added == [ids[1], ids[3], ids[4]]
    assert NM.result_fields(empty) == (0, 0, 1, 0, 0) and len(model.feature_table(MM.ROOT2_ID)) == 0
    assert list(off["point_ids"]) == list(range(600, 608)) and list(off["vertex_ids"]) == [MM.OFFWALK_ID] and off["n_no_slot"] == 8
    assert not set(range(600, 608)) & set(int(p) for p in everything["point_ids"])      # reachable only through OFFWALK_ID
    assert (everything["n_map_points"], everything["n_vertex"], everything["n_no_slot"]) == (456, 5, 0)


def test_capacity_is_all_or_nothing_in_the_model(scene, model):
    ids = MM.scene_ids(scene)
    head = np.array(scene["src"][:7])
    head["kf_index"] = 0
    fit = NM.build(model, [MM.ROOT_ID, ids[2]], NM.slot_table(scene), head=head, head_group_end=[3, 7])
    assert fit["group_end"] == [3, 7, fit["n_points"]] and fit["n_new"] == 7 and fit["n_groups"] == 3 and fit["n_points"] == 7 + fit["n_map_points"]
    assert fit["records"][:7].tobytes() == head.tobytes() and list(fit["point_ids"][:7]) == list(head["point_id"])
    over = NM.build(model, [MM.ROOT_ID, ids[2]], NM.slot_table(scene), head=head, head_group_end=[3, 7], max_points=fit["n_points"] - 1)
    assert NM.result_fields(over) == (fit["n_points"], fit["n_map_points"], 0, 0, 1) and "records" not in over
    narrow = NM.build(model, [MM.ROOT_ID, ids[2]], NM.slot_table(scene), vertex_cap=fit["n_vertex"] - 1)
    assert NM.result_fields(narrow) == (fit["n_map_points"], fit["n_map_points"], fit["n_vertex"], 0, 1)
    assert not NM.build(model, [MM.ROOT_ID, ids[2]], NM.slot_table(scene), head=head, head_group_end=[3, 7], max_points=fit["n_points"], vertex_cap=fit["n_vertex"])["over_capacity"]


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree(tmp_path):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import NbhRequest, NbhResult
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    lib = capi.load()
    name = "svs_frontend_set_candidates_from_map"
    assert name in capi.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr)
    assert hasattr(lib, name)
    req_fields = ["stream", "n_vertex", "n_head", "n_head_groups", "h_vertex_kf", "h_slot_kf", "h_head_group_end", "h_head"]
    res_fields = ["n_points", "n_map_points", "n_vertex", "n_no_slot", "over_capacity", "pad_"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu'
                   + " %zu" * (len(req_fields) + len(res_fields)) + '\\n",sizeof(svs_nbh_request),sizeof(svs_nbh_result)'
                   + "".join(",offsetof(svs_nbh_request,%s)" % f for f in req_fields) + "".join(",offsetof(svs_nbh_result,%s)" % f for f in res_fields)
                   + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(NbhRequest), C.sizeof(NbhResult)] + [getattr(NbhRequest, f).offset for f in req_fields] + [getattr(NbhResult, f).offset for f in res_fields]
