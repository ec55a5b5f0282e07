"""CPU tests of the device-resident map's yardstick (tests/register_map_model.py) and of the boundary of svs_map_* / svs_reg_register_map_batch: the model's
three rules are held against a literal restatement of backend.cpp:480-545 and :853-893 with Python sets, under shuffled hash orders, on the scene of
tests/register_model.make_scene(); the header, the ctypes layouts and the exports agree."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import register_map_model as MM
import register_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = M.SMALL_CAM
MAP_SYMBOLS = ["svs_map_create", "svs_map_destroy", "svs_map_add_keyframes", "svs_map_add_points", "svs_map_add_observations", "svs_map_set_poses",
               "svs_map_set_points", "svs_map_set_window", "svs_map_info", "svs_reg_register_map_batch"]


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model(scene):
    m = MM.MapModel()
    few = scene["src"]["point_id"][:10]
    MM.fill(m, scene, cand_ids_few=few, attach=lambda e: dict(entry=e))
    return m


def _build(model, q):
    return model.request(q["mode"], q["root_kf"], q["T_root_from_world"], q["walk_kf"], q["direct_kf"])


def test_the_scene_has_work_for_every_rule(scene, model):
    """counted on the model alone, at the default seed: 450 source points of which 150 are anchored outside the window; 6 points seen by direct neighbours only"""
    q = MM.scene_request(scene, M.LOCAL)
    walk, direct = set(q["walk_kf"]), set(q["direct_kf"])
    marking = walk - direct
    per_point = {}
    for p, k in model.obs:
        per_point.setdefault(p, set()).add(k)
    seen_twice = [p for p, ks in per_point.items() if len(ks & marking) >= 2]
    direct_only = [p for p, ks in per_point.items() if ks & walk and not ks & marking]
    req = _build(model, q)
    outside = [p for p in req["point_ids"] if not model.kf[int(model.pt[int(p)]["kf_index"])]["window"]]
    keep, _ = M.cull(req, CAM)
    print("source", len(req["src"]), "seen twice", len(seen_twice), "direct only", len(direct_only), "anchor outside", len(outside), "survivors", len(keep))
    assert len(seen_twice) >= 1 and len(direct_only) >= 1 and len(outside) >= 1 and len(keep) >= 50
    assert (len(req["src"]), len(direct_only), len(outside)) == (450, 6, 150)
    assert not set(direct_only) & set(int(p) for p in req["point_ids"])
    assert not set(outside) & set(int(p) for p in req["point_ids"][keep])


def test_the_request_built_for_the_scenes_neighbourhood_is_the_scene(scene, model):
    """ids ascend with the scene's table entries and its points with their ids: rules 1-3 must give back the request svs_reg_register_batch is tested with"""
    req = _build(model, MM.scene_request(scene, M.LOCAL))
    assert list(req["kf_ids"]) == MM.scene_ids(scene) and req["root_kf"] == scene["root_kf"] == 0
    assert np.array_equal(req["kf_T"], scene["kf_T"]) and np.array_equal(req["flags"], scene["flags"])
    assert req["src"].tobytes() == np.ascontiguousarray(scene["src"]).tobytes()
    assert np.array_equal(req["obs_begin"], scene["obs_begin"]) and np.array_equal(req["obs_kf"], scene["obs_kf"])


@pytest.mark.parametrize("seed", [None, 0, 1, 2])
def test_local_walk_equals_the_literal_restatement_in_any_hash_order(scene, model, seed):
    rng = None if seed is None else np.random.default_rng(seed)
    for root in (MM.ROOT_ID, MM.ROOT2_ID):
        q = MM.scene_request(scene, M.LOCAL, root)
        req = _build(model, q)
        point_set, cand, vertex_table = MM.literal_local(model, CAM, root, q["T_root_from_world"], set(q["walk_kf"]), set(q["direct_kf"]) | {root}, rng)
        assert point_set == set(int(p) for p in req["point_ids"]) and len(req["point_ids"]) == len(point_set)      # each once
        assert list(req["point_ids"]) == sorted(point_set)
        keep, in_vt = M.cull(req, CAM)
        assert set(cand) == set(int(p) for p in req["point_ids"][keep]) and len(cand) == len(keep) >= 50
        assert vertex_table == set(int(k) for k in req["kf_ids"][np.nonzero(in_vt)[0]])
        assert vertex_table <= set(int(k) for k in req["kf_ids"])      # every keyframe the reference's vertex table can hold has an entry
        # the observer rows: exactly the observers that have an entry
        for i, p in enumerate(req["point_ids"]):
            row = req["obs_kf"][req["obs_begin"][i]:req["obs_begin"][i + 1]]
            assert list(row) == sorted(row) and len(set(row)) == len(row)
            assert set(int(req["kf_ids"][e]) for e in row) == {k for pp, k in model.obs if pp == p} & set(int(k) for k in req["kf_ids"])


@pytest.mark.parametrize("seed", [None, 3])
def test_loop_walk_equals_the_literal_restatement(scene, model, seed):
    rng = None if seed is None else np.random.default_rng(seed)
    for query in (MM.ALL_ID, MM.FEW_ID, MM.OFFWALK_ID):
        q = dict(MM.scene_request(scene, M.LOOP), walk_kf=[query, MM.scene_ids(scene)[2]])      # only walk[0] is the query
        req = _build(model, q)
        table, cand, vertex_table = MM.literal_loop(model, CAM, MM.ROOT_ID, q["T_root_from_world"], query, rng)
        assert table == set(int(p) for p in req["point_ids"]) and list(req["point_ids"]) == sorted(table)
        keep, in_vt = M.cull(req, CAM)
        assert set(cand) == set(int(p) for p in req["point_ids"][keep])
        assert vertex_table == set(int(k) for k in req["kf_ids"][np.nonzero(in_vt)[0]])
        assert req["kf_ids"][0] == MM.ROOT_ID and list(req["kf_ids"][1:]) == sorted(req["kf_ids"][1:]) and query in req["kf_ids"]


def test_model_refuses_what_the_library_refuses(scene, model):
    before = model.info()
    pt = np.array(scene["src"][:1])
    pt["kf_index"] = 9999
    with pytest.raises(ValueError):
        model.add_keyframes([MM.ROOT_ID], [M.I12])
    with pytest.raises(ValueError):
        model.add_points([2000], pt)                      # the anchor is no keyframe of the map
    with pytest.raises(ValueError):
        model.add_observations([1000, 999], [MM.ROOT_ID, MM.ROOT_ID])
    with pytest.raises(ValueError):
        model.set_window([MM.ROOT_ID, 9999])
    assert model.info() == before
    n = len(model.obs)
    model.add_observations([1000], [MM.ALL_ID])           # present: ignored
    assert len(model.obs) == n


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree(tmp_path):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import REG_OVER_CAPACITY, RegMapRequest
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    lib = capi.load()
    for n in MAP_SYMBOLS:
        assert n in capi.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu %zu %zu %d\\n",'
                   "sizeof(svs_reg_map_request),offsetof(svs_reg_map_request,T_root_from_world),offsetof(svs_reg_map_request,h_walk_kf),"
                   "offsetof(svs_reg_map_request,h_direct_kf),SVS_REG_OVER_CAPACITY);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(RegMapRequest), RegMapRequest.T_root_from_world.offset, RegMapRequest.h_walk_kf.offset, RegMapRequest.h_direct_kf.offset,
                   REG_OVER_CAPACITY]
