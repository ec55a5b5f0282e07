"""CPU tests of the yardstick of svs_map_compute_strength / svs_map_add_keyframe (tests/addkf_model.py): its closed form of computeStrength and its addKeyframe
are held to a literal restatement of slam_graph.cpp:143-186 and :358-552 -- dicts where the reference has unordered_maps, the zeroing loop where the reference
has it (inside the loop over the track points), every table walked in shuffled orders -- and the header, the ctypes layouts and the exports agree.  No oracle
library goes through addKeyframe, so this pin is a restatement, as the one of the walks is."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import addkf_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDKF_SYMBOLS = ["svs_map_compute_strength", "svs_map_add_keyframe", "svs_map_add_first_keyframe", "svs_map_get_points", "svs_map_get_feature_table"]


def _shuffled(items, rng):
    items = list(items)
    if rng is not None:
        rng.shuffle(items)
    return items


def literal_compute_strength(new_points, track_points, point_table, covis_thr, width, height, rng=None):
    """slam_graph.cpp:467-552, line by line"""
    strength, num_top, num_bottom, num_left, num_right = {}, {}, {}, {}, {}
    half_width, half_height = int(width * 0.5), int(height * 0.5)

    def add(table, key):
        table[key] = table.get(key, 0) + 1

    for np_ in new_points:
        add(strength, np_["anchor_id"])
    for tp in track_points:
        if tp["global_id"] not in point_table:
            continue
        vis_set = point_table[tp["global_id"]]
        for kf in _shuffled(vis_set, rng):
            add(strength, kf)
            u, v = tp["center"][0], tp["center"][1]
            if u < half_width:
                add(num_left, kf)
            else:
                add(num_right, kf)
            if v < half_height:
                add(num_top, kf)
            else:
                add(num_bottom, kf)
        for frame_id in _shuffled(strength, rng):
            if (frame_id in num_top and num_top[frame_id] >= covis_thr // 2 and frame_id in num_bottom and num_bottom[frame_id] >= covis_thr // 2
                    and frame_id in num_left and num_left[frame_id] >= covis_thr // 2 and frame_id in num_right and num_right[frame_id] >= covis_thr // 2):
                continue
            strength[frame_id] = 0
    return strength, (num_left, num_right, num_top, num_bottom)


def literal_add_keyframe(g, oldkey, newkey, T_rel, new_points, track_points, covis_thr, width, height, rng=None):
    """slam_graph.cpp:143-186 with :358-465 on a graph g = dict(vertex={id: dict(T, feature_table)}, point={id: dict(vis_set, ...)}, edges={(lo, hi): strength});
    -> neighborid_to_strength after the clamp, and the edges in the order they were made"""
    v_new = dict(T=AM.pose_mul(T_rel, g["vertex"][oldkey]["T"]), feature_table={})
    strength, _ = literal_compute_strength(new_points, track_points, {p: q["vis_set"] for p, q in g["point"].items()}, covis_thr, width, height, rng)
    assert oldkey in strength
    if strength[oldkey] < covis_thr:
        strength[oldkey] = covis_thr
    for np_ in new_points:                                         # addNewPointsToMap
        if strength[np_["anchor_id"]] < covis_thr:
            continue
        g["point"][np_["point_id"]] = dict(vis_set={newkey, np_["anchor_id"]}, xyz_anchor=np_["xyz_anchor"], anchor_id=np_["anchor_id"],
                                           anchor_obs_pyr=np_["anchor_obs_pyr"], anchor_level=np_["anchor_level"])
        feat_anchor = ([c * (2.0 ** np_["anchor_level"]) for c in np_["anchor_obs_pyr"]], np_["anchor_level"])
        v_new["feature_table"].setdefault(np_["point_id"], (list(np_["feat_center"]), np_["feat_level"]))
        g["vertex"][np_["anchor_id"]]["feature_table"].setdefault(np_["point_id"], feat_anchor)
    for tp in track_points:                                        # addNewObsToOldPoints
        if tp["global_id"] not in g["point"]:
            continue
        v_new["feature_table"].setdefault(tp["global_id"], (list(tp["center"]), tp["level"]))      # (insert: the first wins)
        g["point"][tp["global_id"]]["vis_set"].add(newkey)
    g["vertex"][newkey] = v_new
    made = []
    for other in _shuffled(strength, rng):                         # addNewEdges
        if strength[other] >= covis_thr:
            g["edges"][(min(other, newkey), max(other, newkey))] = strength[other]
            made.append(other)
    return strength, made


def _new_point(pid, anchor, rng):
    return dict(point_id=pid, anchor_id=anchor, xyz_anchor=rng.normal(size=3).tolist(), anchor_obs_pyr=rng.uniform(1, 300, 3).tolist(), anchor_level=int(rng.integers(3)),
                feat_center=rng.uniform(1, 600, 3).tolist(), feat_level=int(rng.integers(3)))


def _case(rng, thr, width=640, height=480, n_kf=6, n_pt=40, n_track=30, n_new=8, edge_values=True):
    """a random graph and a random keyframe to insert; centres are drawn from a few values around the two half sizes so that u == half_width happens"""
    hw, hh = int(width * 0.5), int(height * 0.5)
    kfs = [int(k) for k in rng.choice(2000, n_kf, replace=False)]
    g = dict(vertex={k: dict(T=AM.pose_mul(AM.I12, [1, 0, 0, float(k), 0, 1, 0, 0.5, 0, 0, 1, -0.25 * k]), feature_table={}) for k in kfs}, point={}, edges={})
    for p in range(n_pt):
        vis = set(int(k) for k in rng.choice(kfs, int(rng.integers(1, min(4, n_kf) + 1)), replace=False))
        g["point"][100 + 3 * p] = dict(vis_set=vis)
    us = [hw - 1.0, hw - 0.5, float(hw), hw + 0.25, 5.0, width - 3.0] if edge_values else [10.0, width - 10.0]
    vs = [hh - 1.0, float(hh), hh + 0.5, 7.0, height - 2.0] if edge_values else [10.0, height - 10.0]
    ids = list(g["point"]) + [9001, 9002]                          # two unknown ids
    track = [dict(global_id=int(rng.choice(ids)), center=[float(rng.choice(us)), float(rng.choice(vs)), 1.0], level=int(rng.integers(3))) for _ in range(n_track)]
    oldkey = kfs[0]
    new = [_new_point(5000 + i, int(rng.choice(kfs)), rng) for i in range(n_new)]
    if new:
        new[0]["anchor_id"] = oldkey                               # oldkey is a key (the reference asserts)
    else:
        track.append(dict(global_id=next(p for p, q in g["point"].items() if oldkey in q["vis_set"]), center=[1.0, 1.0, 0.0], level=0))
    return g, oldkey, new, track, (width, height)


def _model_graph(g):
    m = AM.Graph()
    m.pose = {k: list(v["T"]) for k, v in g["vertex"].items()}
    m.vis = {p: set(q["vis_set"]) for p, q in g["point"].items()}
    m.point = {p: dict(q) for p, q in g["point"].items()}
    return m


def _check(g, oldkey, new, track, size, thr, rng):
    width, height = size
    hw, hh = int(width * 0.5), int(height * 0.5)
    vis = {p: set(q["vis_set"]) for p, q in g["point"].items()}
    want, quad = literal_compute_strength(new, track, vis, thr, width, height, rng)
    keys, exists, m = AM.strength_closed_form([p["anchor_id"] for p in new], [(t["global_id"], t["center"][0], t["center"][1]) for t in track], vis, thr, hw, hh)
    assert [k[0] for k in keys] == sorted(want) and {k[0]: k[1] for k in keys} == want
    assert exists == [t["global_id"] in vis for t in track] and m == sum(exists)
    for k in keys:
        assert k[2:6] == [q.get(k[0], 0) for q in quad]
    # addKeyframe behind it
    model = _model_graph(g)
    out = model.add_keyframe(7777, oldkey, [1, 0, 0, 0.5, 0, 1, 0, -0.1, 0, 0, 1, 0.02], new, track, thr, hw, hh)
    strength, made = literal_add_keyframe(g, oldkey, 7777, [1, 0, 0, 0.5, 0, 1, 0, -0.1, 0, 0, 1, 0.02], new, track, thr, width, height, rng)
    assert {k[0]: k[1] for k in out["keys"]} == strength
    assert [e[0] for e in out["edges"]] == sorted(made) and all(g["edges"][(min(a, b), max(a, b))] == s for a, b, s in out["edges"])
    assert out["pose"] == g["vertex"][7777]["T"]
    assert set(model.vis) == set(g["point"]) and all(model.vis[p] == g["point"][p]["vis_set"] for p in model.vis)
    assert [p["point_id"] for p, c in zip(new, out["kept"]) if c] == [p["point_id"] for p in new if p["point_id"] in g["point"]]
    # every feature table: the pairs of the log, with the measurement the reference's insert keeps
    ft = {}
    for pid, kf, center, level in out["pairs"]:
        assert (pid, kf) not in ft
        ft[(pid, kf)] = (center, level)
    for kf, v in g["vertex"].items():
        for pid, feat in v["feature_table"].items():
            assert ft.pop((pid, kf)) == feat
    assert not ft
    return out


@pytest.mark.parametrize("thr", [0, 1, 2, 3, 15])
def test_closed_form_and_add_keyframe_equal_the_literal_restatement(thr):
    clamped = dropped = 0
    for seed in range(60):
        rng = np.random.default_rng(1000 * thr + seed)
        g, oldkey, new, track, size = _case(rng, thr, n_track=int(rng.integers(1, 70)), n_kf=int(rng.integers(2, 9)))
        out = _check(g, oldkey, new, track, size, thr, rng if seed % 2 else None)
        want, _ = literal_compute_strength(new, track, {p: q["vis_set"] for p, q in g["point"].items() if p < 5000}, thr, *size)
        clamped += want[oldkey] < thr
        dropped += sum(not c for c in out["kept"])
    if thr >= 2:
        assert clamped >= 1 and dropped >= 1                       # an oldkey that needs the clamp; new points whose anchor was zeroed


def test_no_track_point_of_the_map_keeps_the_new_points_counts():
    rng = np.random.default_rng(5)
    g, oldkey, new, _, size = _case(rng, 3)
    for track in ([], [dict(global_id=9001, center=[1.0, 1.0, 0.0], level=0)] * 3):
        gg = dict(vertex={k: dict(v, feature_table={}) for k, v in g["vertex"].items()}, point={p: dict(vis_set=set(q["vis_set"])) for p, q in g["point"].items()}, edges={})
        out = _check(gg, oldkey, new, track, size, 3, rng)
        assert out["m"] == 0 and {k[0]: k[1] for k in out["keys"] if k[0] != oldkey} == {a: sum(1 for p in new if p["anchor_id"] == a) for a in {p["anchor_id"] for p in new} - {oldkey}}


def test_duplicates_count_twice_and_the_first_feature_wins():
    g = dict(vertex={1: dict(T=list(AM.I12), feature_table={}), 2: dict(T=list(AM.I12), feature_table={})}, point={10: dict(vis_set={1, 2}), 11: dict(vis_set={1})}, edges={})
    track = [dict(global_id=10, center=[1.0, 1.0, 0.5], level=0), dict(global_id=10, center=[600.0, 400.0, 0.25], level=1), dict(global_id=404, center=[0.0, 0.0, 0.0], level=0),
             dict(global_id=11, center=[2.0, 2.0, 0.0], level=2)]
    out = _check(g, 1, [], track, (640, 480), 2, None)
    assert {k[0]: k[1] for k in out["keys"]} == {1: 2, 2: 1}     # both cross at the second entry: it and what follows count
    assert [q[:2] for q in out["pairs"]] == [(10, 7777), (11, 7777)] and out["pairs"][0][2] == [1.0, 1.0, 0.5] and out["exists"] == [True, True, False, True]


def test_a_centre_on_the_half_size_is_right_and_bottom_and_an_odd_width_truncates():
    for width, u, left in ((640, 320.0, False), (640, 319.999, True), (641, 320.0, False), (641, 319.5, True), (641, 320.5, False)):
        g = dict(vertex={1: dict(T=list(AM.I12), feature_table={})}, point={10: dict(vis_set={1})}, edges={})
        track = [dict(global_id=10, center=[u, 240.0, 0.0], level=0)]
        out = _check(g, 1, [], track, (width, 480), 0, None)
        assert out["keys"][0][2:6] == [int(left), int(not left), 0, 1]
    assert int(641 * 0.5) == 320


def test_a_rotated_list_changes_the_strengths():
    """the zeroing runs after every track point: where the h-th entries lie in the list decides what is counted"""
    vis = {p: {1} for p in range(8)}
    track = [(0, 1.0, 1.0), (1, 600.0, 400.0)] + [(p, 1.0, 1.0) for p in range(2, 8)]
    a, _, _ = AM.strength_closed_form([], track, vis, 2, 320, 240)
    b, _, _ = AM.strength_closed_form([], track[2:] + track[:2], vis, 2, 320, 240)
    assert a[0][1] == 7 and b[0][1] == 1 and a[0][2:] == b[0][2:]


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree(tmp_path):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import (MAP_ADDKF_MAX_NEIGHBORS, MAP_KEY_DTYPE, MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE, MapAddKeyframeArgs, MapStrengthResult)
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    lib = capi.load()
    for n in ADDKF_SYMBOLS:
        assert n in capi.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
    fields = ["offsetof(svs_map_new_point,feat_center)", "offsetof(svs_map_new_point,point_id)", "offsetof(svs_map_new_point,feat_level)", "sizeof(svs_map_new_point)",
              "offsetof(svs_map_track_point,global_id)", "sizeof(svs_map_track_point)", "offsetof(svs_map_key,edge)", "sizeof(svs_map_key)",
              "sizeof(svs_map_strength_result)", "offsetof(svs_map_add_keyframe_args,T_newkey_from_oldkey)", "offsetof(svs_map_add_keyframe_args,keyframe)",
              "offsetof(svs_map_add_keyframe_args,disp)", "offsetof(svs_map_add_keyframe_args,track_points)", "offsetof(svs_map_add_keyframe_args,n_cached)",
              "sizeof(svs_map_add_keyframe_args)", "(size_t)SVS_MAP_ADDKF_MAX_NEIGHBORS"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){' + "".join('printf("%%zu\\n",(size_t)%s);' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = MapAddKeyframeArgs
    assert got == [MAP_NEW_POINT_DTYPE.fields["feat_center"][1], MAP_NEW_POINT_DTYPE.fields["point_id"][1], MAP_NEW_POINT_DTYPE.fields["feat_level"][1],
                   MAP_NEW_POINT_DTYPE.itemsize, MAP_TRACK_POINT_DTYPE.fields["global_id"][1], MAP_TRACK_POINT_DTYPE.itemsize, MAP_KEY_DTYPE.fields["edge"][1],
                   MAP_KEY_DTYPE.itemsize, C.sizeof(MapStrengthResult), A.T_newkey_from_oldkey.offset, A.keyframe.offset, A.disp.offset, A.track_points.offset,
                   A.n_cached.offset, C.sizeof(A), MAP_ADDKF_MAX_NEIGHBORS]
