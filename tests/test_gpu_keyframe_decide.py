"""The keyframe decision on the device (svs_keyframe_decide: processMatchedPoints' lists, shallWeSwitchKeyframe, shallWeDropNewKeyframe and addNewKeyframe's
bookkeeping, stereo_frontend.cpp:265-296) against the NumPy restatement tests/keyframe_model.py, which tests/test_keyframe_cpu.py holds to the reference's loops.

Bounds.  The lists are copies and integer compaction; the decisions are integer comparisons and comparisons of f64 values formed by the expression trees the
model writes out (pose.h's row sums, one IEEE square root, one division), compiled without contraction: every output byte must be the model's.  Inputs are
synthetic; the edges are placed on the thresholds themselves."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import keyframe_model as KM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS = 2048
FILL = 0xAB


def run_decide(gpu_ctx, cases, prm=None, resident_map=None, uniform_n=False, vertex_cap=None, cap=None, expect_error=False):
    """one svs_keyframe_decide call over a batch of streams (dicts as keyframe_model.random_case makes them; a set given as the string "map" is read from
    resident_map, `map_sets` then holds its content for the model).  Returns per stream the raw bytes (decision, lists up to their counts) and checks that nothing
    behind a list's count was written."""
    import torch
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import (CANDIDATE_DTYPE, GATED_POINT_DTYPE, KEYFRAME_DECISION_DTYPE, KF_MAX_VERTICES, KF_SET_MAP, KF_TABLE_DTYPE, KF_VERTEX_DTYPE,
                                            MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE, MATCH_RESULT_DTYPE, POINT_STATS_DTYPE, KeyframeDecideArgs, KeyframeDecideParams)
    ctx, stream = gpu_ctx
    B = len(cases)
    n = max(len(c["res"]) for c in cases)
    if uniform_n:
        assert all(len(c["res"]) == n for c in cases)
    cap = n if cap is None else cap
    VB = max(len(c["table"]["kf"]) for c in cases) if vertex_cap is None else vertex_cap
    S = len(cases[0]["table"]["slot_kf"])
    res, pts, gated = np.zeros((B, n + 3), MATCH_RESULT_DTYPE), np.zeros((B, n + 5), CANDIDATE_DTYPE), np.zeros((B, n + 1), GATED_POINT_DTYPE)
    res["status"], gated["accepted"], gated["is_new"] = 5, 1, 1      # behind a stream's own records: not OK, with accepted garbage
    stats, T, ok, ns = np.zeros(B, POINT_STATS_DTYPE), np.zeros((B, 12)), np.zeros(B, np.int32), np.zeros(B, np.int32)
    tab, vtx, slot = np.zeros(B, KF_TABLE_DTYPE), np.zeros((B, max(VB, 1)), KF_VERTEX_DTYPE), np.zeros((B, S + 2), np.int32)
    id_rows = []
    for b, c in enumerate(cases):
        k, t = len(c["res"]), c["table"]
        res[b, :k], pts[b, :k], gated[b, :k] = c["res"], c["pts"], c["gated"]
        stats[b], T[b], ok[b], ns[b] = c["stats"], np.asarray(c["T_cur"], np.float64).reshape(12), c.get("tracking_ok", 1), k
        V = len(t["kf"])
        tab[b]["n_vertex"], tab[b]["act"], tab[b]["n_neighbors"] = V, t["act"], len(t["neighbors"])
        tab[b]["neighbors"][:len(t["neighbors"])] = t["neighbors"]
        row = []
        for v in range(min(V, VB)):
            vtx[b, v]["T_me_from_w"], vtx[b, v]["kf_id"] = np.asarray(t["T"][v], np.float64).reshape(12), t["kf"][v]
            if isinstance(t["sets"][v], str):
                vtx[b, v]["set_begin"] = KF_SET_MAP
            else:
                ids = sorted(int(i) for i in t["sets"][v])
                vtx[b, v]["set_begin"], vtx[b, v]["set_count"] = len(row), len(ids)
                row += ids
        id_rows.append(row)
        slot[b, :S] = t["slot_kf"]
    SB = max(1, max(len(r) for r in id_rows))
    ids = np.full((B, SB), -77, np.int32)
    for b, r in enumerate(id_rows):
        ids[b, :len(r)] = r
    with torch.cuda.stream(stream):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        d = dict(res=dev(res), pts=dev(pts), gated=dev(gated), stats=dev(stats), T=dev(T), ok=dev(ok), n=dev(ns), tab=dev(tab), vtx=dev(vtx), slot=dev(slot), ids=dev(ids))
        rows = max(cap, 1)
        out = dict(dec=dev(np.full((B, KEYFRAME_DECISION_DTYPE.itemsize), FILL, np.uint8)), new=dev(np.full((B, rows, 96), FILL, np.uint8)),
                   track=dev(np.full((B, rows, 32), FILL, np.uint8)), new_rec=dev(np.full((B, rows, 4), FILL, np.uint8)), track_rec=dev(np.full((B, rows, 4), FILL, np.uint8)))
    a = KeyframeDecideArgs()
    a.d_res, a.res_bstride, a.d_pts, a.pts_bstride, a.d_gated, a.gated_bstride = d["res"].data_ptr(), n + 3, d["pts"].data_ptr(), n + 5, d["gated"].data_ptr(), n + 1
    a.d_stats, a.d_T_cur_from_actkey, a.d_tracking_ok = d["stats"].data_ptr(), d["T"].data_ptr(), d["ok"].data_ptr()
    a.d_n, a.n, a.batch = (None if uniform_n else d["n"].data_ptr()), n, B
    a.d_table, a.d_vertex, a.vertex_bstride = d["tab"].data_ptr(), d["vtx"].data_ptr(), max(VB, 1)
    a.d_set_ids, a.set_bstride, a.d_slot_kf, a.slot_bstride, a.max_keyframes = d["ids"].data_ptr(), SB, d["slot"].data_ptr(), S + 2, S
    a.map = resident_map.h if resident_map is not None else None
    p = KeyframeDecideParams.reference()
    for k, v in (prm or {}).items():
        setattr(p, k, v)
    err = None
    try:
        ctx.call("svs_keyframe_decide", C.byref(a), C.byref(p), out["dec"].data_ptr(), out["new"].data_ptr(), out["track"].data_ptr(), out["new_rec"].data_ptr(),
                 out["track_rec"].data_ptr(), cap)
    except SvsError as e:
        err = e
    ctx.sync()
    assert (err is not None) == expect_error, err
    h = {k: v.cpu().numpy() for k, v in out.items()}
    if expect_error:
        assert all((v == FILL).all() for v in h.values()), "a refused call wrote"
        return err
    dec = h["dec"].view(KEYFRAME_DECISION_DTYPE).reshape(B)
    got = []
    for b in range(B):
        nn, nt = (int(dec[b]["n_new"]), int(dec[b]["n_track"])) if dec[b]["valid"] else (0, 0)
        new, track = h["new"].reshape(B, rows, 96)[b], h["track"].reshape(B, rows, 32)[b]
        new_rec, track_rec = h["new_rec"].reshape(B, rows, 4)[b], h["track_rec"].reshape(B, rows, 4)[b]
        assert (new[nn:] == FILL).all() and (new_rec[nn:] == FILL).all() and (track[nt:] == FILL).all() and (track_rec[nt:] == FILL).all(), f"stream {b}: wrote behind its lists"
        got.append(dict(dec=dec[b].tobytes(), new=new[:nn].tobytes(), track=track[:nt].tobytes(), new_rec=new_rec[:nn].tobytes(), track_rec=track_rec[:nt].tobytes(),
                        record=dec[b].copy(), new_points=new[:nn].copy().view(MAP_NEW_POINT_DTYPE).reshape(-1), track_points=track[:nt].copy().view(MAP_TRACK_POINT_DTYPE).reshape(-1)))
    return got


def model_bytes(c, prm=None):
    t = c["table"]
    if any(isinstance(s, str) for s in t["sets"]):
        t = dict(t, sets=[c["map_sets"][v] if isinstance(s, str) else s for v, s in enumerate(t["sets"])])
    m = KM.decide(c["res"], c["pts"], c["gated"], c["stats"], c["T_cur"], c.get("tracking_ok", 1), t, prm)
    return dict(dec=m["dec"].tobytes(), new=m["new"].tobytes(), track=m["track"].tobytes(), new_rec=m["new_rec"].tobytes(), track_rec=m["track_rec"].tobytes(), record=m["dec"])


def assert_equal(got, cases, prm=None, what=""):
    for b, (g, c) in enumerate(zip(got, cases)):
        w = model_bytes(c, prm)
        for k in ("new_rec", "track_rec", "new", "track", "dec"):
            if g[k] != w[k]:
                detail = ""
                if k == "dec":
                    detail = "; ".join(f"{f}: {g['record'][f]} vs {w['record'][f]}" for f in g["record"].dtype.names if g["record"][f].tobytes() != w["record"][f].tobytes())
                raise AssertionError(f"{what} stream {b}: {k} differs from the model's ({detail})")


def masked(c, mode):
    """the accepted / new flags of a case rewritten: none, all, new, track, alt1 (alternating per record), alt64 (per 64-record run)"""
    c = dict(c, res=c["res"].copy(), gated=c["gated"].copy())
    i = np.arange(len(c["res"]))
    c["res"]["status"] = 0
    if mode == "none":
        c["gated"]["accepted"] = 0
    elif mode in ("all", "new", "track"):
        c["gated"]["accepted"] = 1
        if mode != "all":
            c["gated"]["is_new"] = int(mode == "new")
    elif mode == "alt1":
        c["gated"]["accepted"] = i & 1
    else:
        c["gated"]["accepted"] = (i >> 6) & 1 ^ 1
    return c


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, MAX_POINTS])
def test_lists_at_the_chunk_and_wave_edges(gpu_ctx, n):
    rng = np.random.default_rng(n)
    cases = [masked(KM.random_case(rng, n=n, V=3), mode) for mode in ("none", "all", "new", "track", "alt1", "alt64")]
    garbage = KM.random_case(rng, n=n, V=3)                        # records that are not OK carry accepted = 1: ignored
    garbage["gated"]["accepted"] = 1
    assert n == 1 or (garbage["res"]["status"] != 0).any()
    cases.append(garbage)
    prm = dict(switch_min_shared=5, covis_thr=3)
    assert_equal(run_decide(gpu_ctx, cases, prm, uniform_n=True), cases, prm, f"n = {n}")


def _plain(rng, n=300, V=3, **kw):
    """a case that neither switches nor drops by itself: far vertices, full cells, short tracks"""
    c = KM.random_case(rng, n=n, V=V, force="keep")
    t = c["table"]
    c["T_cur"] = list(KM.I12)
    for v in range(V):
        t["T"][v] = [1, 0, 0, 5.0 + v, 0, 1, 0, 0, 0, 0, 1, 0]
    t["T"][t["act"]] = list(KM.I12)
    c["res"]["status"], c["gated"]["accepted"] = 0, 1
    c["stats"]["sum_track_length"], c["stats"]["num_track_points"] = 500.0, 50
    c.update(kw)
    return c


@pytest.mark.parametrize("V", [1, 2, 64])
def test_vertex_counts(gpu_ctx, V):
    rng = np.random.default_rng(V)
    cases = [KM.random_case(rng, n=200, V=V, force=f) for f in ("switch", "drop", "keep", None)]
    prm = dict(switch_min_shared=3, covis_thr=2)
    got = run_decide(gpu_ctx, cases, prm)
    assert_equal(got, cases, prm, f"V = {V}")
    if V == 1:
        assert all(g["record"]["closest_index"] == -1 and g["record"]["decision"] != KM.KF_SWITCH for g in got)


def test_more_vertices_than_the_table_holds_is_refused(gpu_ctx):
    c = KM.random_case(np.random.default_rng(65), n=50, V=65)
    err = run_decide(gpu_ctx, [c], vertex_cap=65, expect_error=True)
    assert "status 4" in str(err)                                  # SVS_ERR_CAPACITY
    # a table that claims more vertices than its row holds is malformed: the stream comes back invalid
    got = run_decide(gpu_ctx, [c], vertex_cap=64)
    assert got[0]["dec"] == bytes(len(got[0]["dec"]))
    err = run_decide(gpu_ctx, [KM.random_case(np.random.default_rng(1), n=50, V=2)], cap=49, expect_error=True)
    assert "status 4" in str(err)


def test_switch_edges(gpu_ctx):
    rng = np.random.default_rng(11)
    cases = []
    # two vertices at bit-equal distance: the lower index; exactly at the bound: not closer; a NaN pose: never closer
    for T1, T2, T3 in (([1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0.25, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.25]),
                       ([1, 0, 0, 0.375, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0.375, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.25]),
                       ([1, 0, 0, 0.375, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, math.nextafter(0.375, 0), 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, float("nan")]),
                       ([float("nan")] * 12, [1, 0, 0, 0.375, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, float("nan")])):
        c = _plain(rng, V=4)
        c["table"].update(act=0, neighbors=[2], T=[list(KM.I12), T1, T2, T3])
        cases.append(c)
    want_closest = [1, 3, 2, -1]
    # shared = 100 and 101 against switch_min_shared = 100, the 101st by an id listed twice
    for shared in (100, 101):
        c = _plain(rng, n=300, V=2)
        c["table"].update(act=0, neighbors=[], T=[list(KM.I12), [1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, 1, 0]])
        c["gated"]["is_new"] = 0
        c["pts"]["point_id"] = 1000 + np.arange(300)
        c["pts"]["point_id"][299] = 1000                           # listed twice
        c["table"]["sets"][1] = list(range(1000, 1099)) + ([1250] if shared == 101 else [5000])      # 99 ids of the list, one of them listed twice; + one more / a stranger
        cases.append(c)
    got = run_decide(gpu_ctx, cases)
    assert_equal(got, cases, None, "switch edges")
    assert [int(g["record"]["closest_index"]) for g in got[:4]] == want_closest
    assert [int(g["record"]["shared"]) for g in got[4:]] == [100, 101] and [int(g["record"]["decision"]) for g in got[4:]] == [KM.KF_KEEP, KM.KF_SWITCH]
    assert got[0]["record"]["closest_dist"] == 0.25 and got[3]["record"]["closest_dist"] == 0.0 and got[3]["record"]["closest_id"] == -1


def test_drop_edges(gpu_ctx):
    rng = np.random.default_rng(12)
    cases, want = [], []
    thr = float(np.float32(0.75))
    for cells, drop in (([14, 14, 15, 40], False), ([14, 14, 14, 40], True), ([15, 15, 15, 15], False), ([14, 14, 14, 14], True)):
        c = _plain(rng)
        c["stats"]["num_points_grid2x2"] = cells
        cases.append(c); want.append(drop)
    for t, drop in ((thr, False), (math.nextafter(thr, 2.0), True)):   # the translation norm at parallax_thr and one ulp above (sqrt of a square is exact here)
        c = _plain(rng)
        c["T_cur"] = [1, 0, 0, 0, 0, 1, 0, t, 0, 0, 1, 0]
        cases.append(c); want.append(drop)
    for s, m, drop in ((75.0, 1, False), (math.nextafter(75.0, math.inf), 1, True), (0.0, 0, False), (1.0, 0, True), (7500.0, 100, False)):
        c = _plain(rng)
        c["stats"]["sum_track_length"], c["stats"]["num_track_points"] = s, m
        cases.append(c); want.append(drop)
    got = run_decide(gpu_ctx, cases)
    assert_equal(got, cases, None, "drop edges")
    assert [int(g["record"]["decision"]) == KM.KF_DROP for g in got] == want
    assert got[8]["record"]["av_track_length"].tobytes() == KM.QUIET_NAN.tobytes()


def _strength_case(rng, counts, ids, anchor_outside=False):
    """a dropping stream whose new entries are anchored in slots 0 .. len(counts) - 1 (keyframe ids `ids`) counts[k] times each, no track entry"""
    n = int(sum(counts))
    c = _plain(rng, n=n, V=3)
    S = len(c["table"]["slot_kf"])
    assert len(counts) <= S
    slot = np.full(S, -1, np.int32)
    slot[:len(ids)] = ids
    c["table"].update(kf=[ids[0], ids[1], 7000], act=0, neighbors=[1], slot_kf=slot, sets=[[], [], []])
    c["gated"]["is_new"] = 1
    c["pts"]["kf_index"] = np.repeat(np.arange(len(counts)), counts)
    c["pts"]["point_id"] = 100 + np.arange(n)
    c["stats"]["num_points_grid2x2"] = 0                           # drops
    return c


def test_strength_edges(gpu_ctx):
    rng = np.random.default_rng(13)
    cases = [_strength_case(rng, [15, 16, 40], [5, 9, 300]),       # num_matches 15 / 16 against covis_thr 15; slot 2's anchor is neither act nor a neighbour
             _strength_case(rng, [20, 20, 20], [9, 5, 7]),         # equal counts, ids in both orders
             _strength_case(rng, [20, 20, 20], [5, 9, 11])]
    # track entries count for act and its neighbour only, on top of the new entries anchored there
    c = _strength_case(rng, [10, 10, 10], [5, 9, 300])
    extra = _plain(rng, n=60, V=3)
    c["res"], c["gated"] = np.concatenate([c["res"], extra["res"]]), np.concatenate([c["gated"], extra["gated"]])
    c["gated"]["is_new"][30:] = 0
    pts = extra["pts"].copy()
    pts["point_id"], pts["kf_index"] = 2000 + np.arange(60), 0
    c["pts"] = np.concatenate([c["pts"], pts])
    c["table"]["sets"] = [list(range(2000, 2006)), list(range(2000, 2030)), list(range(2000, 2060))]      # act 10 + 6 = 16, the neighbour 10 + 30, vertex 2 nothing
    cases.append(c)
    got = run_decide(gpu_ctx, cases)
    assert_equal(got, cases, None, "strength edges")
    r = [g["record"] for g in got]
    assert r[0]["n_strength"] == 2 and r[0]["strength_kf"][:2].tolist() == [9, 300] and r[0]["strength_count"][:2].tolist() == [16, 40]
    assert r[1]["strength_kf"][:3].tolist() == [5, 7, 9] and r[2]["strength_kf"][:3].tolist() == [5, 9, 11]
    assert r[3]["strength_kf"][:2].tolist() == [5, 9] and r[3]["strength_count"][:2].tolist() == [16, 40] and r[3]["n_strength"] == 2


def test_more_strength_keys_than_the_record_holds(gpu_ctx):
    rng = np.random.default_rng(14)
    for keys, over in ((64, 0), (65, 1)):
        n = keys * 2
        c = _plain(rng, n=n, V=2)
        slot = np.full(80, -1, np.int32)
        slot[:keys] = 3000 - 7 * np.arange(keys)
        c["table"].update(kf=[int(slot[0]), 1], act=0, neighbors=[], slot_kf=slot, sets=[[], []])
        c["gated"]["is_new"] = 1
        c["pts"]["kf_index"] = np.arange(n) % keys
        c["pts"]["point_id"] = np.arange(n)
        c["stats"]["num_points_grid2x2"] = 0
        prm = dict(covis_thr=1)
        got = run_decide(gpu_ctx, [c], prm)
        assert_equal(got, [c], prm, f"{keys} keys")
        assert got[0]["record"]["over_capacity"] == over and got[0]["record"]["n_strength"] == (0 if over else 64) and got[0]["record"]["valid"] == 1
        assert got[0]["record"]["decision"] == KM.KF_DROP and got[0]["record"]["n_new"] == n


def test_staged_and_map_backed_sets_give_identical_bytes(gpu_ctx):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, KEYFRAME_DTYPE
    from scavislam_amd.register import ResidentMap
    ctx, _ = gpu_ctx
    rng = np.random.default_rng(15)
    cases = [KM.random_case(rng, n=400, V=4, force=f) for f in ("switch", "drop", None)]
    rm = ResidentMap(ctx, max_keyframes=1024, max_points=8192, max_observations=1 << 16)
    try:
        # one map for the three streams: keyframe ids are made distinct per stream, the point ids are shared
        pairs = set()
        for b, c in enumerate(cases):
            c["table"]["kf"] = [int(k) + 100 * b + 500 for k in range(len(c["table"]["kf"]))]
            c["table"]["slot_kf"] = np.array([c["table"]["kf"][i % 4] if s >= 0 else -1 for i, s in enumerate(c["table"]["slot_kf"])], np.int32)
            for v, s in enumerate(c["table"]["sets"]):
                pairs |= {(int(p), c["table"]["kf"][v]) for p in s}
        kf_ids = sorted({k for _, k in pairs} | {k for c in cases for k in c["table"]["kf"]})
        import torch
        image = torch.zeros(256, dtype=torch.uint8, device="cuda")   # the keyframes' images are never read here: one small block stands for all of them
        kfs = np.zeros(len(kf_ids), KEYFRAME_DTYPE)
        kfs["pyr"], kfs["stride"] = image.data_ptr(), 16
        rm.add_keyframes(kf_ids, kfs, [(image.data_ptr(), 4)] * len(kf_ids), [[[25], [25], [25]]] * len(kf_ids))
        pt_ids = sorted({p for p, _ in pairs})
        pts = np.zeros(len(pt_ids), CANDIDATE_DTYPE)
        pts["kf_index"] = kf_ids[0]
        rm.add_points(pt_ids, pts)
        pairs = sorted(pairs)
        rm.add_observations([p for p, _ in pairs], [k for _, k in pairs])
        prm = dict(switch_min_shared=5, covis_thr=3)
        staged = run_decide(gpu_ctx, cases, prm)
        assert_equal(staged, cases, prm, "staged")
        backed = [dict(c, map_sets=c["table"]["sets"], table=dict(c["table"], sets=["map"] * 4)) for c in cases]
        mixed = [dict(c, map_sets=c["table"]["sets"], table=dict(c["table"], sets=["map", c["table"]["sets"][1], "map", c["table"]["sets"][3]])) for c in cases]
        for name, variant in (("map-backed", backed), ("mixed", mixed)):
            got = run_decide(gpu_ctx, variant, prm, resident_map=rm)
            for b in range(len(cases)):
                for k in ("dec", "new", "track", "new_rec", "track_rec"):
                    assert got[b][k] == staged[b][k], f"{name} stream {b}: {k} differs from the staged run"
        assert any(g["record"]["shared"] > 0 for g in staged) and any(g["record"]["n_strength"] > 0 for g in staged)
    finally:
        rm.close()


def test_a_batch_equals_its_streams_alone_and_a_second_run(gpu_ctx):
    rng = np.random.default_rng(16)
    cases = [KM.random_case(rng, n=int(rng.integers(1, 600)), force=[None, "switch", "drop", "keep"][b % 4]) for b in range(33)]
    for b in (4, 17, 32):
        cases[b]["tracking_ok"] = 0
    prm = dict(switch_min_shared=5, covis_thr=3)
    batch = run_decide(gpu_ctx, cases, prm)
    assert_equal(batch, cases, prm, "batch of 33")
    again = run_decide(gpu_ctx, cases, prm)
    keys = ("dec", "new", "track", "new_rec", "track_rec")
    assert all(batch[b][k] == again[b][k] for b in range(33) for k in keys), "a second run differs"
    for b in (0, 4, 5, 6, 7, 31, 32):                              # (each alone: its own n, its own strides)
        alone = run_decide(gpu_ctx, [cases[b]], prm)[0]
        assert all(alone[k] == batch[b][k] for k in keys), f"stream {b} alone differs from its place in the batch"
    for b in (4, 17, 32):                                          # not tracked: zeroed, no list
        assert batch[b]["dec"] == bytes(len(batch[b]["dec"])) and batch[b]["new"] == b"" and batch[b]["track"] == b""
    seen = {int(g["record"]["decision"]) for g in batch if g["record"]["valid"]}
    assert seen == {KM.KF_KEEP, KM.KF_SWITCH, KM.KF_DROP}
