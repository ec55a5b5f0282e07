"""svs_frontend_set_neighborhood_from_store: svs_frontend_set_neighborhood_from_root with the head taken from the streams' new-point stores, against a TWIN front end
fed through setNeighborhoodFromMap with the store's read-back as its host head -- the active keyframe's group first (the fixed group), the other groups behind it in
store order with their keys, kf_index set by the slot rule of tests/newpoint_model.py (the slot that holds the group's keyframe, -1 without one).  Scene, map and
front ends: those of tests/test_gpu_nbh_root.py, which holds the root call itself to its model.

Bars.  Copying and integer selection only: the candidate table, point ids, vertex rows, strength matrix, resident vertex table and the result record are the twin's
bytes; after one step so are the match, gate and decision records.  The map and the stores are byte-equal before and after."""
import numpy as np
import pytest

import newpoint_model as NM
import test_gpu_nbh_root as NR
from test_gpu_nbh_root import both, frames_of, host_frames      # noqa: F401 (fixtures)
from test_gpu_neighborhood import device_scene, scene           # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
HUB, LONE = NR.HUB, NR.LONE


def records(scene, n, first_id):
    r = np.array(scene["src"][:n])
    r["kf_index"], r["point_id"] = 2, first_id + np.arange(n)      # the stored kf_index is not used
    return r


def fill_store(fe, scene, stream, groups):
    """groups: (key, size) in store order -> the model of the stream's store"""
    m = NM.Store(fe.newpoint_record_cap, 16)
    puts = []
    for i, (key, size) in enumerate(groups):
        puts.append(dict(stream=stream, kf_id=key, records=records(scene, size, 3000 + 100 * i)))
    fe.putNewpoints(puts)
    m.put_all(puts)
    return m


def twin_request(store, model, q):
    """the request setNeighborhoodFromMap takes for the same list: act's group first (empty when the store has none), then every other group whose key is a keyframe
    of the map, in store order; kf_index by the slot rule among the slots that name a keyframe of the map"""
    slot = [k if k in model.kf else -1 for k in q["slot_kf"]]
    order = [q["act_id"]] + [k for k in store.keys if k != q["act_id"] and k in model.kf]
    parts = []
    for k in order:
        g = store.groups[store.keys.index(k)].copy() if k in store.keys else np.zeros(0, store.records().dtype)
        g["kf_index"] = slot.index(k) if k in slot else -1
        parts.append(g)
    head = np.concatenate(parts)
    dropped_outside = sum(len(store.groups[i]) for i, k in enumerate(store.keys) if k != q["act_id"] and k not in model.kf)
    return dict(q, head=head, head_group_end=[int(e) for e in np.cumsum([len(p) for p in parts])], n_fixed_groups=1, head_group_kf=[-1] + order[1:]), dropped_outside


def same(o, t, b, dropped_outside=0, what=""):
    from scavislam_amd.ctypes_types import NBR_RESULT_FIELDS
    for f in NBR_RESULT_FIELDS:
        assert o[f] == t[f] + (dropped_outside if f == "n_head_dropped" else 0), f"{what}: {f} {o[f]} vs the twin's {t[f]}"
    assert o["raw"][1:] == t["raw"][1:], f"{what}: point ids, vertex rows or strength matrix differ from the twin's"
    assert o["table"][b].tobytes() == t["table"][b].tobytes(), f"{what}: the candidate table differs from the twin's"
    assert o["kf_table"].tobytes() == t["kf_table"].tobytes() and o["kf_vertex"].tobytes() == t["kf_vertex"].tobytes(), f"{what}: the resident vertex table differs"
    assert o["slot_T"].tobytes() == t["slot_T"].tobytes(), f"{what}: slot poses"


STORES = [[(13, 4), (40, 5), (7, 5), (19, 1), (HUB, 6), (41, 0)],      # act 40 in the middle; 7 is never a neighbour of 40: dropped; an empty group
          [(19, 3), (13, 2), (99999, 4), (HUB, 7)]]                     # no group of act (an empty fixed group); 99999 is no keyframe of the map: left out


def test_twin_front_end_fed_the_stores_read_back(gpu_ctx, frames_of, scene, both):
    model, table, dmap = both
    ctx = gpu_ctx[0]
    fe, tfe = NR._make_fe(ctx, frames_of, model), NR._make_fe(ctx, frames_of, model)
    try:
        fe.reserveNewpoints(64, 16)
        stores = [fill_store(fe, scene, b, STORES[b]) for b in range(2)]
        reqs = [NR._q(0, 40, 40), NR._q(1, HUB, 40, slot_kf=NR.slots((25,)))]
        map_before, stores_before = NR._map_bytes(dmap, model), [(s["raw"], s["records"].tobytes()) for s in fe.newpoints()]
        outs = fe.setNeighborhoodFromStore(dmap.map, reqs, want_records=True, want_tables=True)
        for b, (q, o) in enumerate(zip(reqs, outs)):
            tq, outside = twin_request(stores[b], model, q)
            t = tfe.setNeighborhoodFromMap(dmap.map, [tq], want_records=True, want_tables=True)[0]
            assert not o["over_capacity"] and not o["root_outside_window"] and o["n_head_kept"] > 0
            same(o, t, b, outside, f"stream {b}")
            assert fe.n_points[b] == tfe.n_points[b] == o["n_points"]
        assert outs[0]["n_head_dropped"] == 5 and outs[1]["n_head_dropped"] >= 4
        # the head's kf_index is the slot rule's: keyframe 40 sits in slot 4, 13 in slot 1, HUB in slot 5
        head0 = outs[0]["table"][0][:outs[0]["n_head_kept"]]
        assert set(head0["kf_index"][:5]) == {4} and set(head0["kf_index"]) <= {1, 2, 4, 5}
        a, b_ = NR._step(fe, frames_of, scene), NR._step(tfe, frames_of, scene)
        assert a == b_ and a[0][3] >= 20, "the twin tracks differently"
        for x, y in zip(fe.decideKeyframes(dmap.map, want_lists=2), tfe.decideKeyframes(dmap.map, want_lists=2)):
            assert x["dec"].tobytes() == y["dec"].tobytes() and x["dec"]["valid"] == 1
            for f in ("new", "track", "new_rec", "track_rec"):
                assert x[f].tobytes() == y[f].tobytes()
        assert NR._map_bytes(dmap, model) == map_before, "the map changed"
        assert [(s["raw"], s["records"].tobytes()) for s in fe.newpoints()] == stores_before, "a store changed"
        # a second run gives the same bytes; a head field in a request, or a front end without a store, is refused
        again = fe.setNeighborhoodFromStore(dmap.map, reqs, want_records=True, want_tables=True)
        for b, (o, o2) in enumerate(zip(outs, again)):
            same(o2, o, b, 0, f"stream {b} again")
        from scavislam_amd.capi import SvsError
        with pytest.raises(ValueError):
            fe.setNeighborhoodFromStore(dmap.map, [dict(reqs[0], head=records(scene, 1, 1))])
        with pytest.raises(SvsError, match=NR.INVALID):      # (the C call itself: a head field beside a store)
            fe.setNeighborhoodFromMap(dmap.map, [dict(reqs[0], head=records(scene, 1, 1), head_group_end=[1], head_group_kf=[-1])], _from_store=True)
        with pytest.raises(SvsError, match=NR.INVALID):
            tfe.setNeighborhoodFromStore(dmap.map, reqs)      # nothing reserved
        n0 = outs[0]["n_points"]
    finally:
        fe.close(); tfe.close()
    # max_points exactly the list's length, and one less: all or nothing, the result record the twin's
    for mp, over in ((n0, 0), (n0 - 1, 1)):
        fe, tfe = NR._make_fe(ctx, frames_of, model, B=1, max_points=mp), NR._make_fe(ctx, frames_of, model, B=1, max_points=mp)
        try:
            fe.reserveNewpoints(64, 16)
            store = fill_store(fe, scene, 0, STORES[0])
            o = fe.setNeighborhoodFromStore(dmap.map, reqs[:1], want_records=True, want_tables=True)[0]
            t = tfe.setNeighborhoodFromMap(dmap.map, [twin_request(store, model, reqs[0])[0]], want_records=True, want_tables=True)[0]
            assert o["over_capacity"] == over and (over or o["n_points"] == mp)
            same(o, t, 0, 0, f"max_points {mp}")
            assert not over or (o["table"][0].view(np.uint8) == 0xFF).all()
        finally:
            fe.close(); tfe.close()


def test_a_batch_of_33_equals_streams_alone_on_a_fresh_front_end(gpu_ctx, frames_of, scene, both):
    model, table, dmap = both
    ctx = gpu_ctx[0]
    B = 33
    roots = [(HUB, 40, 10), (40, 40, 10), (LONE, LONE, 10), (7, 7, 10), (HUB, HUB, 0), (40, 3, 1), (13, 40, 10), (HUB, 19, 20)]
    rng = np.random.default_rng(7)
    keys = [13, 40, 7, 19, HUB, 41, LONE, 99999]
    layouts = [[(int(k), int(rng.integers(0, 7))) for k in rng.permutation(keys)[:int(rng.integers(0, 8))]] for _ in range(B)]
    reqs = [NR._q(b, *roots[b % len(roots)], slot_kf=NR.slots((25,) if b % 3 == 0 else ())) for b in range(B)]
    fe = NR._make_fe(ctx, frames_of, model, B=B)
    try:
        fe.reserveNewpoints(64, 16)
        for b in range(B):
            fill_store(fe, scene, b, layouts[b])
        order = [int(r) for r in rng.permutation(B)]
        outs = fe.setNeighborhoodFromStore(dmap.map, [reqs[r] for r in order], want_records=True, want_tables=True)
        by_stream = {r: o for r, o in zip(order, outs)}
        again = fe.setNeighborhoodFromStore(dmap.map, reqs, want_records=True, want_tables=True)
        for b in range(B):
            o, o2 = by_stream[b], again[b]
            assert o["raw"] == o2["raw"] and o["table"][b].tobytes() == o2["table"][b].tobytes() and o["kf_vertex"].tobytes() == o2["kf_vertex"].tobytes(), f"stream {b}: a second run differs"
        assert {bool(o["root_outside_window"]) for o in outs} == {False, True}
    finally:
        fe.close()
    one = NR._make_fe(ctx, frames_of, model, B=1)
    try:
        one.reserveNewpoints(64, 16)
        for b in (0, 1, 5, 14, 32):
            cur = one.newpoints([0], want_records=False)[0]["keys"]
            one.dropNewpointGroups([dict(stream=0, keys=[int(k) for k in cur])])
            fill_store(one, scene, 0, layouts[b])
            o = one.setNeighborhoodFromStore(dmap.map, [dict(reqs[b], stream=0)], want_records=True, want_tables=True)[0]
            w = by_stream[b]
            assert o["raw"] == w["raw"], f"stream {b} alone: outputs differ from its place in the batch"
            if not (o["over_capacity"] or o["root_outside_window"]):
                n = o["n_points"]
                assert o["table"][0][:n].tobytes() == w["table"][b][:n].tobytes(), f"stream {b} alone: the list differs from its place in the batch"
                assert o["kf_table"].tobytes() == w["kf_table"].tobytes() and o["kf_vertex"].tobytes() == w["kf_vertex"].tobytes()
    finally:
        one.close()


def test_cpp_adaptor_takes_the_head_from_the_store(gpu_ctx, tmp_path):
    """tests/cpp/newpoints_nbh_smoke.cpp: StereoFrontend::setNeighborhoodFromStore of include/scavislam_hip.hpp (one stream, and stream 1 of a batch front end)
    against setNeighborhoodFromMap fed the same lists from the host, compiled with g++ -std=c++11"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "newpoints_nbh_smoke"
    libdir = os.path.join(root, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "newpoints_nbh_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("NEWPOINTS_NBH ")]
    assert tok and tok[0].split()[1] == "ok", out
    assert [int(v) for v in tok[0].split()[3:5]] == [5, 1]
