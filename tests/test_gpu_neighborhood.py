"""GPU tests of svs_frontend_set_candidates_from_map: a stream's neighbourhood list built on the device from the resident map (svs_map_*).  Every output is
held, byte for byte, against tests/neighborhood_model.py on a host mirror of the same map; frames run through one batched front end whose second stream is given
the model's list by svs_frontend_set_candidates_all and its poses by keepKeyframes -- the upload path is the yardstick.  Scene: register_model.make_scene() at
SMALL_CAM put into a map by register_map_model.fill(); the keyframes' frames are rendered again as make_scene renders them."""
import os
import subprocess

import numpy as np
import pytest

import neighborhood_model as NM
import register_map_model as MM
import register_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = M.SMALL_CAM
K = NM.N_SLOTS
ROOT_SLOT = 4
VCAP = 16
INVALID, CAPACITY = "status 1", "status 4"


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def device_scene(gpu_ctx, scene):
    import torch
    ctx, stream = gpu_ctx
    with torch.cuda.stream(stream):
        pyrs = [[torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in pyr] for pyr in scene["kf_pyrs"]]
        disp = torch.as_tensor(np.ascontiguousarray(scene["root_disp"], np.float32)).cuda()
        disp_copy = disp.clone()
        root_copy = [t.clone() for t in pyrs[0]]
    ctx.sync()
    return dict(pyrs=pyrs, disp=disp, disp_copy=disp_copy, root_copy=root_copy)


def _fill_both(ctx, dev, scene):
    from test_gpu_register_map import DeviceMap
    model, dmap = MM.MapModel(), DeviceMap(ctx, dev, scene)
    calls = None
    for m in (model, dmap):
        calls = MM.fill(m, scene, cand_ids_few=scene["src"]["point_id"][:10], attach=lambda e: dict(entry=e))
    return model, dmap, calls


@pytest.fixture(scope="module")
def both(gpu_ctx, device_scene, scene):
    model, dmap, _ = _fill_both(gpu_ctx[0], device_scene, scene)
    yield model, dmap
    dmap.close()


@pytest.fixture(scope="module")
def frames(gpu_ctx, scene):
    """device frames [2][h][w] (both streams see the same camera): the scene's keyframes 1 .. 4 rendered as make_scene renders them, a frame at the root's stored
    pose (the active keyframe) and the root's own image as the current frame"""
    import torch
    from scavislam_amd import synth
    ctx, stream = gpu_ctx
    sc = synth.Scene(2011)
    n_other = len(scene["kf_T"]) - 1
    traj = synth.trajectory(2 * n_other + 2)
    order = [k for k in range(2 * n_other + 1) if k != n_other][:n_other]
    host = [sc.render(CAM, traj[k], seed=k) for k in order]
    for e, (img, _) in enumerate(host, start=1):
        assert np.array_equal(img, scene["kf_pyrs"][e][0])
    host.append(sc.render(CAM, scene["T_root"].reshape(3, 4), seed=41))
    host.append((scene["root_pyr"][0], scene["root_disp"]))
    out = []
    with torch.cuda.stream(stream):
        for img, disp in host:
            out.append(dict(left=torch.as_tensor(np.stack([img, img])).cuda(), disp=torch.as_tensor(np.stack([disp, disp]).astype(np.float32)).cuda()))
    stream.synchronize()
    return dict(kf=out[:n_other], act=out[n_other], cur=out[n_other + 1])


def _off(T, d):
    T = np.array(T, np.float64).reshape(12).copy()
    T[3] += d; T[7] -= 0.5 * d
    return T


def _make_fe(ctx, frames, scene, poses, max_points=1024, stale=0.0):
    """a front end of two streams with the scene's keyframes in slots 0 .. 3 and the active keyframe (the root's id) in slot 4; `poses`: id -> pose for stream 1,
    stream 0 keeps them `stale` metres off"""
    from scavislam_amd.frontend import StereoFrontend
    ids = MM.scene_ids(scene)
    fe = StereoFrontend(ctx, CAM, max_points=max_points, max_keyframes=K, n_streams=2)
    for s, k in enumerate(ids[1:] + [MM.ROOT_ID]):
        fe.processFirstFrames(**(frames["kf"][s] if s < len(ids) - 1 else frames["act"]))
        fe.keepKeyframes(s, np.stack([_off(poses[k], stale), np.asarray(poses[k], np.float64).reshape(12)]))
    return fe


def _step(fe, frames, scene):
    """one frame on both streams -> per stream (svs_frame_result, match records, gate records) as bytes, and n_matched"""
    T_act = np.stack([scene["T_root"].reshape(12)] * 2)
    fe.processFrames(np.stack([np.array(M.I12)] * 2), T_act, **frames["cur"])
    out = []
    for b in range(2):
        res, m, g = fe.results(b)
        out.append((bytes(res), m.tobytes(), g.tobytes(), int(res.n_matched)))
    return out


def _poses(model):
    return {k: model.kf[k]["T"] for k in model.kf}


def _head(scene, n=20):
    """new-point groups as the host would stage them: scene points under other ids with the slots of their anchors"""
    head = np.array(scene["src"][100:100 + n])
    head["kf_index"] -= 1                                   # table entry e lies in slot e - 1
    head["point_id"] = 3000 + np.arange(n)
    return head, [n * 3 // 5, n]


def _request(stream, vertex, slots, head=None, ge=None):
    q = dict(stream=stream, vertex_kf=vertex, slot_kf=slots)
    if head is not None:
        q.update(head=head, head_group_end=ge)
    return q


def _expect(model, q, max_points, vertex_cap=VCAP):
    return NM.build(model, q["vertex_kf"], q["slot_kf"], q.get("head"), q.get("head_group_end"), max_points=max_points, vertex_cap=vertex_cap)


def _check(fe, dmap, model, reqs, refresh=False, vertex_cap=VCAP):
    """the call's outputs against the model -> (outputs, the models' lists)"""
    outs = fe.setCandidatesFromMap(dmap.map, reqs, refresh_poses=refresh, vertex_cap=vertex_cap, want_records=True)
    wants = []
    for o, q in zip(outs, reqs):
        w = _expect(model, q, fe.max_points, vertex_cap)
        wants.append(w)
        got = tuple(o[f] for f in ("n_points", "n_map_points", "n_vertex", "n_no_slot", "over_capacity"))
        print("request", q["vertex_kf"], "->", got)
        assert got == NM.result_fields(w), q["vertex_kf"]
        res, pid, vid, vT = o["raw"]
        if w["over_capacity"]:
            assert (np.frombuffer(pid, np.int32) == -1).all() and (np.frombuffer(vid, np.int32) == -1).all() and not np.frombuffer(vT, np.uint8).any()
            continue
        n, nv = w["n_points"], w["n_vertex"]
        row = o["table"][q["stream"]]
        assert row[:n].tobytes() == w["records"].tobytes(), q["vertex_kf"]
        assert (row[n:].view(np.uint8) == 0xff).all()                                   # "no candidate" behind the list
        assert np.array_equal(np.frombuffer(pid, np.int32), np.concatenate([w["point_ids"], np.full(fe.max_points - n, -1, np.int32)]))
        assert np.array_equal(np.frombuffer(vid, np.int32), np.concatenate([w["vertex_ids"], np.full(vertex_cap - nv, -1, np.int32)]))
        assert vT == np.concatenate([w["vertex_T"], np.zeros((vertex_cap - nv, 12))]).tobytes()
        assert np.array_equal(o["point_ids"], w["point_ids"]) and np.array_equal(o["vertex_ids"], w["vertex_ids"])
    return outs, wants


@pytest.fixture(scope="module")
def list_fe(gpu_ctx, frames, scene, both):
    """a front end for the tests that only build lists"""
    fe = _make_fe(gpu_ctx[0], frames, scene, _poses(both[0]))
    yield fe
    fe.close()


def _vertex_lists(scene):
    ids = MM.scene_ids(scene)
    return [[MM.ROOT_ID, ids[2]], [MM.ROOT_ID], ids, [MM.OFFWALK_ID], [MM.ROOT2_ID]]


# ---- 1. the built list against the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", [False, True])
def test_built_list_equals_the_model(list_fe, both, scene, missing):
    model, dmap = both
    slots = NM.slot_table(scene, missing=(MM.scene_ids(scene)[4],) if missing else ())
    head, ge = _head(scene)
    for i, vertex in enumerate(_vertex_lists(scene)):
        with_head = i % 2 == 0
        outs, wants = _check(list_fe, dmap, model, [_request(i % 2, vertex, slots, head if with_head else None, ge if with_head else None)])
        assert not outs[0]["over_capacity"]
        if i == 0:
            assert (outs[0]["n_no_slot"] > 0) == missing and outs[0]["n_vertex"] == 5
        if vertex == [MM.ROOT2_ID]:
            assert outs[0]["n_map_points"] == 0 and outs[0]["n_points"] == len(head)      # the list is the head alone


# ---- 2. the bitmaps' word and block edges ------------------------------------------------------------------------------------------------------------------------
def test_ids_at_the_edges_of_the_bitmap_words_and_of_the_compaction_block(gpu_ctx, device_scene, list_fe, frames, scene):
    from test_gpu_register_map import DeviceMap
    MAXP, MAXK = 20000, 16384
    kf_ids = [0, 31, 32, MAXK - 1]
    pt_ids = [0, 31, 32, 63, 64, 16383, 16384, 16385, MAXP - 1] + list(range(100, 124))
    rng = np.random.default_rng(3)
    model, dmap = MM.MapModel(), DeviceMap(gpu_ctx[0], device_scene, scene, max_keyframes=MAXK, max_points=MAXP, max_observations=4096)
    try:
        pts = np.array(scene["src"][:len(pt_ids)])
        pts["kf_index"] = [kf_ids[i % 4] for i in range(len(pt_ids))]
        op, ok = [], []
        for i, p in enumerate(pt_ids):
            for k in {kf_ids[i % 4]} | {kf_ids[j] for j in np.nonzero(rng.random(4) < 0.4)[0]}:
                op.append(p); ok.append(k)
        for m in (model, dmap):
            m.add_keyframes(kf_ids, [M.I12] * 4, entry=[1] * 4)
            m.add_points(pt_ids, pts)
            m.add_observations(op, ok)
        slots = [0, 31, MAXK - 1, -1, -1, -1]
        for vertex in ([0], [31], [32], [MAXK - 1], [31, MAXK - 1], [32, 0, 31, MAXK - 1]):
            outs, wants = _check(list_fe, dmap, model, [_request(0, vertex, slots)])
        assert set(pt_ids) == set(int(p) for p in wants[0]["point_ids"]) and wants[0]["n_no_slot"] > 0      # the last list reaches every point
        # a list that ends inside the compaction's second trip (room for 31 of the 33: id 16384 would be the last to fit): counted, over capacity, nothing written
        small = _make_fe(gpu_ctx[0], frames, scene, {k: M.I12 for k in MM.scene_ids(scene)}, max_points=31)
        try:
            outs, wants = _check(small, dmap, model, [_request(0, [32, 0, 31, MAXK - 1], slots)])
            assert wants[0]["over_capacity"] and outs[0]["n_map_points"] == len(pt_ids)
        finally:
            small.close()
    finally:
        dmap.close()


# ---- 3. end to end, and 6. the pose refresh ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_another_slot", [False, True])
def test_a_frame_on_the_list_from_the_map_equals_a_frame_on_the_uploaded_list(gpu_ctx, device_scene, frames, scene, keep_another_slot):
    """stream 0 keeps stale poses and gets list and poses from the map; stream 1 was given the map's poses by keepKeyframes and gets the model's list by
    svs_frontend_set_candidates_all.  keep_another_slot: svs_map_set_poses first, and a keepKeyframes on a free slot behind the refresh, which uploads the whole
    host mirror of the slot table -- a mirror the refresh had not reached would bring the stale poses back"""
    model, dmap, _ = _fill_both(gpu_ctx[0], device_scene, scene)
    fe = None
    try:
        ids = MM.scene_ids(scene)
        if keep_another_slot:
            moved = [ids[2], ids[3]]
            T_moved = [_off(model.kf[k]["T"], 0.002) for k in moved]
            for m in (model, dmap):
                m.set_poses(moved, T_moved)
        slots = NM.slot_table(scene)
        head, ge = _head(scene)
        q = _request(0, [MM.ROOT_ID, ids[2]], slots, head, ge)
        want = _expect(model, q, 1024)
        got = {}
        for refresh in (True, False):
            fe = _make_fe(gpu_ctx[0], frames, scene, _poses(model), stale=0.05)
            fe.setCandidateListsAll([head[:5], want["records"]], [[2, 5, 5], want["group_end"]])
            outs, _ = _check(fe, dmap, model, [q], refresh=refresh)
            assert outs[0]["table"][1][:want["n_points"]].tobytes() == want["records"].tobytes()
            if keep_another_slot:
                fe.keepKeyframes(K - 1, np.stack([scene["T_root"].reshape(12)] * 2))
            got[refresh] = _step(fe, frames, scene)
            fe.close()
            fe = None
        a, b = got[True]
        print("n_matched", a[3], b[3])
        assert a[3] >= 20                          # min_matches: the refinement and the gate really ran
        assert a == b
        assert got[False][1] == b and got[False][0] != a      # the stale poses do matter: without the refresh the streams differ
    finally:
        if fe is not None:
            fe.close()
        dmap.close()


# ---- 4. the tail behind a shorter list -----------------------------------------------------------------------------------------------------------------------------
def test_a_shorter_list_leaves_no_record_of_the_longer_one(gpu_ctx, frames, scene, both):
    model, dmap = both
    ids = MM.scene_ids(scene)
    slots = NM.slot_table(scene)
    head, ge = _head(scene)
    long0, short0, long1 = _request(0, ids, slots, head, ge), _request(0, [MM.ROOT_ID], slots), _request(1, ids, slots, head, ge)
    got = []
    for first in ([long0, long1], [long1]):      # stream 1 keeps the long list: the launches cover stream 0's tail
        fe = _make_fe(gpu_ctx[0], frames, scene, _poses(model))
        try:
            _check(fe, dmap, model, first)
            outs, wants = _check(fe, dmap, model, [short0])
            assert wants[0]["n_points"] < _expect(model, long0, fe.max_points)["n_points"]
            got.append((_step(fe, frames, scene), outs[0]["table"].tobytes()))
        finally:
            fe.close()
    assert got[0] == got[1] and got[0][0][0][3] >= 20


# ---- 5. over capacity ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_request_over_capacity_leaves_its_stream_as_it_was(gpu_ctx, frames, scene, both):
    model, dmap = both
    ids = MM.scene_ids(scene)
    slots = NM.slot_table(scene)
    head, ge = _head(scene)
    big = _request(0, [MM.ROOT_ID, ids[2]], slots, head, ge)
    small = [_request(b, [MM.ROOT_ID], slots) for b in range(2)]
    n = _expect(model, big, 1 << 20)["n_points"]
    got = []
    for refused in (True, False):
        fe = _make_fe(gpu_ctx[0], frames, scene, _poses(model), max_points=n - 1, stale=0.05)
        try:
            _check(fe, dmap, model, [small[0]])
            if refused:      # with a refresh that must not happen either; the other request of the batch is answered
                outs, _ = _check(fe, dmap, model, [big, _request(1, [MM.OFFWALK_ID], slots)], refresh=True)
                assert outs[0]["over_capacity"] == 1 and outs[1]["over_capacity"] == 0 and outs[0]["n_points"] == n
                assert fe.n_points == [_expect(model, small[0], n)["n_points"], 8]
            outs, _ = _check(fe, dmap, model, [small[1]])
            got.append((_step(fe, frames, scene), outs[0]["table"].tobytes()))
        finally:
            fe.close()
    assert got[0] == got[1] and got[0][0][1][3] >= 20
    fe = _make_fe(gpu_ctx[0], frames, scene, _poses(model), max_points=n)
    try:
        outs, _ = _check(fe, dmap, model, [big])      # one more record of capacity: the same request succeeds
        assert outs[0]["over_capacity"] == 0 and outs[0]["n_points"] == n
        outs, _ = _check(fe, dmap, model, [dict(big, stream=1)], vertex_cap=outs[0]["n_vertex"] - 1)
        assert outs[0]["over_capacity"] == 1 and fe.n_points == [n, 0]
    finally:
        fe.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(gpu_ctx, device_scene, frames, scene, both):
    from scavislam_amd import capi
    from scavislam_amd.capi import SvsError
    from scavislam_amd.frontend import StereoFrontend
    from scavislam_amd.register import ResidentMap
    model, dmap = both
    ids = MM.scene_ids(scene)
    slots = NM.slot_table(scene)
    head, ge = _head(scene)
    good = _request(0, [MM.ROOT_ID, ids[2]], slots, head, ge)
    unkept = list(slots); unkept[K - 1] = MM.ALL_ID
    twice = list(slots); twice[0] = twice[1]
    bad_slot = head.copy(); bad_slot["kf_index"][3] = K - 1
    cases = [(INVALID, [good, dict(good, stream=1), dict(good, stream=1)]),                      # more requests than streams
             (INVALID, [good, good]),                                                            # a stream named twice
             (INVALID, [dict(good, stream=2)]),
             (INVALID, [dict(good, vertex_kf=[MM.ROOT_ID, 9])]),                                 # an id that is not in the map
             (INVALID, [dict(good, vertex_kf=[MM.ROOT_ID, ids[2], MM.ROOT_ID])]),                # an id twice in a vertex list
             (INVALID, [dict(good, slot_kf=unkept)]),                                            # a slot that was never kept
             (INVALID, [dict(good, slot_kf=twice)]),                                             # one id in two slots
             (INVALID, [dict(good, head_group_end=[15, 12, 20])]),                               # group ends that descend
             (INVALID, [dict(good, head_group_end=[12, 19])]),                                   # ... that do not end at n_head
             (INVALID, [dict(good, head=bad_slot)]),                                             # kf_index of an unkept slot
             (CAPACITY, [dict(good, head_group_end=[0] * 63 + [20])])]                           # 65 groups
    got = []
    other = capi.Context(0)
    try:
        foreign = ResidentMap(other, max_keyframes=8, max_points=8, max_observations=8)
        for refuse in (True, False):
            fe = _make_fe(gpu_ctx[0], frames, scene, _poses(model), stale=0.05)
            try:
                _check(fe, dmap, model, [dict(good, stream=1)], refresh=True)
                if refuse:
                    for code, reqs in cases:
                        with pytest.raises(SvsError, match=code):
                            fe.setCandidatesFromMap(dmap.map, reqs, refresh_poses=True, vertex_cap=VCAP)
                    with pytest.raises(SvsError, match=INVALID):                                 # fe and map on different contexts
                        fe.setCandidatesFromMap(foreign, [good], vertex_cap=VCAP)
                    assert fe.n_points == [0, _expect(model, good, 1024)["n_points"]]
                got.append(_step(fe, frames, scene))
            finally:
                fe.close()
        foreign.close()
    finally:
        other.close()
    assert got[0] == got[1] and got[0][1][3] >= 20
    # between submit_frame and wait_frame the list of the frame in flight is latched
    ctx = gpu_ctx[0]
    one = StereoFrontend(ctx, CAM, max_points=1024, max_keyframes=K)
    try:
        act, cur = frames["act"], frames["cur"]
        one.processFirstFrame(act["left"][0].cpu().numpy(), disp=act["disp"][0].cpu().numpy())
        one.keepKeyframe(0, scene["T_root"])
        q = _request(0, [MM.ROOT_ID], [MM.ROOT_ID] + [-1] * (K - 1))
        want = _check(one, dmap, model, [q])[1][0]
        one.submitFrame(cur["left"][0].cpu().numpy(), np.array(M.I12), scene["T_root"], disp=cur["disp"][0].cpu().numpy())
        with pytest.raises(SvsError, match=INVALID):
            one.setCandidatesFromMap(dmap.map, [_request(0, [MM.OFFWALK_ID], [MM.ROOT_ID] + [-1] * (K - 1))], vertex_cap=VCAP)
        res, m, g = one.waitFrame()
        assert len(m) == want["n_points"] > 8 and (m["status"] == 1).all()      # the list of before, every anchor without a slot: SVS_MATCH_NO_ANCHOR
    finally:
        one.close()


# ---- 8. invariance -------------------------------------------------------------------------------------------------------------------------------------------------
def test_same_bytes_alone_in_a_batch_repeated_and_on_a_map_built_in_another_order(gpu_ctx, device_scene, list_fe, scene, both):
    from test_gpu_register_map import DeviceMap
    model, dmap = both
    ids = MM.scene_ids(scene)
    slots = NM.slot_table(scene, missing=(ids[3],))
    head, ge = _head(scene)
    q = _request(1, [MM.ROOT_ID, ids[2]], slots, head, ge)
    other = _request(0, ids, NM.slot_table(scene))

    def run(m, reqs, at):
        outs = list_fe.setCandidatesFromMap(m.map, reqs, refresh_poses=True, vertex_cap=VCAP, want_records=True)
        return outs[at]["raw"], outs[at]["table"][1].tobytes()

    alone = run(dmap, [q], 0)
    assert run(dmap, [other, q], 1) == alone
    assert run(dmap, [q], 0) == alone
    # the map again, its updates replayed in another order and split differently
    rng = np.random.default_rng(11)
    second = DeviceMap(gpu_ctx[0], device_scene, scene)
    try:
        kf_ids = sorted(model.kf)
        kf_ids = [kf_ids[i] for i in rng.permutation(len(kf_ids))]
        for chunk in (kf_ids[:3], kf_ids[3:]):
            second.add_keyframes(chunk, [model.kf[k]["T"] for k in chunk], entry=[model.kf[k]["entry"] for k in chunk])
        pt_ids = sorted(model.pt)
        pt_ids = [pt_ids[i] for i in rng.permutation(len(pt_ids))]
        for chunk in (pt_ids[:200], pt_ids[200:]):
            second.add_points(chunk, np.concatenate([model.pt[p].reshape(1) for p in chunk]))
        pairs = sorted(model.obs)
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        a = len(pairs) // 3
        second.add_observations([p for p, _ in pairs[:a]], [k for _, k in pairs[:a]])
        part = run(second, [q], 0)                                                             # a request on a third of the observations, then the rest
        second.add_observations([p for p, _ in pairs[a:] + pairs[:40]], [k for _, k in pairs[a:] + pairs[:40]])
        assert second.info() == dmap.info()
        assert run(second, [q], 0) == alone and part != alone
    finally:
        second.close()


def test_a_staging_block_that_grows_in_mid_life(gpu_ctx, frames, scene, both):
    """one request, then 33 that ask for every optional output, then one again, on ONE front end of 33 streams: the staging block starts at twice the first call's
    need, so the second call outgrows it and the third reuses the bigger one.  Every call against the model, and its outputs and device rows against a fresh front
    end that makes only that call"""
    import torch
    from scavislam_amd.frontend import StereoFrontend
    model, dmap = both
    B, ids = 33, MM.scene_ids(scene)
    poses = _poses(model)

    def wide_fe():
        fe = StereoFrontend(gpu_ctx[0], CAM, max_points=1024, max_keyframes=K, n_streams=B)
        for s, k in enumerate(ids[1:] + [MM.ROOT_ID]):
            with torch.cuda.stream(gpu_ctx[1]):
                fr = {n: t[:1].repeat(B, 1, 1) for n, t in (frames["kf"][s] if s < len(ids) - 1 else frames["act"]).items()}
            fe.processFirstFrames(**fr)
            fe.keepKeyframes(s, np.stack([np.asarray(poses[k], np.float64).reshape(12)] * B))
        return fe

    head, ge = _head(scene)
    lists = _vertex_lists(scene)
    reqs = [_request(b, lists[b % len(lists)], NM.slot_table(scene, missing=(ids[4],) if b % 3 == 0 else ()), head if b % 2 == 0 else None, ge if b % 2 == 0 else None)
            for b in range(B)]
    calls = [[reqs[0]], reqs, [reqs[1]]]
    key = lambda outs, rq: [(o["raw"], o["table"][q["stream"]].tobytes()) for o, q in zip(outs, rq)]
    fe = wide_fe()
    try:
        got = [key(_check(fe, dmap, model, rq, refresh=True)[0], rq) for rq in calls]
        assert got[1][0] == got[0][0] and got[2][0] == got[1][1]
    finally:
        fe.close()
    for rq, g in zip(calls, got):
        fresh = wide_fe() if len(rq) > 1 else _make_fe(gpu_ctx[0], frames, scene, poses)
        try:
            assert key(fresh.setCandidatesFromMap(dmap.map, rq, refresh_poses=True, vertex_cap=VCAP, want_records=True), rq) == g, f"{len(rq)} request(s)"
        finally:
            fresh.close()


# ---- 9. the C++ adaptor --------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_smoke_prints_the_models_counts(gpu_ctx, tmp_path):
    """tests/cpp/neighborhood_smoke.cpp builds a small map of its own (4 keyframes, 40 points, the rule point p is observed by keyframe p % 4 and by its anchor
    (p / 4) % 4) through BackendMap and asks StereoFrontend::setCandidatesFromMap for the list of vertex list {2, 0} with slots {0: 0, 1: 2}"""
    model = MM.MapModel()
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    model.add_keyframes([0, 1, 2, 3], [M.I12] * 4)
    pts = np.zeros(40, CANDIDATE_DTYPE)
    pts["kf_index"] = (np.arange(40) // 4) % 4
    model.add_points(list(range(40)), pts)
    model.add_observations(list(range(40)) * 2, [p % 4 for p in range(40)] + [(p // 4) % 4 for p in range(40)])
    want = NM.build(model, [2, 0], [0, 2])
    exe = tmp_path / "neighborhood_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "neighborhood_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("NEIGHBORHOOD ")]
    assert tok and tok[0].split()[1] == "ok", out
    assert tuple(int(v) for v in tok[0].split()[2:7]) == NM.result_fields(want)
    assert [int(v) for v in tok[0].split()[7:]] == [int(k) for k in want["vertex_ids"]]
