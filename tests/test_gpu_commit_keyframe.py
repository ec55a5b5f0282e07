"""GPU tests of svs_frontend_commit_keyframe: a stream's SVS_KF_DROP decision applied to the resident map in one call, with the lists where the decision left
them on the device.  A batch front end of 3 streams at 160 x 128 (the smallest camera of tests/test_gpu_frame_sizes.py) on big_batch_common's synthetic
streams; stream 2 sees flat frames and is not tracked.  The bar is equality with a twin map fed svs_frontend_decide_keyframes(want_lists = 1)'s downloaded lists
through svs_map_add_keyframe, with the pose from svs_frontend_results and the thresholds read back from the detector: the call's outputs, every read-back of the
map, and what the map stores of the new keyframe (pyramid pointers of the kept slot, disparity, thresholds).  A commit reads the front end only: the next step
of a front end that committed equals the step of one that never did.  Where the reference-built sequence library is present, the 512 x 384 sequence is replayed
up to its third drop and every drop is committed."""
import os

import numpy as np
import pytest

import big_batch_common as BB
import commit_kf_model as CM
import keyframe_model as KM

pytestmark = pytest.mark.gpu
W, H, B = 160, 128, 3
NEW_SLOT = 2
COVIS = 3


def _cam():
    return dict(f=570.342 * W / 640, cx=0.5 * W - 0.3125, cy=0.5 * H + 0.1875, b=0.075, w=W, h=H)


def _ids(b):
    """keyframe ids of stream b's slots 0 / 1 and of its new keyframe"""
    return [100 + 10 * b, 101 + 10 * b], 102 + 10 * b


_S = {}


def _streams():
    if not _S:
        specs = [BB.stream_spec(b, seed=77) for b in range(B)]
        for b, sp in enumerate(specs):
            sp.update(kind="flat" if b == 2 else None, counts=[(200, 100, 40), (200, 100, 40)], length=680, sizes=[0.05] * BB.N_TRACKED)
        cam, S = BB.make_streams(B, specs=specs, cam=_cam())
        for s in S:                                                    # a quarter of the records new points of the active keyframe, a quarter the neighbour's
            s["group_end"] = np.array([170, 340, 680], np.int32)
        _S.update(cam=cam, S=S)
    return _S["cam"], _S["S"]


def _prm(**kw):
    from scavislam_amd.ctypes_types import KeyframeDecideParams
    p = KeyframeDecideParams.reference()
    p.switch_min_shared, p.covis_thr, p.parallax_thr = 1 << 30, COVIS, 0.01      # never a switch; a drop after a centimetre (the streams move about ten)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _vis(s, b):
    """the map of stream b: the track candidates (the records behind the new-point groups) are its points, each seen by its anchor, every second one by both"""
    (id0, id1), _ = _ids(b)
    slot_id = {0: id0, 1: id1}
    n_new = int(s["group_end"][-2])
    vis = {}
    for r in s["pts"][n_new:]:
        a = slot_id[int(r["kf_index"])]
        vis[int(r["point_id"])] = {a, id0, id1} if int(r["point_id"]) % 2 else {a}
    return vis


def _table(s, b):
    (id0, id1), _ = _ids(b)
    vis = _vis(s, b)
    return dict(stream=b, vertex_kf=[id1, id0], vertex_T=[s["T_kf"][1].reshape(12), s["T_kf"][0].reshape(12)],
                sets=[sorted(p for p in vis if id1 in vis[p]), sorted(p for p in vis if id0 in vis[p])], act=0, neighbors=[1], slot_kf=[id0, id1, -1])


class Rig:
    """the front end after one tracked step, and the device frames it was given"""

    def __init__(self, gpu_ctx):
        import torch
        from scavislam_amd import capi
        from scavislam_amd.frontend import StereoFrontend
        self.ctx, self.stream = gpu_ctx
        self.cam, self.S = _streams()
        prm = capi.FrontendParams.reference()
        self.fe = StereoFrontend(self.ctx, self.cam, max_points=BB.MAX_POINTS, max_keyframes=3, params=prm, n_streams=B)
        self.keep = []

        def up(frames):
            with torch.cuda.stream(self.stream):
                left = torch.as_tensor(np.stack([f[0] for f in frames])).cuda()
                disp = torch.as_tensor(np.stack([f[1] for f in frames]).astype(np.float32)).cuda()
            self.stream.synchronize()
            self.keep.append((left, disp))
            return dict(left=left, disp=disp)
        self.up = up
        fe, S = self.fe, self.S
        for j in range(2):
            fe.processFirstFrames(**up([s["kf"][j] for s in S]))
            fe.keepKeyframes(j, np.stack([s["T_kf"][j].reshape(12) for s in S]))
        fe.processFirstFrames(**up([s["first"] for s in S]))
        fe.recomputeCloud(np.stack([s["T_first"].reshape(12) for s in S]))
        fe.setCandidateListsAll([s["pts"] for s in S], [s["group_end"] for s in S])
        fe.setVertexTable([_table(s, b) for b, s in enumerate(S)])
        self.step(0)

    def step(self, k):
        S = self.S
        fr = self.up([s["frames"][k] for s in S])
        self.fe.processFrames(np.stack([s["T_guess"][k].reshape(12) for s in S]), np.stack([s["T_act"].reshape(12) for s in S]), **fr)
        self.disp = [(fr["disp"][b].data_ptr(), W) for b in range(B)]
        self.ctx.sync()

    def outputs(self):
        """every stream's step outputs as bytes"""
        out = []
        for b in range(B):
            res, m, g = self.fe.results(b)
            out.append((bytes(res.T_cur_from_actkey), bytes(res.pose_stats), bytes(res.point_stats), res.n_matched, res.tracking_ok, m.tobytes(), g.tobytes()))
        T, ok = self.fe.poses()
        return out, T.tobytes(), ok.tobytes()

    def thresholds(self, b):
        from scavislam_amd.frontend import fastgrid_for_level
        thr = []
        for l in range(3):
            g = fastgrid_for_level(W >> l, H >> l, l)
            thr.append(self.fe.corners(b, l)[3][:g.gx * g.gy].tolist())
        return thr

    def close(self):
        self.fe.close()


def _new_map(ctx, s, b, blank):
    """the map of one stream in front of the drop"""
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    (id0, id1), _ = _ids(b)
    d = ResidentMap(ctx, max_keyframes=256, max_points=2048, max_observations=1 << 13)
    d.reserve_edges(64)
    kfs = keyframe_table([([blank.data_ptr()] * 3, [16, 16, 16], s["T_kf"][j].reshape(12)) for j in range(2)])
    d.add_keyframes([id0, id1], kfs, [(blank.data_ptr(), 4)] * 2, [[[25], [25], [25]]] * 2)
    vis = _vis(s, b)
    n_new = int(s["group_end"][-2])
    rec = np.array(s["pts"][n_new:], CANDIDATE_DTYPE)
    rec["kf_index"] = [(id0, id1)[int(k)] for k in rec["kf_index"]]
    d.add_points(rec["point_id"], rec)
    pp = [p for p in sorted(vis) for _ in vis[p]]
    kk = [k for p in sorted(vis) for k in sorted(vis[p])]
    d.add_measured_observations(pp, kk, np.ones((len(pp), 3)), np.zeros(len(pp), np.int32))
    return d, sorted(vis)


def _raw(d):
    r = d.raw
    return [r["keys"].tobytes(), r["new_kept"].tobytes(), r["track_exists"].tobytes(), r["results"].tobytes(), r["missing"].tobytes(),
            repr((r["n_keys"], r["m"], r["over_capacity"])).encode()]


@pytest.fixture(scope="module")
def blank(gpu_ctx):
    import torch
    with torch.cuda.stream(gpu_ctx[1]):
        t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    gpu_ctx[0].sync()
    return t


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    r = Rig(gpu_ctx)
    yield r
    r.close()


def _model_decisions(rig, prm):
    """the CPU model on the step's downloaded records"""
    from scavislam_amd.ctypes_types import POINT_STATS_DTYPE
    out = []
    for b, s in enumerate(rig.S):
        res, m, g = rig.fe.results(b)
        stats = np.frombuffer(bytes(res.point_stats), POINT_STATS_DTYPE)[0]
        t = _table(s, b)
        table = dict(kf=t["vertex_kf"], T=t["vertex_T"], sets=t["sets"], act=t["act"], neighbors=t["neighbors"], slot_kf=t["slot_kf"])
        p = {f: getattr(prm, f) for f, _ in prm._fields_ if f != "pad_"}
        out.append((KM.decide(m, s["pts"], g, stats, np.array(res.T_cur_from_actkey), res.tracking_ok, table, p), res))
    return out


def _twin_insert(rig, twin, b, lists, res, blank, **kw):
    from scavislam_amd.register import keyframe_table
    (id0, id1), newkey = _ids(b)
    kf = keyframe_table([([blank.data_ptr()] * 3, [16, 16, 16], KM.I12)])[0]
    return twin.add_keyframe(newkey, id1, np.array(res.T_cur_from_actkey), kf, rig.disp[b], rig.thresholds(b), lists["new"], lists["track"], COVIS, W // 2, H // 2, **kw)


def _commit(rig, d, b, **kw):
    (id0, id1), newkey = _ids(b)
    return rig.fe.commitKeyframe(d, b, NEW_SLOT, newkey, id1, rig.disp[b % B], COVIS, W // 2, H // 2, **kw)


def test_commits_of_two_streams_equal_their_twins_and_refusals_leave_everything_untouched(gpu_ctx, rig, blank):
    from scavislam_amd import capi
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import KF_DROP
    ctx = gpu_ctx[0]
    prm = _prm()
    # ---- the inputs drop, on the CPU model first, with lists that are not empty ---------------------------------------------------------------------------------------
    model = _model_decisions(rig, prm)
    for b in (0, 1):
        d = model[b][0]["dec"]
        print(f"stream {b}: matched {model[b][1].n_matched}, model decision {d['decision']}, n_new {d['n_new']}, n_track {d['n_track']}")
        assert model[b][1].tracking_ok and d["valid"] == 1 and d["decision"] == KF_DROP and d["n_new"] > 0 and d["n_track"] > 0
    assert model[2][0]["dec"]["valid"] == 0                            # the flat stream is not tracked
    maps = [_new_map(ctx, s, b, blank) for b, s in enumerate(rig.S)]
    twins = [_new_map(ctx, s, b, blank) for b, s in enumerate(rig.S)]
    other = capi.Context(ctx.device)
    fe = rig.fe
    try:
        before_fe = rig.outputs()
        before_maps = [CM.map_bytes(d, _ids(b)[0], pts) for b, (d, pts) in enumerate(maps)]

        def refused(b, d=None, **kw):
            with pytest.raises(SvsError) as e:
                _commit(rig, maps[b][0] if d is None else d, b, **kw)
            assert "status 1" in str(e.value), e.value
            assert [CM.map_bytes(d, _ids(k)[0], pts) for k, (d, pts) in enumerate(maps)] == before_maps and rig.outputs() == before_fe

        # every refusal below has ONE deciding condition: all the others are met when it is tried
        refused(0)                                                     # nothing decided yet (with a kept slot and a stale drop: at the end of this test)
        dropped = fe.decideKeyframes(params=prm, want_lists=0)
        assert all(dropped[b]["dec"]["valid"] == 1 and dropped[b]["dec"]["decision"] == KF_DROP for b in (0, 1))
        refused(0)                                                     # a valid drop on this step and this list, the right map -- but the slot was never kept
        refused(1)
        for b in range(B):
            fe.keepKeyframe(NEW_SLOT, KM.I12 if b == 2 else model[b][0]["dec"]["T_newkey_from_w"], stream=b)
        before_fe = rig.outputs()
        dec = fe.decideKeyframes(params=_prm(parallax_thr=1e9, max_av_track_length=1e9, featureless_corners_thr=4), want_lists=0)
        assert dec[0]["dec"]["valid"] == 1 and dec[0]["dec"]["decision"] != KF_DROP
        refused(0)                                                     # the slot kept, a decision on this step: but not a drop
        lists = fe.decideKeyframes(params=prm, want_lists=1)
        for b in (0, 1):
            for f in ("valid", "decision", "n_new", "n_track", "T_newkey_from_w"):
                assert lists[b]["dec"][f].tobytes() == model[b][0]["dec"][f].tobytes(), (b, f)
            assert lists[b]["new"].tobytes() == model[b][0]["new"].tobytes() and lists[b]["track"].tobytes() == model[b][0]["track"].tobytes()
        assert lists[2]["dec"]["valid"] == 0
        refused(2)                                                     # the slot kept: the stream's record is not valid
        refused(3, d=maps[0][0])                                       # no such stream
        with pytest.raises(SvsError):
            fe.commitKeyframe(maps[0][0], 0, 3, _ids(0)[1], _ids(0)[0][1], rig.disp[0], COVIS, W // 2, H // 2)      # no such slot
        foreign = capi_map_of_another_context(other)
        try:
            refused(0, d=foreign)                                      # the map belongs to another context
        finally:
            foreign.close()
        # ---- stream 1, then stream 0, into their own maps -----------------------------------------------------------------------------------------------------------
        raws = {}
        for b in (1, 0):
            (id0, id1), newkey = _ids(b)
            out = _commit(rig, maps[b][0], b)
            raws[b] = _raw(maps[b][0])
            want = _twin_insert(rig, twins[b][0], b, lists[b], model[b][1], blank)
            assert raws[b] == _raw(twins[b][0]) and out["edges"] == want["edges"] and (id1, newkey) in out["edges"]
            pts = sorted(maps[b][1] + [int(p) for p, c in zip(lists[b]["new"]["point_id"], out["new_kept"]) if c])
            got, twin = CM.map_bytes(maps[b][0], [id0, id1, newkey], pts), CM.map_bytes(twins[b][0], [id0, id1, newkey], pts)
            assert got == twin and out["new_kept"].any() and out["track_exists"].any()
            # what the map stores of the new keyframe: the thresholds the detector holds, the disparity, the kept slot's pyramid
            kf, disp, thr = maps[b][0].get_keyframe(newkey)
            assert thr.tobytes() == twins[b][0].get_keyframe(newkey)[2].tobytes() and disp == rig.disp[b]
            assert all(int(v) >= (W >> l) for l, v in enumerate(kf["stride"])) and len({int(p) for p in kf["pyr"]}) == 3 and all(int(p) for p in kf["pyr"])
            assert rig.outputs() == before_fe                          # the front end was only read
        assert maps[0][0].get_keyframe(_ids(0)[1])[0]["pyr"].tolist() != maps[1][0].get_keyframe(_ids(1)[1])[0]["pyr"].tolist()      # each stream its own slot
        with pytest.raises(SvsError) as e:
            _commit(rig, maps[0][0], 0)                                # newkey is a keyframe now
        assert "status 1" in str(e.value)
        # ---- a stream alone gives what it gave behind another stream: stream 0 once more, into a fresh map, with nothing committed in front of it ----------------------
        alone, alone_pts = _new_map(ctx, rig.S[0], 0, blank)
        try:
            fe.decideKeyframes(params=prm, want_lists=0)
            _commit(rig, alone, 0)
            assert _raw(alone) == raws[0]
            (id0, id1), newkey = _ids(0)
            pts = sorted(alone_pts + [int(p) for p, c in zip(lists[0]["new"]["point_id"], alone.raw["new_kept"]) if c])
            assert CM.map_bytes(alone, [id0, id1, newkey], pts) == CM.map_bytes(maps[0][0], [id0, id1, newkey], pts)
        finally:
            alone.close()
        # ---- the clouds re-made since the step: the refined poses a commit would insert are overwritten (for every stream), so it is refused, decided again or not ------
        fe.recomputeCloud(fe.poses()[0])
        alone3, _ = _new_map(ctx, rig.S[1], 1, blank)
        try:
            for again in (False, True):
                if again:
                    assert fe.decideKeyframes(params=prm, want_lists=0)[1]["dec"]["decision"] == KF_DROP
                with pytest.raises(SvsError) as e:
                    _commit(rig, alone3, 1)
                assert "status 1" in str(e.value) and alone3.info()[0] == 2
        finally:
            alone3.close()
        # ---- a candidate list set since the decision: refused; then the next step equals that of a front end that never committed -----------------------------------
        fe.setCandidateListsAll([s["pts"] for s in rig.S], [s["group_end"] for s in rig.S])
        alone2, _ = _new_map(ctx, rig.S[1], 1, blank)
        try:
            with pytest.raises(SvsError) as e:
                _commit(rig, alone2, 1)
            assert "status 1" in str(e.value) and alone2.info()[0] == 2
        finally:
            alone2.close()
        rig.step(1)
        after = rig.outputs()
        plain = Rig(gpu_ctx)
        try:
            for b in range(B):
                plain.fe.keepKeyframe(NEW_SLOT, KM.I12 if b == 2 else model[b][0]["dec"]["T_newkey_from_w"], stream=b)
            # on this front end the list alone decides: a valid drop, the slot kept, the poses the step's -- and a candidate list set since
            assert plain.fe.decideKeyframes(params=prm, want_lists=0)[1]["dec"]["decision"] == KF_DROP
            plain.fe.setCandidateListsAll([s["pts"] for s in rig.S], [s["group_end"] for s in rig.S])
            alone4, _ = _new_map(ctx, rig.S[1], 1, blank)
            try:
                with pytest.raises(SvsError) as e:
                    plain.fe.commitKeyframe(alone4, 1, NEW_SLOT, _ids(1)[1], _ids(1)[0][1], plain.disp[1], COVIS, W // 2, H // 2)
                assert "status 1" in str(e.value) and alone4.info()[0] == 2
            finally:
                alone4.close()
            plain.fe.recomputeCloud(plain.fe.poses()[0])
            plain.step(1)
            assert plain.outputs() == after
        finally:
            plain.close()
        # a step since the decision: stream 1's record is still a drop, its slot is kept, list and poses are the new step's, the map is fresh -- the decision is stale
        alone5, _ = _new_map(ctx, rig.S[1], 1, blank)
        try:
            with pytest.raises(SvsError) as e:
                _commit(rig, alone5, 1)
            assert "status 1" in str(e.value) and alone5.info()[0] == 2
        finally:
            alone5.close()
    finally:
        for d, _ in maps + twins:
            d.close()
        other.close()


def capi_map_of_another_context(other):
    from scavislam_amd.register import ResidentMap
    return ResidentMap(other, max_keyframes=8, max_points=8, max_observations=8)


def _have(name):
    import oracle as O
    return os.path.exists(os.path.join(os.path.dirname(O.__file__), "_ref", name))


def test_every_drop_of_the_sequence_up_to_the_third_is_committed_and_equals_its_twin(gpu_ctx):
    """tests/test_gpu_keyframe_sequence.py's replay of the 512 x 384 sequence, with a map beside it: every drop is committed from the device lists, and the map
    equals a twin fed the downloaded lists after each"""
    if not _have("libsvs_hipbranch_seq_onecall.so"):
        pytest.skip("oracle/_ref/libsvs_hipbranch_seq_onecall.so not present (built by oracle/Makefile where the reference lies; travels prebuilt)")
    import torch
    import oracle as O
    import seq_common as S
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import KF_DROP, KF_SWITCH, KEYFRAME_DTYPE, level_cams
    from scavislam_amd.frontend import StereoFrontend, fastgrid_for_level
    from scavislam_amd.register import ResidentMap
    ctx, stream = gpu_ctx
    MAXK = 32
    cam = S.cam_of("newcollege")
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    seq = O.RefSequence(cams, hip_branch=True, one_call=True)
    frames = S.frames("newcollege", S.N_FRAMES)
    loop, recs, imgs = [], [], []
    drops = 0
    for img, disp in frames:                                            # the reference's loop, one frame past its third drop (that frame names the drop's slot)
        imgs.append((img, disp))
        loop.append(seq.step(img, disp))
        recs.append(seq.onecall_record())
        if drops >= 3:
            break
        drops += int(bool(loop[-1]["dropped"])) if len(loop) > 1 else 0
    seq.close()
    assert drops == 3, "the sequence ended before its third drop"
    with torch.cuda.stream(stream):
        image = torch.zeros(256, dtype=torch.uint8, device="cuda")
        d_disp = [torch.as_tensor(np.ascontiguousarray(d, np.float32)).cuda() for _, d in imgs]
    ctx.sync()
    blank_kf = np.zeros(1, KEYFRAME_DTYPE)
    blank_kf["pyr"], blank_kf["stride"] = image.data_ptr(), 16
    fe = StereoFrontend(ctx, cam, max_points=16384, max_keyframes=MAXK, params=capi.FrontendParams.reference())
    maps = [ResidentMap(ctx, max_keyframes=4096, max_points=1 << 15, max_observations=1 << 16) for _ in range(2)]
    try:
        fe.processFirstFrame(imgs[0][0], disp=imgs[0][1])
        act_id = loop[0]["actkey_id"]
        for d in maps:
            d.reserve_edges(256)
            d.add_first_keyframe(act_id, blank_kf, (image.data_ptr(), 4), [[25], [25], [25]])
        vertices, pending = [], dict(id=act_id, ids=set(), strength=[])
        slot_kf = np.full(MAXK, -1, np.int32)
        kfs, pts, done, kept_ahead = [act_id], [], 0, False
        for k in range(1, len(loop)):
            rc, r = recs[k], loop[k]
            if rc["kept_slot"] >= 0:
                if not kept_ahead:
                    fe.keepKeyframe(rc["kept_slot"], rc["kept_pose"])
                slot_kf[rc["kept_slot"]] = pending["id"]
                vertices.append(dict(pending, T=rc["kept_pose"].copy()))
                pending, kept_ahead = None, False
            if done == 3:
                break
            fe.setCandidateLists(rc["pts"], rc["group_end"])
            res, m, g = fe.processFrame(imgs[k][0], rc["T_guess"], rc["T_act"], disp=imgs[k][1])
            index = {v["id"]: i for i, v in enumerate(vertices)}
            act = index[act_id]
            fe.setVertexTable([dict(stream=0, vertex_kf=[v["id"] for v in vertices], vertex_T=np.stack([v["T"] for v in vertices]),
                                    sets=[sorted(v["ids"]) for v in vertices], act=act, neighbors=[index[i] for i in vertices[act]["strength"]], slot_kf=slot_kf)])
            out = fe.decideKeyframes(want_lists=1)[0]
            d = out["dec"]
            assert (d["decision"] == KF_DROP, d["decision"] == KF_SWITCH) == (r["dropped"], r["switched"]), k
            if r["switched"]:
                act_id = r["actkey_id"]
            if r["dropped"]:
                nxt = recs[k + 1]
                assert nxt["kept_slot"] >= 0
                fe.keepKeyframe(nxt["kept_slot"], nxt["kept_pose"])      # the loop keeps the frame in front of its next step: here in front of the commit
                kept_ahead = True
                newkey = r["actkey_id"]
                disp = (d_disp[k].data_ptr(), cam["w"])
                got = fe.commitKeyframe(maps[0], 0, nxt["kept_slot"], newkey, act_id, disp, 15, cam["w"] // 2, cam["h"] // 2)
                raw = _raw(maps[0])
                thr = []
                for l in range(3):
                    grid = fastgrid_for_level(cam["w"] >> l, cam["h"] >> l, l)
                    thr.append(fe.corners(0, l)[3][:grid.gx * grid.gy].tolist())
                want = maps[1].add_keyframe(newkey, act_id, np.array(res.T_cur_from_actkey), blank_kf, disp, thr, out["new"], out["track"], 15, cam["w"] // 2, cam["h"] // 2)
                assert raw == _raw(maps[1]) and got["edges"] == want["edges"] and not got["over_capacity"]
                kfs.append(newkey)
                pts = sorted(pts + [int(p) for p, c in zip(out["new"]["point_id"], got["new_kept"]) if c])
                assert CM.map_bytes(maps[0], kfs, pts) == CM.map_bytes(maps[1], kfs, pts), f"drop {done}: the maps differ"
                assert maps[0].get_keyframe(newkey)[2].tobytes() == maps[1].get_keyframe(newkey)[2].tobytes()
                print(f"frame {k}: drop {done} committed: {len(out['new'])} new ({int(got['new_kept'].sum())} kept), {len(out['track'])} track entries, edges {got['edges']}")
                pending = dict(id=newkey, ids=set(int(i) for i in out["new"]["point_id"]) | set(int(i) for i in out["track"]["global_id"]),
                               strength=[int(i) for i in d["strength_kf"][:d["n_strength"]]])
                act_id = newkey
                done += 1
            if rc["recloud"]:
                fe.recomputeCloud(rc["recloud_pose"])
        assert done == 3 and len(pts) > 0
    finally:
        fe.close()
        for d in maps:
            d.close()
