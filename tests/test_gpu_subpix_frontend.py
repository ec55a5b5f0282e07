"""The sub-pixel pass inside the front end's step (svs_frontend_set_subpixel; scavislam_amd/csrc/frontend.hip: one launch between the matcher and matchAndTrack's
cut), one stream and a batch of three, CPU build and cuda_build = 1:
  * the records and svs_subpix_info of a step with the option on = tests/subpix_model.py applied to the records of a twin front end with the option off;
  * the refined pose, its statistics, the gate records and the point statistics = svs_motion_only + svs_process_matched_points run stateless on those records;
  * the cut counts the observations left after the refinement;
  * switched off again, a step is the step of a front end that never had the option, and svs_frontend_subpixel_info is refused.
All comparisons are byte for byte.  Frames: the synthetic scene at 320 x 240.

The fused tail (ctx option "fe_fuse_tail": refinement, gate and clouds in one kernel) is taken from 2 * streams >= compute units on, i.e. from 128 streams: not reachable
at these batches.  Both tails read the same records behind the pass; test_option_on_fused_tail_equals_separate_launches runs 128 streams once per tail."""
import functools

import numpy as np
import pytest

import subpix_model as M

pytestmark = pytest.mark.gpu
W, H = 320, 240
I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)


def _cam():
    from scavislam_amd import synth
    return dict(synth.CAM_DEFAULT, w=W, h=H, cx=W / 2.0, cy=H / 2.0, f=285.0)


@functools.lru_cache(maxsize=None)
def _streams(n):
    """n independent streams: keyframe frame a, tracked frames b and c, the keyframe's pose, candidates anchored in a"""
    from scavislam_amd import synth
    out = []
    for b in range(n):
        sc = synth.Scene(2011 + b)
        traj = synth.trajectory(6)
        fa, fb, fc = (sc.render(_cam(), traj[i], seed=10 * b + i) for i in (1, 2, 3))
        pts = synth.candidate_points(np.random.default_rng(4 + b), _cam(), np.maximum(fa[1], 0), traj[1], (150 - 20 * b, 60, 20))
        out.append(dict(a=fa, b=fb, c=fc, T_kf=traj[1].reshape(12), pts=pts))
    return out


class _Run:
    """a front end over the streams S: first frame a (kept as keyframe 0), then steps on demand"""

    def __init__(self, ctx, stream, S, cuda_build=False, num_max_points=300, subpix=None, lists=None, disp_b=None):
        from scavislam_amd import capi
        from scavislam_amd.frontend import StereoFrontend
        self.ctx, self.stream, self.S, self.B = ctx, stream, S, len(S)
        self.disp_b = disp_b
        prm = capi.FrontendParams.reference(cuda_build=cuda_build, num_max_points=num_max_points)
        self.prm = prm
        self.fe = StereoFrontend(ctx, _cam(), max_points=512, max_keyframes=1, params=prm, n_streams=self.B)
        if self.B == 1:
            self.fe.processFirstFrame(S[0]["a"][0], disp=S[0]["a"][1])
            self.fe.keepKeyframe(0, S[0]["T_kf"])
        else:
            self.fe.processFirstFrames(**self._dev("a"))
            self.fe.keepKeyframes(0, np.stack([s["T_kf"] for s in S]))
        for b, s in enumerate(S):
            pts, ge = lists[b] if lists else (s["pts"], [100, len(s["pts"])])
            self.fe.setCandidateLists(pts, ge, stream=b)
        if subpix:
            self.fe.setSubpixel(*subpix)

    def _dev(self, key):
        import torch
        disp = [s[key][1] if key != "b" or self.disp_b is None else self.disp_b[b] for b, s in enumerate(self.S)]
        with torch.cuda.stream(self.stream):
            left = torch.as_tensor(np.stack([s[key][0] for s in self.S])).cuda()
            d = torch.as_tensor(np.stack(disp).astype(np.float32)).cuda()
        self.stream.synchronize()
        self._keep = (left, d)
        return dict(left=left, disp=d)

    def step(self, key):
        """[(FrameResult, matches, gated)] per stream"""
        if self.B == 1:
            disp = self.S[0][key][1] if key != "b" or self.disp_b is None else self.disp_b[0]
            return [self.fe.processFrame(self.S[0][key][0], I34, self.S[0]["T_kf"], disp=disp)]
        self.fe.processFrames(np.stack([I34] * self.B), np.stack([s["T_kf"] for s in self.S]), **self._dev(key))
        return [self.fe.results(b) for b in range(self.B)]

    def close(self):
        self.fe.close()


def _tracked_poses(ctx, stream, S, cuda_build):
    """the dense tracker's pose of step b per stream: a front end with empty candidate lists leaves it untouched"""
    r = _Run(ctx, stream, S, cuda_build, lists=[(s["pts"][:0], [0, 0]) for s in S])
    out = [np.array(x[0].T_cur_from_actkey) for x in r.step("b")]
    r.close()
    return out


def _model(s, m_off, T1, disp, pts, params):
    import oracle as O
    from scavislam_amd.ctypes_types import level_cams
    from scavislam_amd.frontend import _pose_mul
    c = _cam()
    cams = level_cams(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"])
    return M.refine(m_off, pts, [s["T_kf"]], [O.build_pyramid(s["a"][0])], _pose_mul(T1, s["T_kf"]), O.build_pyramid(s["b"][0]), disp, cams, *params)


class _Records:
    """what PoseOptimizer takes for a matcher: the records and candidates of one stream on the device"""

    def __init__(self, stream, m, pts):
        import torch
        with torch.cuda.stream(stream):
            d_res, d_pts = torch.as_tensor(m.view(np.uint8).reshape(-1).copy()).cuda(), torch.as_tensor(np.ascontiguousarray(pts).view(np.uint8).reshape(-1).copy()).cuda()
        self._keep, self._n = (None, d_pts, None, None, d_res), len(m)


@pytest.mark.parametrize("cuda_build", [False, True], ids=["cpu_build", "cuda_build"])
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("params", [(8, 1.5, 0.03), (1, 1.5, 0.03)], ids=["it8", "it1"])
def test_option_on_equals_model_on_the_twin_and_the_stateless_tail(gpu_ctx, n_streams, cuda_build, params):
    from scavislam_amd.ctypes_types import POINT_STATS_DTYPE
    from scavislam_amd.frontend import FramePyramid, PoseOptimizer
    ctx, stream = gpu_ctx
    S = _streams(n_streams)
    T1 = _tracked_poses(ctx, stream, S, cuda_build)
    off, on = _Run(ctx, stream, S, cuda_build), _Run(ctx, stream, S, cuda_build, subpix=params)
    r_off, r_on = off.step("b"), on.step("b")
    infos = [on.fe.subpixelInfo(b) for b in range(len(S))]
    fr = FramePyramid(ctx, stream, _cam(), batch=1, with_float=False)
    n_refined = 0
    for b, s in enumerate(S):
        (res_off, m_off, _), (res_on, m_on, g_on) = r_off[b], r_on[b]
        ok = m_off["status"] == 0
        assert ok.sum() >= 40, (b, np.bincount(m_off["status"]))
        lv = s["pts"]["anchor_level"][ok]
        assert (s["b"][1][m_off["v"][ok] << lv, m_off["u"][ok] << lv] > 0).all()      # no OK record of the matcher sits on a disparity hole: the mirror case cannot occur
        want, want_info = _model(s, m_off, T1[b], s["b"][1], s["pts"], params)
        assert m_on.tobytes() == want.tobytes(), (b, np.flatnonzero(m_on != want)[:5])
        assert infos[b].tobytes() == want_info.tobytes(), (b, np.flatnonzero(infos[b] != want_info)[:5])
        n_refined += int((want_info["state"] == M.REFINED).sum())
        # the tail: stateless calls on the option-on records, from the tracker's pose
        po = PoseOptimizer(ctx, fr)
        rec = _Records(stream, m_on, s["pts"])
        pp = on.prm.pose_opt
        pp.min_obs = on.prm.min_matches or 20
        T, stats = po.calcFastMotionOnly(rec, T1[b], params=pp)
        gated, pstats = po.processMatchedPoints(rec, 100, on.prm.max_reproj_error)
        assert T[0].tobytes() == np.array(res_on.T_cur_from_actkey).tobytes(), (b, "pose")
        assert bytes(stats[0]) == bytes(res_on.pose_stats), (b, "pose statistics")
        assert gated[0].tobytes() == g_on.tobytes(), (b, "gate records")
        assert pstats.view(np.uint8).tobytes()[:POINT_STATS_DTYPE.itemsize] == bytes(res_on.point_stats), (b, "point statistics")
        assert m_on.tobytes() != m_off.tobytes() and np.array(res_on.T_cur_from_actkey).tobytes() != np.array(res_off.T_cur_from_actkey).tobytes()
    assert n_refined >= 10 * len(S), n_refined
    off.close()
    on.close()


def test_cut_counts_observations_after_the_refinement(gpu_ctx):
    """Three lists (the active keyframe's new points, one neighbour's, the neighbourhood's).  Holes are punched into the disparity where refined records of the first
    list read it, and num_max_points is set to twice the first list's observations WITHOUT the option: off, `2 * obs < num_max_points` fails and the neighbour's list
    is SVS_MATCH_SKIPPED; on, the records that became NO_DISP no longer count and the neighbour's list is matched."""
    ctx, stream = gpu_ctx
    S = _streams(1)
    s = S[0]
    params = (8, 1.5, 0.03)
    n = len(s["pts"])
    ge = [n // 2, n // 2 + n // 4, n]
    lists = [(s["pts"], ge)]
    T1 = _tracked_poses(ctx, stream, S, False)[0]
    r = _Run(ctx, stream, S, num_max_points=100000, lists=lists)
    m0 = r.step("b")[0][1]
    r.close()
    _, info0 = _model(s, m0, T1, s["b"][1], s["pts"], params)
    disp = s["b"][1].copy()
    n_holes = 0
    for i in np.flatnonzero((info0["state"] == M.REFINED)[:ge[0]]):
        l = int(s["pts"]["anchor_level"][i])
        iu, iv = int(np.float32(m0["u"][i]) + info0["dx"][i]), int(np.float32(m0["v"][i]) + info0["dy"][i])
        at_match = ((m0["status"] == 0) & ((m0["u"] << s["pts"]["anchor_level"]) == iu << l) & ((m0["v"] << s["pts"]["anchor_level"]) == iv << l)).any()
        if (iu, iv) != (int(m0["u"][i]), int(m0["v"][i])) and not at_match and n_holes < 4:
            disp[iv << l, iu << l] = 0.0
            n_holes += 1
    assert n_holes >= 1
    r = _Run(ctx, stream, S, num_max_points=100000, lists=lists, disp_b=[disp])
    m1 = r.step("b")[0][1]
    r.close()
    assert m1.tobytes() == m0.tobytes()                                        # no hole under a match
    nmp = 2 * int((m1["status"][:ge[0]] == 0).sum())
    off, on = _Run(ctx, stream, S, num_max_points=nmp, lists=lists, disp_b=[disp]), _Run(ctx, stream, S, num_max_points=nmp, lists=lists, disp_b=[disp], subpix=params)
    m_off, m_on = off.step("b")[0][1], on.step("b")[0][1]
    info = on.fe.subpixelInfo(0)
    off.close()
    on.close()
    assert (m_off["status"][ge[0]:ge[1]] == 7).all()                           # SVS_MATCH_SKIPPED
    assert (m_on["status"][ge[0]:ge[1]] != 7).all() and (m_on["status"][ge[0]:ge[1]] == 0).sum() >= 5
    n_nodisp = int((info["state"][:ge[0]] == M.NO_DISP).sum())
    assert n_nodisp >= 1 and (m_on["status"][:ge[0]] == 0).sum() == nmp // 2 - n_nodisp
    want, want_info = _model(s, m1, T1, disp, s["pts"], params)                # the whole list, matched without a cut, through the model
    assert m_on.tobytes() == want.tobytes() and info.tobytes() == want_info.tobytes()


def test_switched_off_again_is_the_never_switched_twin(gpu_ctx):
    from scavislam_amd import capi
    ctx, stream = gpu_ctx
    S = _streams(1)
    twin, fe = _Run(ctx, stream, S), _Run(ctx, stream, S, subpix=(8, 1.5, 0.03))
    a, b = twin.step("b")[0], fe.step("b")[0]
    assert a[1].tobytes() != b[1].tobytes() and len(fe.fe.subpixelInfo(0)) == len(b[1])
    fe.fe.setSubpixel(None)
    with pytest.raises(capi.SvsError):
        fe.fe.subpixelInfo(0)
    for r in (twin, fe):                                                       # the clouds a step leaves are made at its refined pose: the same pose for both
        r.fe.recomputeCloud(np.array(a[0].T_cur_from_actkey))
    a, b = twin.step("c")[0], fe.step("c")[0]
    assert bytes(a[0]) == bytes(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    for l in range(3):
        assert twin.fe.cloud_host(l).tobytes() == fe.fe.cloud_host(l).tobytes()
    with pytest.raises(capi.SvsError):                                         # still off
        fe.fe.subpixelInfo(0)
    with pytest.raises(capi.SvsError):                                         # parameters are refused as svs_match_subpixel refuses them
        fe.fe.setSubpixel(8, 2.5, 0.03)
    twin.close()
    fe.close()


def test_option_on_fused_tail_equals_separate_launches(gpu_ctx):
    """128 streams (2 * streams >= compute units: the fused tail is taken) with the option on, once per tail: every stream's results are the same bytes, and the first
    stream's records are the model's."""
    import big_batch_common as BB
    ctx, stream = gpu_ctx
    B = 128
    assert 2 * B >= BB.n_cu()
    S = [_streams(3)[b % 3] for b in range(B)]
    out = {}
    for fuse in (1, 0):
        ctx.set_option("fe_fuse_tail", fuse)
        try:
            r = _Run(ctx, stream, S, subpix=(8, 1.5, 0.03))
            res = r.step("b")
            out[fuse] = [(bytes(x[0]), x[1].tobytes(), x[2].tobytes()) for x in res] + [r.fe.subpixelInfo(b).tobytes() for b in (0, 1, 2)]
            r.close()
        finally:
            ctx.set_option("fe_fuse_tail", 1)
    assert out[1] == out[0]
    assert out[1][0] != out[1][1]                                              # (streams 0 and 1 differ)
