"""The front end at frame sizes other than 640 x 480 and 512 x 384, where a level's row pitch (round_up(w, 64)) differs from its width and the quarter-grid
tracker's level-0 sums are longer than the 512 x 40 terms exact_seq_sum_f32 forms in parallel (dense.hip: beyond that it takes the sequential chain):
  160 x 128   pitch 192 / 128 / 64, borders dominate, 1 280 level-0 samples
  272 x 480   taller than wide, pitch != width on every level
  752 x 480   EuRoC: pitch 768 / 384 / 192, 22 560 samples (the chain), 47 quarter-grid columns on level 2
  1232 x 368  pitch 1280 / 640 / 320, 28 336 samples, 23 quarter-grid rows on level 2
(a) the per-frame chain, every stage fed by the previous stage's device output and held to the oracle; (b) every launch form of the tracker at 752 x 480;
(c) caller strides: host rows and device views with padded rows give the same bytes as contiguous frames."""
import numpy as np
import pytest

import big_batch_common as BB
from test_gpu_big_batch import POSE_TOL, _Oracle, _check_hostile_trajectory, _decisions_part_at_a_near_tie, _dedup, _digest, _outputs, _parked, _run_frontend
from test_gpu_frontend import _check_cpu_sem_trajectory

pytestmark = pytest.mark.gpu

SIZES = [(160, 128), (272, 480), (752, 480), (1232, 368)]
SEQ_PAR_MAX = 512 * 40            # level-0 samples up to which exact_seq_sum_f32 forms the float sum in parallel; beyond: the chain
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def cam_of(w, h):
    """intrinsics of a w x h camera: the default camera's field of view (f scaled with w), principal point off the pixel grid"""
    return dict(f=570.342 * w / 640, cx=0.5 * w - 0.3125, cy=0.5 * h + 0.1875, b=0.075, w=w, h=h)


_FRAMES = {}


def frames(w, h):
    """keyframe, previous and current frame of the chain (left, right, true disparity), rendered once per module and size"""
    if (w, h) not in _FRAMES:
        from scavislam_amd import synth
        cam = cam_of(w, h)
        sc = synth.Scene(2011)
        traj = synth.trajectory(8)
        idx = dict(kf=0, prev=4, cur=5)
        _FRAMES[(w, h)] = dict(cam=cam, traj=traj, idx=idx, **{n: synth.render_stereo(sc, cam, traj[i], seed=s + 1) for s, (n, i) in enumerate(idx.items())})
    return _FRAMES[(w, h)]


def _n_samples(cam):
    return (cam["w"] // 4) * (cam["h"] // 4)


def _lvl0_float_trials(rec, rec_ref):
    """level-0 trials whose chi2 pair is the oracle's float pair bit for bit: decided on the exact float sums (_check_cpu_sem_trajectory's count, level 0 only)"""
    ref = _dedup(rec_ref)
    on = (ref[:, 0] == 0) & (ref[:, 1] < 2) & (rec["chi2"].astype(np.float32) == ref[:, 2].astype(np.float32)) & \
         (rec["new_chi2"].astype(np.float32) == ref[:, 3].astype(np.float32))
    return int(on.sum())


@pytest.mark.parametrize("w,h", SIZES)
def test_chain_at_frame_size(gpu_ctx, w, h):
    """calcDisparityCpu -> pyramid / Sobel -> cloud -> denseTrackingCpu (default accept test and trk_seq_chi2) -> FAST (two calls) -> guided matcher (all three
    kernels) -> calcFastMotionOnly -> gate -> next frame's cloud, each against the oracle on the device output of the stage before"""
    import oracle as O
    from scavislam_amd import synth
    from scavislam_amd.frontend import DenseTracker, FastGrid, FramePyramid, GuidedMatcher, PoseOptimizer, StereoMatcher
    ctx, stream = gpu_ctx
    F = frames(w, h)
    cam, traj, idx = F["cam"], F["traj"], F["idx"]
    label = f"{w} x {h}"

    # ---- block matching, then the pyramid (and the Sobel images of the current frame) of every level
    fr, disps, pyr = {}, {}, {}
    for name in ("kf", "prev", "cur"):
        L, R, _ = F[name]
        f = FramePyramid(ctx, stream, cam, batch=1, with_float=(name == "cur"))
        f.upload(L[None])
        sm = StereoMatcher(ctx, f)
        sm.upload_right(R[None])
        sm.calcDisparityCpu()
        d = sm.disparity_host(0)
        sm.close()
        assert np.array_equal(d, O.stereo_bm(L, R)), (label, name, "disparity")
        assert 0.3 < (d > 0).mean() < 1.0, (label, name)
        f.preprocessing()
        fr[name], disps[name], pyr[name] = f, d, O.build_pyramid(L)
        for l in range(3):
            assert np.array_equal(f.level_host(l), pyr[name][l]), (label, name, "pyramid", l)
    cur, prev, kf = fr["cur"], fr["prev"], fr["kf"]
    assert [cur.stride[l] != cur.w[l] for l in range(3)].count(True) >= 2, "a size whose row pitch equals its width on two levels"
    fl = [O.convert_sobel(p) for p in pyr["cur"]]
    for l in range(3):
        wl = cur.w[l]
        for t, ref in zip((cur.f32, cur.dx, cur.dy), fl[l]):
            assert np.array_equal(t[l][0, :, :wl].cpu().numpy(), ref), (label, "Sobel", l)

    # ---- cloud of the previous frame, tracker prev -> cur from the identity
    dtp = DenseTracker(ctx, prev)
    dtp.computeDensePointCloudCpu(I34.reshape(12))
    clouds = [O.pointcloud_cpu(disps["prev"], prev.cams[l], l, I34) for l in range(3)]
    for l in range(3):
        assert np.array_equal(dtp.ref_dense_points[l][0].cpu().numpy(), clouds[l]), (label, "cloud", l)
    dt = DenseTracker(ctx, cur)
    dt.ref_dense_points = dtp.ref_dense_points
    T_ref, passes_ref, rec_ref = O.dense_tracking_cpu(clouds, pyr["prev"], [f[0] for f in fl], [f[1] for f in fl], [f[2] for f in fl], cur.cams, I34, want_rec=True)
    fb0, ex0 = ctx.get_stat("trk_exact_fallbacks"), ctx.get_stat("trk_exact_sums")
    T_gpu, passes = dt.denseTrackingCpu(prev.pyr, I34.reshape(12), from_u8=True)
    rec = dt.lm_records()[0]
    fb, ex = ctx.get_stat("trk_exact_fallbacks") - fb0, ctx.get_stat("trk_exact_sums") - ex0
    n_float = _check_cpu_sem_trajectory(rec, passes[0], rec_ref, passes_ref, f"{label}, default accept test")
    n_float0 = _lvl0_float_trials(rec, rec_ref)
    np.testing.assert_allclose(T_gpu[0], T_ref, rtol=0, atol=1e-8)
    ctx.set_option("trk_seq_chi2", 1)
    try:
        T_seq, passes_seq = dt.denseTrackingCpu(prev.pyr, I34.reshape(12), from_u8=True)
        rec_seq = dt.lm_records()[0]
    finally:
        ctx.set_option("trk_seq_chi2", 0)
    _check_cpu_sem_trajectory(rec_seq, passes_seq[0], rec_ref, passes_ref, f"{label}, trk_seq_chi2")
    np.testing.assert_allclose(T_seq[0], T_ref, rtol=0, atol=1e-8)
    T_true = synth.pose_mul(traj[idx["cur"]], synth.pose_inv(traj[idx["prev"]]))
    assert np.abs(T_gpu[0] - T_true).max() < 0.5 * np.abs(I34 - T_true).max(), label
    # the chain branch of exact_seq_sum_f32 runs inside the tracker exactly where the level-0 sums are longer than its parallel form takes (at the two small
    # sizes the f64 sums decide every trial: their error bound shrinks with the number of terms)
    if _n_samples(cam) > SEQ_PAR_MAX:
        assert ex > 0 and n_float0 > 0 and fb > 0, (label, "the tracker's exact sums never took the chain", ex, n_float0, fb)
    else:
        assert fb == 0, (label, fb)

    # ---- grid FAST on the current frame, two calls (thresholds carry over)
    fast = FastGrid(ctx, cur)
    grids = [O.fastgrid_for_level(cur.w[l], cur.h[l], l) for l in range(3)]
    n_corners = 0
    for it in range(2):
        fast.detectAdaptively(trials=6 if it else 5)
        trees = []
        for l in range(3):
            xy_ref, cc_ref, et_ref = O.fastgrid_detect_adaptively(grids[l], pyr["cur"][l], 6 if it else 5)
            xy, cc, et, ts = fast.corners(0, l)
            assert np.array_equal(xy, xy_ref) and np.array_equal(cc, cc_ref) and np.array_equal(et, et_ref), (label, it, l)
            trees.append(O.quadtree_from_corners(xy_ref, cc_ref, cur.w[l], cur.h[l]))
            n_corners += len(xy)

    # ---- guided matcher against the keyframe, all three kernels (the default one last: motion-only and the gate read its device-resident records)
    rng = np.random.default_rng(7)
    pts = synth.candidate_points(rng, cam, np.maximum(disps["kf"], 0), traj[idx["kf"]], (500, 250, 80))
    T_cur_kf_true = synth.pose_mul(traj[idx["cur"]], synth.pose_inv(traj[idx["kf"]]))
    T_guess = synth.pose_mul(synth.pose(synth.so3_exp(np.array([0.001, -0.002, 0.0005])), np.array([0.005, 0.0, -0.005])), T_cur_kf_true)
    ref = O.match([pyr["kf"]], [traj[idx["kf"]].reshape(12)], T_guess, traj[idx["kf"]], pyr["cur"], disps["cur"], trees, cur.cams, pts)
    ok = ref["status"] == 0
    m = GuidedMatcher(ctx, cur, fast)
    for legacy in (1, 2, 0):
        ctx.set_option("match_legacy", legacy)
        try:
            res = m.match([(kf.pyr, 0, traj[idx["kf"]].reshape(12))], T_guess.reshape(12), traj[idx["kf"]].reshape(12), pts)[0]
        finally:
            ctx.set_option("match_legacy", 0)
        for k in ("status", "u", "v", "znssd"):
            assert np.array_equal(res[k], ref[k]), (label, legacy, k)
        assert np.array_equal(res["obs"][ok], ref["obs"][ok]) and np.array_equal(res["xyz_actkey"][ok], ref["xyz_actkey"][ok]), (label, legacy)
    assert ok.sum() >= 20, (label, int(ok.sum()))

    # ---- calcFastMotionOnly + processMatchedPoints on the device-resident track data
    po = PoseOptimizer(ctx, cur)
    T_mo, st = po.calcFastMotionOnly(m, T_guess.reshape(12))
    T_mo_ref, st_ref = O.motion_only(res, cur.cams[0], T_guess)
    np.testing.assert_allclose(T_mo[0], T_mo_ref, rtol=0, atol=1e-9)
    assert st[0].num_obs == st_ref.num_obs == int(ok.sum()), label
    gated, pstats = po.processMatchedPoints(m, n_new_records=500)
    g_ref, s_ref = O.process_matched_points(res, pts, 500, cur.cams[0], T_mo[0])
    for k in ("accepted", "is_new", "uv_pyr", "curkey_uv_pyr"):
        assert np.array_equal(gated[0][k], g_ref[k]), (label, k)
    for k in ("num_points_grid2x2", "num_points_grid3x3", "num_matched_points", "num_track_points", "num_obs"):
        assert np.array_equal(pstats[0][k], s_ref[k]), (label, k)
    assert pstats[0]["num_track_points"] > 0, label

    # ---- the next frame's cloud at the tracked pose
    dt.computeDensePointCloudCpu(T_gpu[0].reshape(12))
    for l in range(3):
        assert np.array_equal(dt.ref_dense_points[l][0].cpu().numpy(), O.pointcloud_cpu(disps["cur"], cur.cams[l], l, T_gpu[0])), (label, "next cloud", l)
    print(f"{label}: {_n_samples(cam)} level-0 samples; {len(rec)} LM records x 2 modes equal to the oracle's ({n_float} trials on the float sums, "
          f"{n_float0} of them on level 0); {ex} exact sums, {fb} by the chain; {n_corners} corners; {len(pts)} candidates x 3 kernels, {int(ok.sum())} matches, "
          f"{int(pstats[0]['num_track_points'])} gated")


# ---- (b) the tracker's launch forms at 752 x 480 ---------------------------------------------------------------------------------------------------------
W_B, H_B = 752, 480
_TRK = {}


def _tracker_streams():
    """40 distinct tracker inputs at 752 x 480 (previous frame + cloud at the identity, current frame, start pose) and the oracle's run of each, once per module"""
    if "T" not in _TRK:
        cam = cam_of(W_B, H_B)
        _, S = BB.make_streams(40, seed=31, cam=cam)
        T = [dict(prev=s["first"], cur=s["frames"][0], T0=s["T_guess_first"], kind=s["spec"]["kind"]) for s in S]
        orc = _Oracle(cam)
        _TRK.update(cam=cam, T=T, ref=[orc.track(t["prev"], t["cur"], I34, t["T0"]) for t in T])
    return _TRK["cam"], _TRK["T"], _TRK["ref"]


@pytest.mark.parametrize("form", ["B=1", "trk_nwg=2", "trk_nwg=16", "B=24", "B=40"])
def test_tracker_launch_forms_752x480(gpu_ctx, form):
    """latency mode (B = 1: eight workgroups per stream; four streams with "trk_nwg" 2 and 16), four workgroups per stream (B = 24) and one (B = 40), every stream's
    LM records against the oracle's, pose within POSE_TOL; the level-0 sums (22 560 terms) take exact_seq_sum_f32's chain: the fallback count rises"""
    from scavislam_amd.frontend import DenseTracker, FramePyramid
    ctx, stream = gpu_ctx
    cam, T_all, refs = _tracker_streams()
    B, nwg = {"B=1": (1, 0), "trk_nwg=2": (4, 2), "trk_nwg=16": (4, 16), "B=24": (24, 0), "B=40": (40, 0)}[form]
    T = T_all[:B]
    prev = FramePyramid(ctx, stream, cam, batch=B)
    cur = FramePyramid(ctx, stream, cam, batch=B)
    prev.upload(np.stack([t["prev"][0] for t in T]), np.stack([t["prev"][1] for t in T]))
    cur.upload(np.stack([t["cur"][0] for t in T]), np.stack([t["cur"][1] for t in T]))
    prev.preprocessing(); cur.preprocessing()
    dtp = DenseTracker(ctx, prev)
    dtp.computeDensePointCloudCpu(I34.reshape(12))
    dt = DenseTracker(ctx, cur)
    dt.ref_dense_points = dtp.ref_dense_points
    ctx.set_option("trk_nwg", nwg)
    try:
        fb0 = ctx.get_stat("trk_exact_fallbacks")
        Tout, passes = dt.denseTrackingCpu(prev.pyr, np.stack([t["T0"].reshape(12) for t in T]), from_u8=True)
        recs = dt.lm_records()
        fb = ctx.get_stat("trk_exact_fallbacks") - fb0
    finally:
        ctx.set_option("trk_nwg", 0)
    n_rec = n_float0 = 0
    for b in range(B):
        T_ref, passes_ref, rec_ref = refs[b]
        lab = f"{form}, stream {b} ({T[b]['kind']})"
        assert passes[b] > 0, lab
        check = _check_hostile_trajectory if T[b]["kind"] in ("flat", "saturated") else _check_cpu_sem_trajectory
        check(recs[b], passes[b], rec_ref, passes_ref, lab)
        np.testing.assert_allclose(Tout[b], T_ref, rtol=0, atol=POSE_TOL[T[b]["kind"]], err_msg=lab)
        n_rec += len(recs[b])
        n_float0 += _lvl0_float_trials(recs[b], rec_ref) if check is _check_cpu_sem_trajectory else 0
    assert n_float0 > 0 and fb > 0, (form, "exact float sums on level 0 / by the chain", n_float0, fb)
    print(f"752 x 480, {form}: {B} streams, {n_rec} LM records equal to the oracle's; {n_float0} level-0 trials on the float sums, {fb} workgroups took the chain")


def test_big_batch_752x480(gpu_ctx):
    """B = 2 n_cu + 1 streams through svs_frontend_process_frames (balanced order, flat tracker, continuation launch with "trk_split" = 2, side-stream FAST), dealt
    round-robin from 17 distinct inputs so that neighbouring slots differ: each input's LM records of three tracked frames against the oracle, every replica of an
    input the same BYTES in every output; the same inputs dealt into a batch of another size and order, and with "trk_cont_slots" = 64, give the same bytes again"""
    ctx, stream = gpu_ctx
    cam = cam_of(W_B, H_B)
    ncu = BB.n_cu()
    ND = 17
    _, D = BB.make_streams(ND, seed=37, cam=cam)
    BX = 2 * ncu + 1
    X = [D[b % ND] for b in range(BX)]
    BY = 2 * ncu + 37
    y_of = np.random.default_rng(5).permutation(BY) % ND
    Y = [D[i] for i in y_of]

    def collect(fe, k):
        from scavislam_amd import capi
        from scavislam_amd.ctypes_types import DENSE_LM_RECORD_DTYPE
        out = {}
        for b in range(fe.n_streams):
            o = _outputs(fe, b)
            out[b] = dict(dig=_digest(o), rec=np.frombuffer(o["dense_records"], DENSE_LM_RECORD_DTYPE), res=capi.FrameResult.from_buffer_copy(o["frame_result"]))
        out["parked"] = sum(_parked(out[b]["rec"], 2) for b in range(fe.n_streams))
        return out

    fb0 = ctx.get_stat("trk_exact_fallbacks")
    runs = {"X": _run_frontend(ctx, stream, cam, X, collect, {"trk_split": 2})}
    fb = ctx.get_stat("trk_exact_fallbacks") - fb0
    runs["Y"] = _run_frontend(ctx, stream, cam, Y, collect, {"trk_split": 2})
    runs["X, trk_cont_slots 64"] = _run_frontend(ctx, stream, cam, X, collect, {"trk_split": 2, "trk_cont_slots": 64})
    parked = {n: [r[k]["parked"] for k in range(BB.N_TRACKED)] for n, r in runs.items()}
    assert all(p > 0 for p in parked["X"]), parked
    assert fb > 0, "the flat / continuation tracker never took exact_seq_sum_f32's chain"
    # every replica of an input, in every batch, the bytes of its first slot in X
    diffs = {}
    for name, r in runs.items():
        of = (lambda b: b % ND) if name != "Y" else (lambda b: int(y_of[b]))
        for k in range(BB.N_TRACKED):
            for b in range(len(r[k]) - 1):
                a = runs["X"][k][of(b)]["dig"]
                for kind, v in r[k][b]["dig"].items():
                    if v != a[kind]:
                        diffs.setdefault((name, k, kind), []).append(b)
    assert not diffs, f"outputs that depend on the slot or the batch: { {f'{n} / frame {k} / {kind}': len(v) for (n, k, kind), v in sorted(diffs.items())} }"
    # each input against the oracle, frame by frame (the cloud of a later frame formed at the pose the front end refined)
    orc = _Oracle(cam)
    n_rec, drifted = 0, []
    for i, s in enumerate(D):
        prev_f, T_cloud = s["first"], s["T_first"]
        for k in range(BB.N_TRACKED):
            r = runs["X"][k][i]
            T_ref, passes_ref, rec_ref = orc.track(prev_f, s["frames"][k], T_cloud, s["T_guess"][k])
            lab = f"frame {k}, input {i} ({s['spec']['kind']})"
            rec, res = r["rec"], r["res"]
            assert res.dense_passes > 0, lab
            ref = _dedup(rec_ref)
            T_out = np.array(res.T_cur_from_actkey).reshape(3, 4)
            if s["spec"]["kind"] in ("flat", "saturated"):
                _check_hostile_trajectory(rec, res.dense_passes, rec_ref, passes_ref, lab)
                if not res.tracking_ok:
                    np.testing.assert_allclose(T_out, T_ref, rtol=0, atol=POSE_TOL[s["spec"]["kind"]], err_msg=lab)
            elif k > 0 and not (len(rec) == len(ref) and np.array_equal(rec["accepted"], ref[:, 1].astype(np.int32))
                                and np.array_equal(rec["level"], ref[:, 0].astype(np.int32))):
                drifted.append((i, k, _decisions_part_at_a_near_tie(rec, rec_ref, lab)))
            else:
                _check_cpu_sem_trajectory(rec, res.dense_passes, rec_ref, passes_ref, lab)
                if not res.tracking_ok:
                    np.testing.assert_allclose(T_out, T_ref, rtol=0, atol=POSE_TOL[s["spec"]["kind"]], err_msg=lab)
            n_rec += len(rec)
            prev_f, T_cloud = s["frames"][k], T_out
    assert len(drifted) <= 1, drifted
    print(f"752 x 480 big batch: B = {BX} / {BY}, {ND} inputs x {BB.N_TRACKED} frames, {n_rec} LM records compared with the oracle; parked per frame {parked}; "
          f"{fb} workgroups took the chain; runs that part at a level-0 near-tie (input, frame, record): {drifted}; every replica byte-equal")


# ---- (c) caller strides ----------------------------------------------------------------------------------------------------------------------------------
def _padded_host(a, extra, fill):
    """a [h, w] view into a buffer whose rows are `extra` elements longer, the padding filled with `fill`"""
    buf = np.full((a.shape[0], a.shape[1] + extra), fill, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]]


def _staged(ctx, stream, F, pts, T_guess, block_matching):
    """tests/test_gpu_process_frame.py's stages one by one: (FrameResult fields, matches, gated, per-point stats, clouds)"""
    from scavislam_amd.frontend import DenseTracker, FastGrid, FramePyramid, GuidedMatcher, PoseOptimizer, StereoMatcher
    cam, traj, idx = F["cam"], F["traj"], F["idx"]
    fr = {}
    for name in ("kf", "prev", "cur"):
        L, R, d_true = F[name]
        f = FramePyramid(ctx, stream, cam, batch=1, with_float=False)
        if block_matching:
            f.upload(L[None])
            sm = StereoMatcher(ctx, f)
            sm.upload_right(R[None])
            sm.calcDisparityCpu()
            ctx.sync()
            sm.close()
        else:
            f.upload(L[None], d_true[None])
        f.preprocessing(with_float=False)
        fr[name] = f
    kf, prev, cur = fr["kf"], fr["prev"], fr["cur"]
    fast = FastGrid(ctx, cur)
    fast.detectAdaptively(pyr=kf.pyr, trials=5)
    fast.detectAdaptively(pyr=prev.pyr, trials=5)
    dtp = DenseTracker(ctx, prev)
    dtp.computeDensePointCloudCpu(I34.reshape(12))
    dt = DenseTracker(ctx, cur)
    dt.ref_dense_points = dtp.ref_dense_points
    T_trk, passes = dt.denseTrackingCpu(prev.pyr, T_guess.reshape(12), from_u8=True)
    fast.detectAdaptively(trials=6)
    m = GuidedMatcher(ctx, cur, fast)
    res = m.match([(kf.pyr, 0, traj[idx["kf"]].reshape(12))], T_trk[0].reshape(12), traj[idx["prev"]].reshape(12), pts)[0]
    po = PoseOptimizer(ctx, cur)
    T_mo, st = po.calcFastMotionOnly(m, T_trk[0].reshape(12))
    gated, pstats = po.processMatchedPoints(m, n_new_records=len(pts) // 2)
    dt.computeDensePointCloudCpu(T_mo[0].reshape(12))
    ctx.sync()
    clouds = [dt.ref_dense_points[l][0].cpu().numpy() for l in range(3)]
    return dict(passes=int(passes[0]), T=T_mo[0], st=st[0], res=res, gated=gated[0], pstats=pstats[0], clouds=clouds)


def _candidates(F):
    from scavislam_amd import synth
    return synth.candidate_points(np.random.default_rng(7), F["cam"], np.maximum(F["kf"][2], 0), F["traj"][F["idx"]["kf"]], (300, 150, 50))


def _guess(F):
    from scavislam_amd import synth
    traj, idx = F["traj"], F["idx"]
    return synth.pose_mul(synth.pose(synth.so3_exp(np.array([0.001, -0.002, 0.0005])), np.array([0.004, 0.0, -0.004])),
                          synth.pose_mul(traj[idx["cur"]], synth.pose_inv(traj[idx["prev"]])))


def _one_call(ctx, F, pts, T_guess, block_matching, pad):
    """svs_frontend_process_frame over kf, prev, cur; pad: host rows 7 bytes (u8) / 5 floats (disparity) longer than w, padding 255 / 1e30 / NaN"""
    from scavislam_amd import capi
    from scavislam_amd.frontend import StereoFrontend
    traj, idx = F["traj"], F["idx"]
    fe = StereoFrontend(ctx, F["cam"], max_points=1024, max_keyframes=2, params=capi.FrontendParams.reference(use_block_matching=block_matching))
    def imgs(name):
        L, R, d = F[name]
        if pad:
            L, R, d = _padded_host(L, 7, 255), _padded_host(R, 7, 0), _padded_host(d, 5, np.nan if name == "cur" else 1e30)
        return L, (dict(right=R) if block_matching else dict(disp=d))

    L, kw = imgs("kf")
    fe.processFirstFrame(L, strided=pad, **kw)
    fe.keepKeyframe(0, traj[idx["kf"]])
    L, kw = imgs("prev")
    fe.processFirstFrame(L, strided=pad, **kw)
    fe.setCandidates(pts, len(pts) // 2)
    L, kw = imgs("cur")
    out, m, g = fe.processFrame(L, T_guess, traj[idx["prev"]], strided=pad, **kw)
    clouds = [fe.cloud_host(l) for l in range(3)]
    rec = fe.denseRecords()
    fe.close()
    return out, m, g, clouds, rec


@pytest.mark.parametrize("block_matching", [False, True])
@pytest.mark.parametrize("w,h", [(752, 480), (160, 128)])
def test_host_row_strides(gpu_ctx, w, h, block_matching):
    """svs_frontend_process_frame with host rows longer than w (an odd number of extra bytes for u8, extra floats for the disparity, padding that would change
    any result) gives the bytes of the contiguous call, and those are the bytes of the stages run one by one"""
    ctx, stream = gpu_ctx
    F = frames(w, h)
    pts, T_guess = _candidates(F), _guess(F)
    base = _one_call(ctx, F, pts, T_guess, block_matching, pad=False)
    padded = _one_call(ctx, F, pts, T_guess, block_matching, pad=True)
    out, m, g, clouds, rec = base
    assert bytes(padded[0]) == bytes(out), "FrameResult"
    assert padded[1].tobytes() == m.tobytes() and padded[2].tobytes() == g.tobytes(), "match records / gated points"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(padded[3], clouds)), "clouds"
    assert padded[4].tobytes() == rec.tobytes(), "dense LM records"
    s = _staged(ctx, stream, F, pts, T_guess, block_matching)
    ok = s["res"]["status"] == 0
    assert out.dense_passes == s["passes"] and out.n_points == len(pts)
    assert np.array_equal(np.array(out.T_cur_from_actkey).reshape(3, 4), s["T"])
    for k in ("status", "u", "v", "znssd", "obs", "xyz_actkey"):
        assert np.array_equal(m[k], s["res"][k]), k
    assert out.n_matched == int(ok.sum()) == s["st"].num_obs
    for k in ("accepted", "is_new", "uv_pyr", "curkey_uv_pyr"):
        assert np.array_equal(g[k][ok], s["gated"][k][ok]), k
    for k in ("num_points_grid2x2", "num_points_grid3x3", "num_matched_points"):
        assert np.array_equal(np.array(getattr(out.point_stats, k)), s["pstats"][k]), k
    assert out.point_stats.num_track_points == s["pstats"]["num_track_points"] and out.point_stats.num_obs == s["pstats"]["num_obs"]
    assert out.pose_stats.chi2 == s["st"].chi2 and out.pose_stats.initial_chi2 == s["st"].initial_chi2
    for l in range(3):
        assert np.array_equal(clouds[l], s["clouds"][l]), f"cloud level {l}"
    assert ok.sum() > 0
    print(f"{w} x {h}, block matching {block_matching}: padded host rows = contiguous = staged chain; {len(rec)} LM records, {len(pts)} match records, "
          f"{int(ok.sum())} matches, {out.point_stats.num_track_points} gated points")


def _device_run(ctx, stream, F, pts, T_guess, block_matching, pad):
    """svs_frontend_process_frames, two streams, frames as device views: contiguous [B][h][w], or (pad) rows 64 bytes / 16 floats longer than w and 3 extra rows
    between streams, padding 255 / 1e30 / NaN"""
    import torch
    from scavislam_amd import capi
    from scavislam_amd.frontend import StereoFrontend
    cam, traj, idx = F["cam"], F["traj"], F["idx"]
    w, h = cam["w"], cam["h"]
    order = [("kf", "prev", "cur"), ("kf", "cur", "prev")]           # two streams of the cached frames; the second one tracks backwards
    B = len(order)
    fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2, params=capi.FrontendParams.reference(use_block_matching=block_matching), n_streams=B)

    def dev(arrs, dtype, extra, fill):
        a = np.stack(arrs).astype(dtype, copy=False)
        with torch.cuda.stream(stream):
            if not pad:
                t = torch.as_tensor(a).cuda()
            else:
                buf = torch.full((B, h + 3, w + extra), fill, dtype=torch.uint8 if dtype == np.uint8 else torch.float32, device="cuda")
                buf[:, :h, :w] = torch.as_tensor(a).cuda()
                t = buf[:, :h, :w]
        stream.synchronize()
        return t

    def frames_of(j):
        names = [o[j] for o in order]
        L = dev([F[n][0] for n in names], np.uint8, 64, 255)
        if block_matching:
            return dict(left=L, right=dev([F[n][1] for n in names], np.uint8, 64, 0))
        return dict(left=L, disp=dev([F[n][2] for n in names], np.float32, 16, float("nan") if j == 2 else 1e30))

    fe.processFirstFrames(**frames_of(0))
    fe.keepKeyframes(0, np.stack([traj[idx["kf"]].reshape(12)] * B))
    fe.processFirstFrames(**frames_of(1))
    fe.setCandidateListsAll([pts] * B, [[len(pts) // 2, len(pts)]] * B)
    T_act = np.stack([traj[idx[o[1]]].reshape(12) for o in order])
    fe.processFrames(np.stack([T_guess.reshape(12), np.linalg.inv(np.vstack([T_guess, [0, 0, 0, 1]]))[:3].reshape(12)]), T_act, **frames_of(2))
    out = [_outputs(fe, b) for b in range(B)]
    T, ok = fe.poses()
    fe.close()
    return out, T.tobytes() + ok.tobytes()


@pytest.mark.parametrize("block_matching", [False, True])
@pytest.mark.parametrize("w,h", [(752, 480), (160, 128)])
def test_device_frame_strides(gpu_ctx, w, h, block_matching):
    """svs_frontend_process_frames with device views whose rows are padded (lstride % 4 == 0, > w) and with extra rows between streams (l_bstride > h lstride):
    every output of every stream the bytes of the contiguous call"""
    ctx, stream = gpu_ctx
    F = frames(w, h)
    pts, T_guess = _candidates(F), _guess(F)
    base, poses = _device_run(ctx, stream, F, pts, T_guess, block_matching, pad=False)
    padded, poses_p = _device_run(ctx, stream, F, pts, T_guess, block_matching, pad=True)
    assert poses_p == poses, "poses"
    for b in range(len(base)):
        for kind in base[b]:
            assert padded[b][kind] == base[b][kind], (b, kind)
    print(f"{w} x {h}, block matching {block_matching}: {len(base)} streams from padded device views = contiguous (FrameResult, {len(pts)} match records and "
          f"gated points per stream, clouds, corners, LM records, poses)")
