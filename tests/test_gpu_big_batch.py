"""Big batches of DISTINCT streams (tests/big_batch_common.py) through the path bench.py times: the one-call front end at B > 2 n_cu (flat tracker kernel,
balanced grid order, continuation launch of parked streams, side-stream FAST, cross-frame pipeline), and the tracker at the batch sizes where its launch
changes form.  Every stream is held to the oracle, and a stream's output bits must not depend on the batch it sits in."""
import hashlib

import numpy as np
import pytest

import big_batch_common as BB
from test_gpu_frontend import _check_cpu_sem_trajectory
from test_gpu_ref_frame import _have_ref, _lines

pytestmark = pytest.mark.gpu

TRK_SPLIT = 10            # the context's default "trk_split"
# the tracker's pose against the oracle's, where every LM record is already asserted equal: the two add H,b in another f64 order, which the last solve amplifies
# by the conditioning of H.  1e-9 (test_gpu_frontend.py's scenes) does not hold for every motion: measured 1.3e-9 and 2.6e-9 on ordinary streams (B = n_cu + 1,
# B = 33), 1.9e-9 on a flat one.  A stream without depth is never moved: its pose must be the oracle's exactly
POSE_TOL = {None: 1e-8, "no_depth": 0.0, "flat": 1e-8, "saturated": 1e-8}


def _cams(cam):
    from scavislam_amd.ctypes_types import level_cams
    return level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])


class _Oracle:
    """the oracle's denseTrackingCpu of one stream and frame; pyramids / Sobel images of the shared frames formed once"""

    def __init__(self, cam):
        self.cams, self.pc = _cams(cam), {}

    def prep(self, img):
        import oracle as O
        k = id(img)
        if k not in self.pc:
            p = O.build_pyramid(img)
            self.pc[k] = (img, p, [O.convert_sobel(x) for x in p])      # (img kept alive: its id is the key)
        return self.pc[k][1], self.pc[k][2]

    def clouds(self, disp, T):
        import oracle as O
        return [O.pointcloud_cpu(disp, self.cams[l], l, np.asarray(T).reshape(3, 4)) for l in range(3)]

    def track(self, prev, cur, T_cloud, T_start):
        import oracle as O
        pyr_p, _ = self.prep(prev[0])
        _, fl = self.prep(cur[0])
        return O.dense_tracking_cpu(self.clouds(prev[1], T_cloud), pyr_p, [f[0] for f in fl], [f[1] for f in fl], [f[2] for f in fl], self.cams,
                                    np.asarray(T_start).reshape(3, 4), want_rec=True)


def _check_hostile_trajectory(rec, passes, rec_ref, passes_ref, label):
    """_check_cpu_sem_trajectory for the flat / saturated streams: the same decisions record for record, but their chi2 are sums of ~20 000 nearly equal terms,
    where the reference's serial float sum drifts from the exact sum by more than the 2e-5 that bar allows -- they are held to the rigorous bound of the
    serial sum instead, ((1 + 2^-24)^(n - 1) - 1) < 1.2e-3 for a level-0 sum"""
    ref = rec_ref.copy()
    keep = np.ones(len(ref), bool)
    for k in range(1, len(ref)):
        if ref[k, 1] == 0 and ref[k - 1, 1] == 0 and ref[k, 0] == ref[k - 1, 0]:
            assert ref[k, 2] == ref[k - 1, 2] and ref[k, 3] == ref[k - 1, 3], label
            keep[k] = False
    ref = ref[keep]
    assert passes == len(rec) == len(ref), (label, passes, len(rec), len(ref))
    assert np.array_equal(rec["level"], ref[:, 0].astype(np.int32)) and np.array_equal(rec["accepted"], ref[:, 1].astype(np.int32)), label
    np.testing.assert_allclose(rec["chi2"], ref[:, 2], rtol=1.2e-3, err_msg=label)
    np.testing.assert_allclose(rec["new_chi2"], ref[:, 3], rtol=1.2e-3, err_msg=label)
    assert passes_ref == 3 + 2 * (int((ref[:, 1] < 2).sum()) + int((~keep).sum())), label


def _dedup(rec_ref):
    """the oracle's records without the repeated rejected trials (the device loop records such a trial once)"""
    keep = np.ones(len(rec_ref), bool)
    for k in range(1, len(rec_ref)):
        if rec_ref[k, 1] == 0 and rec_ref[k - 1, 1] == 0 and rec_ref[k, 0] == rec_ref[k - 1, 0]:
            keep[k] = False
    return rec_ref[keep]


def _lvl0_trials(rec):
    return int(((rec["level"] == 0) & (rec["accepted"] < 2)).sum())


def _parked(rec, K=TRK_SPLIT):
    """a stream parks iff it still iterates after K trials on level 0, i.e. iff it takes more than K of them"""
    return _lvl0_trials(rec) > K


def _upload(stream, arrays, dtype):
    import torch
    with torch.cuda.stream(stream):
        t = torch.as_tensor(np.stack(arrays).astype(dtype, copy=False)).to(torch.device("cuda", 0))
    stream.synchronize()
    return t


def _run_frontend(ctx, stream, cam, S, collect, options=None, fresh_fast=()):
    """the streams S through svs_frontend_process_frames: two keyframes, the first frame (its cloud at its pose relative to the active keyframe), BB.N_TRACKED
    tracked frames; collect(fe, k) after tracked frame k.  fresh_fast: streams whose FAST thresholds are reset to 25 before the first tracked frame (a freshly
    initialised FastGrid, as the reference-compiled processFrame sees it)"""
    from scavislam_amd import capi
    from scavislam_amd.frontend import StereoFrontend
    options = options or {}
    for name, v in options.items():
        ctx.set_option(name, v)
    try:
        B = len(S)
        fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=3, params=capi.FrontendParams.reference(), n_streams=B)
        for j in range(2):
            fe.processFirstFrames(left=_upload(stream, [s["kf"][j][0] for s in S], np.uint8), disp=_upload(stream, [s["kf"][j][1] for s in S], np.float32))
            fe.keepKeyframes(j, np.stack([s["T_kf"][j].reshape(12) for s in S]))
        fe.processFirstFrames(left=_upload(stream, [s["first"][0] for s in S], np.uint8), disp=_upload(stream, [s["first"][1] for s in S], np.float32))
        fe.recomputeCloud(np.stack([s["T_first"].reshape(12) for s in S]))
        fe.setCandidateListsAll([s["pts"] for s in S], [s["group_end"] for s in S])
        thr = np.full(64, 25, np.int32)
        for b in fresh_fast:
            for l in range(3):
                ctx.check(ctx.lib.svs_fast_set_thresholds(fe.fast_handle(), b, l, thr.ctypes.data))
        T_act = np.stack([s["T_act"].reshape(12) for s in S])
        out = []
        for k in range(BB.N_TRACKED):
            fe.processFrames(np.stack([s["T_guess"][k].reshape(12) for s in S]), T_act,
                             left=_upload(stream, [s["frames"][k][0] for s in S], np.uint8), disp=_upload(stream, [s["frames"][k][1] for s in S], np.float32))
            out.append(collect(fe, k))
        fe.close()
        return out
    finally:
        for name in options:
            ctx.set_option(name, {"trk_cont_slots": 0, "trk_split": TRK_SPLIT}.get(name, 1))


def _outputs(fe, b):
    """every output of stream b, as bytes per kind"""
    out, m, g = fe.results(b)
    d = dict(frame_result=bytes(out), matches=m.tobytes(), gated=g.tobytes(), dense_records=fe.denseRecords(b).tobytes())
    d["clouds"] = b"".join(fe.cloud_host(l, stream=b).tobytes() for l in range(3))
    d["corners"] = b"".join(x.tobytes() for l in range(3) for x in fe.corners(b, l))
    return d


def _digest(d):
    return {k: hashlib.sha256(v).hexdigest() for k, v in d.items()}


def _against_reference(out, gated, clouds, pts, r, label):
    """tests/test_gpu_ref_frame.py's bar (_check_against_reference_outputs): identical draw lists, refined pose 1e-6, average track length 1e-9, cloud validity
    identical and points 4e-6 -- and the same tracking flag, whatever the number of accepted points (these streams' lists are short: the reference accepts a
    dozen or so of them, below the 40 that test's scenes guarantee)"""
    assert out.tracking_ok == int(r["ok"]), label
    lines = _lines(pts, gated)
    for l in range(3):
        assert lines[l].shape == r["lines"][l].shape and np.array_equal(lines[l], r["lines"][l]), (label, "draw lines", l, lines[l].shape, r["lines"][l].shape)
    n = sum(len(x) for x in lines)
    assert n == out.point_stats.num_track_points, label
    dT = float(np.abs(np.array(out.T_cur_from_actkey).reshape(3, 4) - r["T"]).max())
    assert dT < 1e-6, (label, dT)
    if n:
        assert abs(out.point_stats.sum_track_length / n - r["av_track_length"]) <= 1e-9 * max(r["av_track_length"], 1.0), label
    for l in range(3):
        assert np.array_equal(clouds[l][..., 3], r["clouds"][l][..., 3]), (label, "cloud validity", l)
        np.testing.assert_allclose(clouds[l][..., :3], r["clouds"][l][..., :3], rtol=0, atol=4e-6, err_msg=label)
    return dT


def _decisions_part_at_a_near_tie(rec, rec_ref, label):
    """a later frame's LM run that leaves the oracle's: allowed only as (1) every record before the first different DECISION is the oracle's (level, accept, chi2 to
    2e-5), (2) that decision is on level 0, and (3) the oracle took it on a near-tie: its two float sums within 1e-5 of each other -- the cloud of that frame is
    formed at a refined pose which is the oracle's to ~1e-12 only, and a 15-step level-0 run carries that into its last chi2 digits (measured: 2e-6)"""
    ref = _dedup(rec_ref)
    n = min(len(rec), len(ref))
    same = (rec["level"][:n] == ref[:n, 0]) & (rec["accepted"][:n] == ref[:n, 1])
    i = int(np.argmin(same)) if not same.all() else n
    assert i < n, (label, "the records agree up to the shorter run's end")
    np.testing.assert_allclose(rec["chi2"][:i], ref[:i, 2], rtol=2e-5, err_msg=label)
    np.testing.assert_allclose(rec["new_chi2"][:i], ref[:i, 3], rtol=2e-5, err_msg=label)
    assert ref[i, 0] == 0 and ref[i, 1] < 2 and abs(ref[i, 2] - ref[i, 3]) <= 1e-5 * ref[i, 2], (label, i, rec[i], ref[i])
    return i


def test_big_batch_every_stream_against_the_oracle(gpu_ctx):
    """(a) B = 2 n_cu + 37 distinct streams, default options (balanced order and continuation on), three tracked frames.
    * Every stream and frame: the dense LM record equals the oracle's decision for decision (the tracker starts at the stream's guess, from the cloud the frame
      before left at its refined pose); where tracking failed the front end hands back the tracker's own pose, held to the oracle's.
    * A seeded sample of 64 streams: the cloud each frame leaves equals the oracle's bit for bit; the corner lists of all levels and the persistent FAST thresholds
      equal the oracle's FastGrid, thresholds carried across the frames; and the first tracked frame's WHOLE result -- tracking flag, draw lists (matches, gate), refined pose,
      clouds -- is held to the reference-compiled processFrame at its own bar (tests/test_gpu_ref_frame.py: identical draw lists, pose 1e-6, clouds 4e-6).  The
      sample is taken among the streams with lists of 300 candidates or more and no hostile frames."""
    import oracle as O
    ctx, stream = gpu_ctx
    B = 2 * BB.n_cu() + 37
    cam, S = BB.make_streams(B)
    eligible = [b for b, s in enumerate(S) if s["spec"]["kind"] is None and len(s["pts"]) >= 300]
    sample = set(np.random.default_rng(1).choice(eligible, 64, replace=False).tolist())

    def collect(fe, k):
        res = []
        for b in range(B):
            out, m, g = fe.results(b)
            r = dict(T=np.array(out.T_cur_from_actkey), ok=out.tracking_ok, passes=out.dense_passes, rec=fe.denseRecords(b))
            if b in sample:
                r["clouds"] = [fe.cloud_host(l, stream=b) for l in range(3)]
                r["corners"] = [fe.corners(b, l) for l in range(3)]
                if k == 0:
                    r["full"] = (out, m, g)
            res.append(r)
        return res

    n0 = ctx.get_stat("trk_exact_fallbacks")
    runs = _run_frontend(ctx, stream, cam, S, collect, fresh_fast=sorted(sample))
    assert ctx.get_stat("trk_exact_fallbacks") == n0
    orc = _Oracle(cam)
    n_parked = [0] * BB.N_TRACKED
    drifted = []
    for b, s in enumerate(S):
        prev, T_cloud = s["first"], s["T_first"]
        for k in range(BB.N_TRACKED):
            r = runs[k][b]
            T_ref, passes_ref, rec_ref = orc.track(prev, s["frames"][k], T_cloud, s["T_guess"][k])
            label = f"frame {k}, stream {b} ({s['spec']})"
            assert r["passes"] > 0, label
            if s["spec"]["kind"] in ("flat", "saturated"):
                _check_hostile_trajectory(r["rec"], r["passes"], rec_ref, passes_ref, label)
                if not r["ok"]:
                    np.testing.assert_allclose(r["T"].reshape(3, 4), T_ref, rtol=0, atol=POSE_TOL[s["spec"]["kind"]], err_msg=label)
            elif k > 0 and not (len(r["rec"]) == len(_dedup(rec_ref)) and
                                np.array_equal(r["rec"]["accepted"], _dedup(rec_ref)[:, 1].astype(np.int32)) and np.array_equal(r["rec"]["level"], _dedup(rec_ref)[:, 0].astype(np.int32))):
                drifted.append((b, k, _decisions_part_at_a_near_tie(r["rec"], rec_ref, label)))
            else:
                _check_cpu_sem_trajectory(r["rec"], r["passes"], rec_ref, passes_ref, label)
                if not r["ok"]:
                    np.testing.assert_allclose(r["T"].reshape(3, 4), T_ref, rtol=0, atol=POSE_TOL[s["spec"]["kind"]], err_msg=label)
            n_parked[k] += _parked(r["rec"])
            prev, T_cloud = s["frames"][k], r["T"].reshape(3, 4)
            if b in sample:
                for l, c in enumerate(orc.clouds(prev[1], T_cloud)):
                    assert np.array_equal(r["clouds"][l], c), (label, "cloud", l)
    print(f"{B} distinct streams; LM runs that part from the oracle's at a level-0 near-tie (stream, frame, record): {drifted}; parked per frame "
          f"(K = {TRK_SPLIT}): {n_parked}")
    assert len(drifted) <= 2, drifted
    assert max(n_parked) > 0, "no stream parked: the continuation launch was not exercised"
    # FAST: fresh grids at the first tracked frame (6 trials each frame), thresholds carried
    for b in sorted(sample):
        s = S[b]
        pyrs = [O.build_pyramid(f[0]) for f in s["frames"]]
        grids = [O.fastgrid_for_level(pyrs[0][l].shape[1], pyrs[0][l].shape[0], l) for l in range(3)]
        for k in range(BB.N_TRACKED):
            for l in range(3):
                xy, cc, et = O.fastgrid_detect_adaptively(grids[l], pyrs[k][l], 6)
                gxy, gcc, get, gts = runs[k][b]["corners"][l]
                nc = grids[l].gx * grids[l].gy
                assert np.array_equal(gxy, xy) and np.array_equal(gcc[:nc], cc), (b, k, l)
                assert np.array_equal(gts[:nc], np.array(grids[l].thr[:nc])), (b, k, l, "persistent thresholds")
    # the first tracked frame of the sample against the reference-compiled processFrame
    if not _have_ref("libsvs_ref_frame.so"):
        pytest.skip("oracle/_ref/libsvs_ref_frame.so not present (built where /root/reference exists): everything but the reference-compiled processFrame checked")
    worst = 0.0
    for b in sorted(sample):
        s = S[b]
        pyr_p, _ = orc.prep(s["first"][0])
        pyr_c, fl = orc.prep(s["frames"][0][0])
        r = O.ref_process_frame([O.build_pyramid(kf[0]) for kf in s["kf"]], [T.reshape(12) for T in s["T_kf"]], BB.ACTKEY, [(BB.NEIGHBOUR, 37)], orc.cams,
                                s["pts"], s["list_of"], s["T_guess"][0], orc.clouds(s["first"][1], s["T_first"]), pyr_p, pyr_c,
                                [f[0] for f in fl], [f[1] for f in fl], [f[2] for f in fl], s["frames"][0][1])
        out, m, g = runs[0][b]["full"]
        worst = max(worst, _against_reference(out, g, runs[0][b]["clouds"], s["pts"], r, f"stream {b}"))
    print(f"64 streams of the batch vs the reference-compiled processFrame: draw lists identical, pose deviation {worst:.2e}")


def test_big_batch_stream_bits_do_not_depend_on_the_batch(gpu_ctx):
    """(b) A set S of distinct streams in four batches -- X: B = 2 n_cu + 37 in stream order; Y: S permuted, a quarter of the batch replaced by fillers that park
    (so that the number of parked streams differs from X's by a large factor); Z: B = 4 n_cu with S inside; X again with "trk_cont_slots" = 64 -- must give every
    stream of S the same BYTES in every output: FrameResult, match records, gated points, the three clouds, corners and thresholds, dense LM records.  (B > n_cu:
    the flat tracker in either grid order.  Latency mode and B <= 32 keep their own summation order and are not part of this.)"""
    ctx, stream = gpu_ctx
    ncu = BB.n_cu()
    BX = 2 * ncu + 37
    cam, X = BB.make_streams(BX)
    n_fill = BX // 4
    rng = np.random.default_rng(3)
    keep = np.sort(rng.choice(BX, BX - n_fill, replace=False))               # the streams of S that are in Y
    # fillers: the pair of sequence frames whose LM takes the most level-0 trials (offset 7: 13 trials), with their own guesses and lists
    fill_specs = [dict(BB.stream_spec(10000 + i, seed=1), o=7, kind=None) for i in range(n_fill)]
    _, F = BB.make_streams(0, specs=fill_specs)
    y_order = list(rng.permutation(np.concatenate([keep, -1 - np.arange(n_fill)])))
    Y = [X[i] if i >= 0 else F[-1 - i] for i in y_order]
    z_fill = [BB.stream_spec(20000 + i, seed=2) for i in range(4 * ncu - BX)]
    _, ZF = BB.make_streams(0, specs=z_fill)
    z_pos = np.sort(np.random.default_rng(4).choice(4 * ncu, BX, replace=False))
    Z, zi = [], iter(ZF)
    xi = iter(range(BX))
    pos = set(z_pos.tolist())
    z_of = {}
    for p in range(4 * ncu):
        if p in pos:
            i = next(xi); z_of[i] = p; Z.append(X[i])
        else:
            Z.append(next(zi))

    def collector(index_of):
        def collect(fe, k):
            return {i: _digest(_outputs(fe, p)) for i, p in index_of.items()} | {"parked": sum(_parked(fe.denseRecords(p)) for p in range(fe.n_streams))}
        return collect

    runs = {
        "X": _run_frontend(ctx, stream, cam, X, collector({i: i for i in range(BX)})),
        "Y": _run_frontend(ctx, stream, cam, Y, collector({int(i): p for p, i in enumerate(y_order) if i >= 0})),
        "Z": _run_frontend(ctx, stream, cam, Z, collector(z_of)),
        "X, trk_cont_slots 64": _run_frontend(ctx, stream, cam, X, collector({i: i for i in range(BX)}), {"trk_cont_slots": 64}),
    }
    parked = {n: [r[k]["parked"] for k in range(BB.N_TRACKED)] for n, r in runs.items()}
    print(f"parked streams per frame: {parked}")
    assert all(p > 0 for p in parked["X"]), parked
    assert parked["Y"][0] >= 3 * parked["X"][0], parked           # (the fillers' first pair is the one that parks)
    diffs = {}
    for name in ("Y", "Z", "X, trk_cont_slots 64"):
        for k in range(BB.N_TRACKED):
            for i in runs[name][k]:
                if i == "parked":
                    continue
                a, b = runs["X"][k][i], runs[name][k][i]
                for kind in a:
                    if a[kind] != b[kind]:
                        diffs.setdefault((name, k, kind), []).append(int(i))
    summary = {f"{n} / frame {k} / {kind}": len(v) for (n, k, kind), v in sorted(diffs.items())}
    assert not diffs, f"outputs of S that depend on the batch (streams differing): {summary}"


def _tracker_streams(B, seed):
    """B distinct tracker inputs (previous frame + cloud at the identity, current frame, start pose) out of BB.make_streams"""
    cam, S = BB.make_streams(B, seed=seed)
    return cam, [dict(prev=s["first"], cur=s["frames"][0], T0=s["T_guess_first"], kind=s["spec"]["kind"]) for s in S]


def _track(ctx, stream, cam, T, options=None):
    from scavislam_amd.frontend import DenseTracker, FramePyramid
    B = len(T)
    prev = FramePyramid(ctx, stream, cam, batch=B)
    cur = FramePyramid(ctx, stream, cam, batch=B)
    prev.upload(np.stack([t["prev"][0] for t in T]), np.stack([t["prev"][1] for t in T]))
    cur.upload(np.stack([t["cur"][0] for t in T]), np.stack([t["cur"][1] for t in T]))
    prev.preprocessing(); cur.preprocessing()
    dtp = DenseTracker(ctx, prev)
    dtp.computeDensePointCloudCpu(BB.I34.reshape(12))
    dt = DenseTracker(ctx, cur)
    dt.ref_dense_points = dtp.ref_dense_points
    options = options or {}
    for name, v in options.items():
        ctx.set_option(name, v)
    try:
        n0 = ctx.get_stat("trk_exact_fallbacks")
        Tout, passes = dt.denseTrackingCpu(prev.pyr, np.stack([t["T0"].reshape(12) for t in T]), from_u8=True)
        recs = dt.lm_records()
        assert ctx.get_stat("trk_exact_fallbacks") == n0
    finally:
        for name in options:
            ctx.set_option(name, {"trk_split": TRK_SPLIT}.get(name, 0))
    return Tout, passes, recs


def _check_against_oracle(cam, T, Tout, passes, recs, which, label):
    orc = _Oracle(cam)
    for b in which:
        T_ref, passes_ref, rec_ref = orc.track(T[b]["prev"], T[b]["cur"], BB.I34, T[b]["T0"])
        assert passes[b] > 0, (label, b)
        check = _check_hostile_trajectory if T[b]["kind"] in ("flat", "saturated") else _check_cpu_sem_trajectory
        check(recs[b], passes[b], rec_ref, passes_ref, f"{label}, stream {b}")
        np.testing.assert_allclose(Tout[b], T_ref, rtol=0, atol=POSE_TOL[T[b]["kind"]], err_msg=f"{label}, stream {b}")


def _which(B, seed):
    if B <= 33:
        return list(range(B))
    return sorted({0, B - 1} | set(np.random.default_rng(seed).choice(B, 64, replace=False).tolist()))


@pytest.mark.parametrize("where", ["16", "17", "32", "33", "n_cu", "n_cu+1"])
def test_tracker_path_boundaries_against_the_oracle(gpu_ctx, where):
    """(c) DenseTracker with distinct scenes and motions at batch sizes on both sides of every switch of svs_dense_track_cpu_sem_work: 16 / 17 and 32 / 33
    (workgroups per stream 8 -> 4 -> 1), n_cu / n_cu + 1 (the many-waves build and the flat kernel with its continuation).  Every LM record equals the oracle's,
    pose within POSE_TOL (all streams up to 33, else the first, the last and a seeded 64).  The switch at 2 n_cu (balanced grid order) is the front end's alone --
    the bare tracker has no balance state -- and is crossed by the tests above (B = 2 n_cu + 37) against test_gpu_frontend_batch.py's smaller batches."""
    ctx, stream = gpu_ctx
    ncu = BB.n_cu()
    B = {"n_cu": ncu, "n_cu+1": ncu + 1}.get(where) or int(where)
    cam, T = _tracker_streams(B, seed=B)
    Tout, passes, recs = _track(ctx, stream, cam, T)
    _check_against_oracle(cam, T, Tout, passes, recs, _which(B, B), f"B = {B}")


def test_tracker_continuation_extremes(gpu_ctx):
    """(d) "trk_split" = 1 at B = 4 n_cu: far more streams park than the continuation has groups for, so its groups resume several streams each; and a batch in
    which no stream parks.  Every stream finishes (dense_passes > 0), no exact sum falls back to the chain, records equal the oracle's (first, last, seeded 64
    + every parked stream of the first run)."""
    ctx, stream = gpu_ctx
    ncu = BB.n_cu()
    B = 4 * ncu
    cam, T = _tracker_streams(B, seed=7)
    Tout, passes, recs = _track(ctx, stream, cam, T, {"trk_split": 1})
    assert (passes > 0).all()
    parked = [b for b in range(B) if _parked(recs[b], 1)]
    assert len(parked) > 2 * ncu // 8, f"only {len(parked)} streams parked"
    which = sorted(set(_which(B, 8)) | set(parked[:: max(1, len(parked) // 64)]))
    _check_against_oracle(cam, T, Tout, passes, recs, which, "trk_split 1")
    # no stream parks: distinct streams whose LM, by the oracle, takes at most K - 2 level-0 trials
    orc, T2, b = _Oracle(cam), [], 0
    while len(T2) < 2 * ncu + 5:                      # streams whose oracle LM takes at most K - 2 level-0 trials
        _, (s,) = BB.make_streams(0, specs=[dict(BB.stream_spec(b, seed=9), o=(3, 4, 11, 12)[b % 4])])
        b += 1
        t = dict(prev=s["first"], cur=s["frames"][0], T0=s["T_guess_first"], kind=s["spec"]["kind"])
        rec = orc.track(t["prev"], t["cur"], BB.I34, t["T0"])[2]
        if int(((rec[:, 0] == 0) & (rec[:, 1] < 2)).sum()) <= TRK_SPLIT - 2:
            T2.append(t)
    Tout, passes, recs = _track(ctx, stream, cam, T2)
    assert (passes > 0).all()
    assert not any(_parked(r) for r in recs), [_lvl0_trials(r) for r in recs if _parked(r)]
    _check_against_oracle(cam, T2, Tout, passes, recs, _which(len(T2), 10), "no stream parks")
