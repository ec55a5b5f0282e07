"""The dense tracker's sweep after its instruction diet (profiles/tracker_sweep.md): an invalid sample is SKIPPED under one `if (ok)` instead of added as
zeros, a prefetch past the level's end reads the level's first sample instead of constants, and the sample loop runs two trips per iteration on two register
sets with one more trip behind it for an odd count.  No floating-point expression changed, so every LM record must stay the oracle's and the launch forms
that were bit-equal stay bit-equal.

Sizes (512 lanes per workgroup, one sample per lane and trip; w and h are multiples of 16):
  160 x 128   levels 1 and 2 (320 / 80 samples) have fewer samples than lanes: lanes with 0 and 1 trips -- no iteration of the two-trip loop, the trip behind it
              alone; level 0 (1 280): 2 and 3 trips
  256 x 128   level 0 has exactly 4 x 512 samples: every lane runs off the end in the same trip, two full iterations and nothing behind them
  320 x 240   4 800 level-0 samples: lanes with 9 and 10 trips; with the continuation's / latency mode's 8 workgroups lanes with 1 and 2
  336 x 240   every level's row pitch differs from its width
Forms: the flat kernel of big batches ("trk_regs" 2) without and with its continuation ("trk_split" 1: the shared sweeps run from the second level-0 trial on),
latency mode with 8 workgroups per stream and with 1, each with "trk_lazy_chi2" 0 / 1 / 2.  Latency mode with ONE workgroup walks the samples in the flat
kernel's order, lane for lane, so the two are bit-equal (tests/test_gpu_frontend.py holds them so at 640 x 480); with 8 workgroups the f64 partial sums are
added in another order and the poses agree to 1e-9 only -- that form is held to the oracle like the others, not to the flat kernel's bits.

Two batches of three streams per size.  "plain": three different frame pairs (forwards from a perturbed guess, the same pair backwards, another pair of the
trajectory from the identity).  "masked", for the skipped accumulation: a previous frame with 10 % invalid depth in blobs; a start pose displaced (roll 0.1 rad,
0.6 m along the optical axis) so far that at least 14 % of every level's valid samples project outside the border of 2 -- chosen on the oracle, which still
converges from it at all four sizes (pose error 0.6 -> < 0.01); a stream without any valid depth (zero valid samples: pose returned as it came in)."""
import numpy as np
import pytest

from test_gpu_big_batch import POSE_TOL, _Oracle, _dedup
from test_gpu_frame_sizes import _candidates, _guess, frames
from test_gpu_frontend import _check_cpu_sem_trajectory

pytestmark = pytest.mark.gpu

I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
SIZES = [(160, 128), (256, 128), (320, 240), (336, 240)]
DEFAULTS = {"trk_regs": 0, "trk_nwg": 0, "trk_split": 10, "trk_lazy_chi2": 1, "trk_balance": 1}
FORMS = {
    "flat": {"trk_regs": 2, "trk_nwg": 1, "trk_split": 0},
    "flat+continuation": {"trk_regs": 2, "trk_nwg": 1, "trk_split": 1},
    "latency x8": {"trk_nwg": 8},
    "latency x1": {"trk_nwg": 1},
}
OUTSIDE_SHARE = 0.14      # of a level's valid samples, at the displaced start pose
_CASES = {}


def _share_outside(orc, disp, T0):
    """per level: the share of the valid samples that the tracker's in-frame test (border 2, on the truncated float position) rejects at pose T0"""
    out = []
    for l, c in enumerate(orc.clouds(disp, I34)):
        cam = orc.cams[l]
        p = c.reshape(-1, 4).astype(np.float64)
        q = p[p[:, 3] > 0, :3] @ T0[:, :3].T + T0[:, 3]
        ui = np.trunc((cam.f * q[:, 0] / q[:, 2] + cam.cx).astype(np.float32)).astype(np.int64)
        vi = np.trunc((cam.f * q[:, 1] / q[:, 2] + cam.cy).astype(np.float32)).astype(np.int64)
        out.append(1.0 - float(((ui >= 2) & (vi >= 2) & (ui < cam.w - 2) & (vi < cam.h - 2)).mean()))
    return out


def _streams(w, h, kind):
    """(camera, three tracker inputs, the oracle's run of each), formed once per size and kind"""
    if (w, h, kind) not in _CASES:
        from scavislam_amd import synth
        F = frames(w, h)
        cam, traj, idx = F["cam"], F["traj"], F["idx"]
        prev, cur = (F["prev"][0], F["prev"][2]), (F["cur"][0], F["cur"][2])
        g = _guess(F)
        orc = _Oracle(cam)
        if kind == "plain":
            sc = synth.Scene(2011)
            a, b = sc.render(cam, traj[2], seed=21), sc.render(cam, traj[3], seed=22)
            T = [dict(prev=prev, cur=cur, T0=g), dict(prev=cur, cur=prev, T0=synth.pose_inv(g)), dict(prev=a, cur=b, T0=I34)]
        else:
            T_true = synth.pose_mul(traj[idx["cur"]], synth.pose_inv(traj[idx["prev"]]))
            far = synth.pose_mul(synth.pose(synth.so3_exp(np.array([0.0, 0.0, 0.1])), np.array([0.0, 0.0, -0.6])), T_true)
            holes = synth.depth_holes(prev[1], np.random.default_rng(5))
            assert 0.08 < float((holes <= 0).mean()) - float((prev[1] <= 0).mean()) < 0.2
            share = _share_outside(orc, prev[1], far)
            print(f"{w} x {h}: share of the valid samples outside at the displaced start, levels 0..2: {share}")
            assert min(share) >= OUTSIDE_SHARE, share
            T = [dict(prev=(prev[0], holes), cur=cur, T0=g), dict(prev=prev, cur=cur, T0=far), dict(prev=(prev[0], np.zeros_like(prev[1])), cur=cur, T0=g)]
        refs = [orc.track(t["prev"], t["cur"], I34, t["T0"]) for t in T]
        if kind == "masked":
            err0, err1 = np.abs(far - T_true).max(), np.abs(refs[1][0] - T_true).max()
            print(f"{w} x {h}: the oracle from the displaced start: pose error {err0:.2e} -> {err1:.2e}")
            assert err1 < 0.02 * err0, "the oracle does not converge from the displaced start"
            assert np.array_equal(refs[2][0], np.asarray(g).reshape(3, 4)) and not refs[2][2][:, 2:].any()      # no valid sample: every chi2 0, pose untouched
        _CASES[(w, h, kind)] = (cam, T, refs)
    return _CASES[(w, h, kind)]


def _track(ctx, stream, cam, T, options, sums_at=None):
    """the three streams through denseTrackingCpu with `options`; sums_at: also one H,b pass per level at these poses (svs_dense_pass_cpu_sem)"""
    from scavislam_amd.frontend import DenseTracker, FramePyramid
    B = len(T)
    prev = FramePyramid(ctx, stream, cam, batch=B)
    cur = FramePyramid(ctx, stream, cam, batch=B)
    prev.upload(np.stack([t["prev"][0] for t in T]), np.stack([t["prev"][1] for t in T]))
    cur.upload(np.stack([t["cur"][0] for t in T]), np.stack([t["cur"][1] for t in T]))
    prev.preprocessing(); cur.preprocessing()
    dtp = DenseTracker(ctx, prev)
    dtp.computeDensePointCloudCpu(I34.reshape(12))
    dt = DenseTracker(ctx, cur)
    dt.ref_dense_points = dtp.ref_dense_points
    sums = [dt.pass_sums(l, prev.pyr, sums_at, True) for l in range(3)] if sums_at is not None else None
    for name, v in options.items():
        ctx.set_option(name, v)
    try:
        fb0 = ctx.get_stat("trk_exact_fallbacks")
        Tout, passes = dt.denseTrackingCpu(prev.pyr, np.stack([np.asarray(t["T0"]).reshape(12) for t in T]), from_u8=True)
        recs = dt.lm_records()
        fb = ctx.get_stat("trk_exact_fallbacks") - fb0
    finally:
        for name in options:
            ctx.set_option(name, DEFAULTS[name])
    return Tout, passes, recs, fb, sums


@pytest.mark.parametrize("lazy", [0, 1, 2])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["plain", "masked"])
@pytest.mark.parametrize("w,h", SIZES)
def test_sweep_against_the_oracle(gpu_ctx, w, h, kind, form, lazy):
    ctx, stream = gpu_ctx
    cam, T, refs = _streams(w, h, kind)
    Tout, passes, recs, fb, _ = _track(ctx, stream, cam, T, dict(FORMS[form], trk_lazy_chi2=lazy))
    assert fb == 0, "an exact float sum fell back to the chain"
    for b, (T_ref, passes_ref, rec_ref) in enumerate(refs):
        lab = f"{w} x {h}, {kind}, {form}, trk_lazy_chi2 {lazy}, stream {b}"
        assert passes[b] > 0, lab
        ref = _dedup(rec_ref)
        if form == "flat+continuation" and ((ref[:, 0] == 0) & (ref[:, 1] < 2)).sum() > 1:      # (it parks after one level-0 trial iff it takes another)
            assert ((recs[b]["level"] == 0) & (recs[b]["accepted"] < 2)).sum() > 1, (lab, "the stream never parked: no shared sweep ran")
        _check_cpu_sem_trajectory(recs[b], passes[b], rec_ref, passes_ref, lab)
        no_valid = kind == "masked" and b == 2
        np.testing.assert_allclose(Tout[b], T_ref, rtol=0, atol=POSE_TOL["no_depth" if no_valid else None], err_msg=lab)
        if no_valid:
            assert np.array_equal(Tout[b], np.asarray(T[b]["T0"]).reshape(3, 4)), (lab, "no valid sample: the pose must come back as it went in")


@pytest.mark.parametrize("lazy", [0, 1, 2])
@pytest.mark.parametrize("kind", ["plain", "masked"])
@pytest.mark.parametrize("w,h", SIZES)
def test_flat_and_latency_mode_bit_equal(gpu_ctx, w, h, kind, lazy):
    """the flat kernel and the latency-mode kernel with one workgroup per stream: same samples per lane in the same order, so the same bytes"""
    ctx, stream = gpu_ctx
    cam, T, _ = _streams(w, h, kind)
    Tf, pf, rf, fbf, _ = _track(ctx, stream, cam, T, dict(FORMS["flat"], trk_lazy_chi2=lazy))
    Tl, pl, rl, fbl, _ = _track(ctx, stream, cam, T, dict(FORMS["latency x1"], trk_lazy_chi2=lazy))
    assert fbf == 0 and fbl == 0
    assert np.array_equal(Tf, Tl) and np.array_equal(pf, pl)
    for b in range(len(T)):
        assert np.array_equal(rf[b], rl[b]), (w, h, kind, lazy, b)


@pytest.mark.parametrize("w,h", SIZES)
def test_masked_samples_are_not_counted(gpu_ctx, w, h):
    """one H,b pass per level at the start poses of the masked batch (the f32-source instantiation of the same sample function): n_valid is the oracle's count,
    H and b within 1e-9 of the serial oracle (the bar of test_dense_pointcloud_and_single_pass); the stream without depth: n_valid 0 and every sum +0"""
    import oracle as O
    ctx, stream = gpu_ctx
    cam, T, _ = _streams(w, h, "masked")
    orc = _Oracle(cam)
    T0 = np.stack([np.asarray(t["T0"]).reshape(12) for t in T])
    sums = _track(ctx, stream, cam, T, {}, sums_at=T0)[4]
    for b, t in enumerate(T):
        clouds = orc.clouds(t["prev"][1], I34)
        pyr_p, _ = orc.prep(t["prev"][0])
        _, fl = orc.prep(t["cur"][0])
        for l in range(3):
            ref = O.dense_pass_cpu(clouds[l], pyr_p[l], fl[l][0], fl[l][1], fl[l][2], orc.cams[l], T0[b].reshape(3, 4), True)
            got = sums[l][b]
            print(f"{w} x {h}, stream {b}, level {l}: n_valid {got['n_valid']} of {clouds[l].shape[0] * clouds[l].shape[1]}")
            assert got["n_valid"] == ref["n_valid"], (w, h, b, l)
            if b == 2:
                assert got["n_valid"] == 0 and got["chi2"] == 0
                for name in ("H", "b", "chi2"):
                    assert not np.asarray(got[name]).view(np.uint64).any(), (name, "not +0")
            else:
                assert ref["n_valid"] > 20
                np.testing.assert_allclose(got["chi2"], ref["chi2"], rtol=1e-4)
                np.testing.assert_allclose(got["H"], ref["H"], rtol=0, atol=1e-9 * np.abs(ref["H"]).max())
                np.testing.assert_allclose(got["b"], ref["b"], rtol=0, atol=1e-9 * np.abs(ref["b"]).max() + 1e-12)


def test_balanced_order_bit_equal_to_stream_order(gpu_ctx):
    """B = 2 n_cu + 1 streams of 320 x 240 through the front end (the flat kernel's ordered launch and its continuation), three tracked frames -- the order
    changes from the second on: "trk_balance" 0 and 1 give the same bytes (LM records, results, poses)"""
    import torch
    from scavislam_amd import capi, synth
    from scavislam_amd.frontend import StereoFrontend
    ctx, stream = gpu_ctx
    w, h = 320, 240
    F = frames(w, h)
    cam, traj, idx = F["cam"], F["traj"], F["idx"]
    pts, g = _candidates(F), _guess(F)
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    fwd = np.arange(B) % 3 != 1                       # every third stream tracks backwards: neighbouring slots differ
    dev = torch.device("cuda", 0)

    def up(j):                                        # frame j of every stream's own order (kf, then prev / cur or cur / prev)
        names = [("kf", "prev", "cur", "prev", "cur")[j] if f else ("kf", "cur", "prev", "cur", "prev")[j] for f in fwd]
        with torch.cuda.stream(stream):
            left = torch.as_tensor(np.stack([F[n][0] for n in names])).to(dev)
            disp = torch.as_tensor(np.stack([F[n][2] for n in names]).astype(np.float32)).to(dev)
        stream.synchronize()
        return dict(left=left, disp=disp)

    frames_dev = [up(j) for j in range(5)]
    T_guess = np.stack([(g if f else synth.pose_inv(g)).reshape(12) for f in fwd])
    T_guess_back = np.stack([(synth.pose_inv(g) if f else g).reshape(12) for f in fwd])
    T_act = np.stack([traj[idx["prev"] if f else idx["cur"]].reshape(12) for f in fwd])

    def run(mode):
        ctx.set_option("trk_balance", mode)
        try:
            fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2, params=capi.FrontendParams.reference(), n_streams=B)
            fe.processFirstFrames(**frames_dev[0])
            fe.keepKeyframes(0, np.stack([traj[idx["kf"]].reshape(12)] * B))
            fe.processFirstFrames(**frames_dev[1])
            fe.setCandidateListsAll([pts] * B, [[len(pts) // 2, len(pts)]] * B)
            out = []
            for j, Tg in ((2, T_guess), (3, T_guess_back), (4, T_guess)):
                fe.processFrames(Tg, T_act, **frames_dev[j])
                T, ok = fe.poses()
                out.append(dict(T=T.tobytes(), ok=ok.tobytes(), rec=[fe.denseRecords(b) for b in range(B)],
                                res=[tuple(bytes(x) if not isinstance(x, np.ndarray) else x.tobytes() for x in fe.results(b)) for b in (0, 1, 2, B - 1)]))
            fe.close()
            return out
        finally:
            ctx.set_option("trk_balance", 1)

    fb0 = ctx.get_stat("trk_exact_fallbacks")
    base, order = run(0), run(1)
    assert ctx.get_stat("trk_exact_fallbacks") == fb0
    for k in range(3):
        assert base[k]["T"] == order[k]["T"] and base[k]["ok"] == order[k]["ok"], k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base[k]["rec"], order[k]["rec"])), k
        assert base[k]["res"] == order[k]["res"], k
        assert all(len(r) > 3 for r in order[k]["rec"]), k
