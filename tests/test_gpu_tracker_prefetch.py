"""The dense tracker's sample loop at its edges, every launch form against the oracle (profiles/tracker_prefetch.md: the sweep's term store and prefetch are no
longer waited for in front of the tap loads; the arithmetic is untouched, so every LM record must stay the oracle's).

Sizes, the smallest at which the loop's edges occur (512 lanes per workgroup, one sample per lane and trip):
  320 x 240   4 800 level-0 samples: 9.4 trips per lane with one workgroup (the last one partly out of range), 1.2 with eight; 1 200 on level 1 (2.3 trips);
              300 on level 2, fewer than the lanes.  (w and h must be multiples of 16 -- three quarter-grid levels --, so this is the frame with the 4 800 / 300
              samples; its level-1 and level-2 rows are padded: pitch 192 / 128 for 160 / 80 pixels.)
  160 x 128   1 280 level-0 samples: first trip, one steady-state trip, a partly filled last one; levels 1 and 2 (320 / 80 samples) run the first-trip path only.
              64 x 48 (192 samples, no steady-state trip anywhere) does not track with the synthetic scene: on the CPU oracle no step is accepted on level 2 and
              the pose error GROWS from the guess (4.1e-3 -> 1.5e-2; backwards 4.0e-3 -> 5.6e-2), so the smallest frame of tests/test_gpu_frame_sizes.py that
              converges stands in (from the identity 5.0e-2 -> 6.3e-3, 10 accepted steps).
  336 x 240   the level-0 pitch (384) differs from the width too.
Forms: the flat kernel of big batches on 3 streams ("trk_regs" 2) without and with its continuation launch ("trk_split" 1: a stream parks after ONE level-0
trial, the shared sweeps -- terms stored past the caches -- run from the second on); latency mode with 8 workgroups per stream; each with "trk_lazy_chi2" 0
(no term is ever stored), 1 and 2.  "trk_balance" 0 / 1 (the ordered launch, B > 2 n_cu through the front end) bit-equal to each other."""
import numpy as np
import pytest

from test_gpu_big_batch import POSE_TOL, _Oracle
from test_gpu_frame_sizes import _candidates, _guess, cam_of, frames
from test_gpu_frontend import _check_cpu_sem_trajectory

pytestmark = pytest.mark.gpu

I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
DEFAULTS = {"trk_regs": 0, "trk_nwg": 0, "trk_split": 10, "trk_lazy_chi2": 1, "trk_balance": 1}
FORMS = {
    "flat": {"trk_regs": 2, "trk_nwg": 1, "trk_split": 0},
    "flat+continuation": {"trk_regs": 2, "trk_nwg": 1, "trk_split": 1},
    "latency x8": {"trk_nwg": 8},
}
_CASES = {}


def _streams(w, h):
    """three tracker inputs out of the size's cached frames (forwards from a perturbed guess, backwards, forwards from the identity) + the oracle's run of each"""
    if (w, h) not in _CASES:
        from scavislam_amd import synth
        F = frames(w, h)
        g = _guess(F)
        T = [dict(prev=(F["prev"][0], F["prev"][2]), cur=(F["cur"][0], F["cur"][2]), T0=g),
             dict(prev=(F["cur"][0], F["cur"][2]), cur=(F["prev"][0], F["prev"][2]), T0=synth.pose_inv(g)),
             dict(prev=(F["prev"][0], F["prev"][2]), cur=(F["cur"][0], F["cur"][2]), T0=I34)]
        orc = _Oracle(F["cam"])
        _CASES[(w, h)] = (F["cam"], T, [orc.track(t["prev"], t["cur"], I34, t["T0"]) for t in T])
    return _CASES[(w, h)]


def _track(ctx, stream, cam, T, options):
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
    return Tout, passes, recs, fb


@pytest.mark.parametrize("lazy", [0, 1, 2])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("w,h", [(320, 240), (160, 128), (336, 240)])
def test_sweep_edges_against_the_oracle(gpu_ctx, w, h, form, lazy):
    ctx, stream = gpu_ctx
    cam, T, refs = _streams(w, h)
    Tout, passes, recs, fb = _track(ctx, stream, cam, T, dict(FORMS[form], trk_lazy_chi2=lazy))
    assert fb == 0, "an exact float sum fell back to the chain"
    for b, (T_ref, passes_ref, rec_ref) in enumerate(refs):
        lab = f"{w} x {h}, {form}, trk_lazy_chi2 {lazy}, stream {b}"
        assert passes[b] > 0, lab
        if form == "flat+continuation":
            assert ((recs[b]["level"] == 0) & (recs[b]["accepted"] < 2)).sum() > 1, (lab, "the stream never parked: no shared sweep ran")
        _check_cpu_sem_trajectory(recs[b], passes[b], rec_ref, passes_ref, lab)
        np.testing.assert_allclose(Tout[b], T_ref, rtol=0, atol=POSE_TOL[None], err_msg=lab)


def test_balanced_order_bit_equal_to_stream_order(gpu_ctx):
    """B = 2 n_cu + 1 streams of 320 x 240 through the front end (the flat kernel's ordered launch and its continuation), three tracked frames -- the order
    changes from the second on: "trk_balance" 0 and 1 give the same bytes (LM records, results, poses)"""
    import torch
    from scavislam_amd import capi
    from scavislam_amd.frontend import StereoFrontend
    ctx, stream = gpu_ctx
    w, h = 320, 240
    F = frames(w, h)
    cam, traj, idx = F["cam"], F["traj"], F["idx"]
    pts, g = _candidates(F), _guess(F)
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    from scavislam_amd import synth
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
