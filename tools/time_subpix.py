"""Times and figures of the matcher's sub-pixel refinement (svs_match_subpixel, svs_frontend_set_subpixel) for profiles/subpix.md.  Needs an MI355X.

    python tools/time_subpix.py step --mode off|on [--root DIR]    the front-end step at bench.py's headline shape (512 streams, 640 x 480, 2000 candidates, the
                                                                   frames in device memory), per step between two HIP events, median and spread over --reps steps.
                                                                   --root: import the package from another checkout (the parent commit's build, mode off)
    python tools/time_subpix.py pass                               the stateless pass alone at 512 streams x 2000 candidates, per call between two HIP events
    python tools/time_subpix.py sequence                           synth.trajectory's sequence, one stream, calcFastMotionOnly in the loop: chi2 / num_obs and the
                                                                   pose error against the rendered ground truth with the pass off, on (1 iteration), on (8),
                                                                   and the count of every svs_subpix_info state
Every run prints one JSON line.  Times are medians over at least 30 repetitions after warm-up; "spread" is (min, 25 %, 75 %, max)."""
import argparse
import json
import os
import sys
import time

import numpy as np


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_ms=round(float(np.median(ms)), 4), spread_ms=[round(float(np.percentile(ms, q)), 4) for q in (0, 25, 75, 100)], reps=len(ms))


def inputs(cam, npair):
    """bench.py's pairs: NPAIR (previous, current) frames with different inter-frame motions"""
    from concurrent.futures import ThreadPoolExecutor
    from scavislam_amd import synth
    scene, traj = synth.Scene(2011), synth.trajectory(8)
    mrng = np.random.default_rng(77)
    T_prev, T_cur = [], []
    for p in range(npair):
        T_p = traj[4 + p % 4]
        step, yaw = mrng.uniform(0.02, 0.08), np.deg2rad(mrng.uniform(0.05, 0.5)) * mrng.choice([-1, 1])
        R_rel = synth.so3_exp(np.array([mrng.normal(0, 0.0005), yaw, mrng.normal(0, 0.0005)]))
        T_rel = synth.pose(R_rel, np.array([mrng.normal(0, 0.003), mrng.normal(0, 0.002), -step]))
        T_prev.append(T_p)
        T_cur.append(synth.pose_mul(T_rel, T_p))
    jobs = [(T_prev[p], 100 + p) for p in range(npair)] + [(T_cur[p], 200 + p) for p in range(npair)]
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        rend = list(ex.map(lambda j: scene.render(cam, j[0], seed=j[1]), jobs))
    return dict(T_prev=T_prev, T_cur=T_cur, prev=rend[:npair], cur=rend[npair:], T_AB=[synth.pose_mul(T_cur[p], synth.pose_inv(T_prev[p])) for p in range(npair)])


def candidates(cam, inp, p, n):
    from scavislam_amd import synth
    pts = synth.candidate_points(np.random.default_rng(2011 + p), cam, np.maximum(inp["prev"][p][1], 0), inp["T_prev"][p],
                                 (int(n * 0.6), int(n * 0.3), n - int(n * 0.6) - int(n * 0.3)))
    pts["point_id"] = np.arange(len(pts))
    return pts


def run_step(args):
    import torch
    from scavislam_amd import capi, synth
    from scavislam_amd.frontend import StereoFrontend
    ctx, stream = capi.torch_context(0)
    cam, B = synth.CAM_DEFAULT, args.batch
    inp = inputs(cam, args.pairs)
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
    pair = [b % args.pairs for b in range(B)]
    fe = StereoFrontend(ctx, cam, max_points=args.points, max_keyframes=1, params=capi.FrontendParams.reference(), n_streams=B)
    with torch.cuda.stream(stream):
        left = [torch.as_tensor(np.stack([inp[k][p][0] for p in pair])).cuda() for k in ("prev", "cur")]
        disp = [torch.as_tensor(np.stack([inp[k][p][1] for p in pair]).astype(np.float32)).cuda() for k in ("prev", "cur")]
    stream.synchronize()
    ready = torch.cuda.Event()
    with torch.cuda.stream(stream):
        ready.record(stream)
    T_act = np.stack([inp["T_prev"][p].reshape(12) for p in pair])
    T_pose = [np.tile(I34, (B, 1)), np.stack([inp["T_AB"][p].reshape(12) for p in pair])]
    fe.processFirstFrames(left=left[0], disp=disp[0])
    fe.keepKeyframes(0, T_act)
    pts = {p: candidates(cam, inp, p, args.points) for p in set(pair)}
    fe.setCandidateListsAll([pts[p] for p in pair], [[len(pts[p]) // 2, len(pts[p])] for p in pair])
    if args.mode == "on":
        fe.setSubpixel(args.iterations, 1.5, 0.03)
    k = 0

    def step():
        nonlocal k
        k += 1
        f = k & 1
        fe.processFrames(T_pose[1 - f], T_act, left=left[f], disp=disp[f], ready_event=ready)
    ms = []
    with torch.cuda.stream(stream):
        for _ in range(args.warmup + (args.warmup & 1)):
            step()
        ctx.sync()
        t0 = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
        ev[0].record(stream)
        for i in range(args.reps):
            step()
            ev[i + 1].record(stream)
        ctx.sync()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.reps * 1e3
        ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
    out = dict(what="front-end step", root=args.root or ".", mode=args.mode, streams=B, points=args.points, frame="640x480", wall_ms_per_step=round(wall, 4), **stats(ms))
    if args.mode == "on":
        st = np.zeros(5, np.int64)
        n_ok = 0
        for b in range(0, B, max(B // 32, 1)):
            st += np.bincount(fe.subpixelInfo(b)["state"], minlength=5)[:5]
            n_ok += int((fe.results(b)[1]["status"] == 0).sum())
        out.update(iterations=args.iterations, states_of_sampled_streams=dict(zip(("refined", "untouched", "singular", "shift", "no_disp"), (int(x) for x in st))), ok_after=n_ok)
    fe.close()
    print(json.dumps(out))


def run_pass(args):
    """svs_match on 512 streams x 2000 candidates through the stateless classes, then the pass alone on a fresh copy of those records per repetition"""
    import torch
    from scavislam_amd import capi, synth
    from scavislam_amd.frontend import FastGrid, FramePyramid, GuidedMatcher
    ctx, stream = capi.torch_context(0)
    cam, B = synth.CAM_DEFAULT, args.batch
    inp = inputs(cam, args.pairs)
    pair = [b % args.pairs for b in range(B)]
    kf, cur = FramePyramid(ctx, stream, cam, batch=B, with_float=False), FramePyramid(ctx, stream, cam, batch=B, with_float=False)
    kf.upload(np.stack([inp["prev"][p][0] for p in pair]), np.stack([inp["prev"][p][1] for p in pair]))
    kf.preprocessing()
    cur.upload(np.stack([inp["cur"][p][0] for p in pair]), np.stack([inp["cur"][p][1] for p in pair]))
    cur.preprocessing()
    fg = FastGrid(ctx, cur)
    fg.detectAdaptively(trials=6)
    # one keyframe table for all slots (the stateless default): stream b's keyframe is entry b
    gm = GuidedMatcher(ctx, cur, fg)
    per_pair = {p: candidates(cam, inp, p, args.points) for p in set(pair)}
    n = min(len(v) for v in per_pair.values())
    pts = np.stack([per_pair[p][:n] for p in pair])
    pts["kf_index"] = np.arange(B)[:, None]
    a = gm.prepare([(kf.pyr, b, inp["T_prev"][pair[b]].reshape(12)) for b in range(B)], np.stack([inp["T_AB"][p].reshape(12) for p in pair]),
                   np.stack([inp["T_prev"][p].reshape(12) for p in pair]), pts)
    gm.launch(a)
    ctx.sync()
    d_res = gm._keep[4]
    saved = d_res.clone()
    res = gm.download()
    ms = []
    for it in range(args.warmup + args.reps):
        with torch.cuda.stream(stream):
            d_res.copy_(saved)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        gm.refineSubpixel(a, args.iterations, 1.5, 0.03, want_info=False)
        with torch.cuda.stream(stream):
            e1.record(stream)
        ctx.sync()
        torch.cuda.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    d_res.copy_(saved)
    info = gm.refineSubpixel(a, args.iterations, 1.5, 0.03)
    n_ok = int((res["status"] == 0).sum())
    print(json.dumps(dict(what="stateless pass", streams=B, points=args.points, iterations=args.iterations, ok_records=n_ok, **stats(ms),
                          ns_per_ok_record=round(float(np.median(ms)) * 1e6 / max(n_ok, 1), 2),
                          states=dict(zip(("refined", "untouched", "singular", "shift", "no_disp"), (int(x) for x in np.bincount(info["state"].ravel(), minlength=5)[:5]))))))
    fg.close()


def run_sequence(args):
    from scavislam_amd import capi, synth
    from scavislam_amd.frontend import StereoFrontend
    ctx, stream = capi.torch_context(0)
    cam = synth.CAM_DEFAULT
    sc, traj = synth.Scene(2011), synth.trajectory(args.frames + 1)
    frames = [sc.render(cam, traj[i], seed=i) for i in range(args.frames + 1)]
    pts = synth.candidate_points(np.random.default_rng(4), cam, np.maximum(frames[0][1], 0), traj[0], (1200, 600, 200))
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
    rows = {}
    for name, sp in (("off", None), ("on_1", (1, 1.5, 0.03)), ("on_8", (8, 1.5, 0.03))):
        fe = StereoFrontend(ctx, cam, max_points=len(pts), max_keyframes=1)
        fe.processFirstFrame(frames[0][0], disp=frames[0][1])
        fe.keepKeyframe(0, traj[0])
        fe.setCandidates(pts, len(pts) // 2)
        if sp:
            fe.setSubpixel(*sp)
        T = I34.copy()
        chi2n, et, er, nobs, states = [], [], [], [], np.zeros(5, np.int64)
        for i in range(1, args.frames + 1):
            res, m, g = fe.processFrame(frames[i][0], T, traj[0], disp=frames[i][1])
            T = np.array(res.T_cur_from_actkey)
            Tt = synth.pose_mul(traj[i], synth.pose_inv(traj[0]))
            D = synth.pose_mul(T.reshape(3, 4), synth.pose_inv(Tt))
            et.append(float(np.linalg.norm(D[:, 3])))
            er.append(float(np.degrees(np.arccos(np.clip((np.trace(D[:, :3]) - 1) / 2, -1, 1)))))
            nobs.append(res.pose_stats.num_obs)
            chi2n.append(res.pose_stats.chi2 / max(res.pose_stats.num_obs, 1))
            if sp:
                states += np.bincount(fe.subpixelInfo(0)["state"], minlength=5)[:5]
        fe.close()
        rows[name] = dict(chi2_per_obs_mean=round(float(np.mean(chi2n)), 5), chi2_per_obs_median=round(float(np.median(chi2n)), 5), num_obs_mean=round(float(np.mean(nobs)), 1),
                          trans_err_mm_mean=round(1e3 * float(np.mean(et)), 4), trans_err_mm_max=round(1e3 * float(np.max(et)), 4), rot_err_mdeg_mean=round(1e3 * float(np.mean(er)), 4),
                          states=dict(zip(("refined", "untouched", "singular", "shift", "no_disp"), (int(x) for x in states))) if sp else None)
    print(json.dumps(dict(what="sequence", frames=args.frames, frame="640x480", candidates=len(pts), **rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "pass", "sequence"])
    ap.add_argument("--mode", choices=["off", "on"], default="off")
    ap.add_argument("--root", default=None, help="import scavislam_amd from this checkout instead of the one the tool lies in")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    assert args.reps >= 30
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"step": run_step, "pass": run_pass, "sequence": run_sequence}[args.what](args)


if __name__ == "__main__":
    main()
