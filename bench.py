#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric: "stereo frames/sec + DWO Schur ms @ 50 KF / 20k pts".

One JSON line on rank 0.  Two timed regions (B with --full only), each K steps, barrier + synchronize on both
sides, max over ranks:
  A. front-end: a step = one pass of the per-frame hot path (pyramid, device-resident dense tracking
     with the f32 conversion + Sobel taps of preprocessing fused into its gathers, dense point cloud, grid FAST, guided ZNSSD matching of 2000 candidate points)
     over a batch of B independent 640x480 camera streams, inputs resident in HBM.
     value = N * B * K / time  [frames/s]   (weak scaling: front-end frames are replicas)
  B. back-end: a step = one SlamGraph::optimize (2 LM iterations) of a 50-keyframe / 20k-landmark
     window, landmarks sharded over the N ranks, one RCCL all-reduce of the packed reduced camera
     system per LM trial.  schur.ms_per_optimize (strong scaling: the window is fixed).
`roofline` is the Schur (landmark) kernel: algorithmic bytes / its average launch duration measured
with HIP events on its own stream; `roofline_frontend` lists the front-end kernels the same way.
`cpu_baseline` is the CPU oracle (a port of the reference's CPU path) timed on the host cores of
this box on a bounded sample; it is the checker's code used as a baseline, never the product.

A plain run times region A alone and prints the headline (metric, value, ms_per_step, ...); region B,
the rooflines, the CPU baseline and every other row run with --full.  --dump-outputs DIR writes what
the last timed step of region A computed (dump_outputs below).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec (MI355X_MICROARCH.md); 6290 GB/s is the measured copy ceiling


class _stdout_to_stderr:
    """RCCL prints a version banner on STDOUT when a communicator is created; rank 0's stdout must carry exactly one JSON line."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *a):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def launch_ranks(args):
    """one rank per GPU of this node over RCCL: re-exec through torch.distributed.run with the caller's own arguments"""
    import socket
    import subprocess
    if not args.dry_launch:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} requested, {have} visible on this node")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc:
        raise SystemExit(rc)


def dry_launch(args, world, rank):
    """--dry-launch: the ranks of `--gpus N` meet over gloo on the CPU and rank 0 reports them (tests/test_dist_gloo.py keeps the launcher from rotting)"""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(seen, torch.tensor([rank], dtype=torch.int64))
    if rank == 0:
        print(json.dumps({"dry_launch": True, "n_gpus": world, "requested": args.gpus, "ranks_seen": sorted(int(t.item()) for t in seen)}))
    dist.barrier()
    dist.destroy_process_group()


def _flat_fields(s):
    """a ctypes result structure as a flat list of floats, padding left out (every field here is an int32 or a double: exact in float64)"""
    import ctypes as C
    out = []
    for name, _ in s._fields_:
        if name.startswith("pad"):
            continue
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out += _flat_fields(v)
        elif isinstance(v, C.Array):
            out += [float(x) for x in v]
        else:
            out.append(float(v))
    return out


def dump_outputs(dirname, fe, n_streams, n_sample=64):
    """--dump-outputs: what the last timed step handed back, as a caller of svs_frontend_process_frames receives it.  Every stream: refined pose,
    tracking flag and FrameResult scalars.  A fixed sample of streams (seeded): match records, gated points and the three dense clouds -- all streams'
    records and clouds would be ~180 MB.  Integer fields are stored as float64 (exact)."""
    os.makedirs(dirname, exist_ok=True)
    T, ok = fe.poses()
    sample = np.sort(np.random.default_rng(0).choice(n_streams, min(n_sample, n_streams), replace=False))
    arrays = {"poses": T.astype(np.float64), "tracking_ok": ok.astype(np.float64), "sample_streams": sample.astype(np.float64)}
    scalars, match, gated = [], [], []
    in_sample = set(int(b) for b in sample)
    for b in range(n_streams):
        res, m, g = fe.results(b)
        scalars.append(_flat_fields(res))
        if b in in_sample:
            match.append(np.concatenate([np.stack([m[k].astype(np.float64) for k in ("status", "u", "v", "znssd")], 1), m["obs"], m["xyz_actkey"]], 1))
            gated.append(np.concatenate([np.stack([g[k].astype(np.float64) for k in ("accepted", "is_new")], 1), g["uv_pyr"], g["curkey_uv_pyr"]], 1))
    arrays["frame_results"] = np.asarray(scalars, np.float64)
    arrays["match_records_sample"] = np.concatenate(match)          # status u v znssd obs[3] xyz_actkey[3], sampled streams in order
    arrays["gated_points_sample"] = np.concatenate(gated)           # accepted is_new uv_pyr[2] curkey_uv_pyr[2]
    for l in range(3):
        arrays[f"cloud_level{l}_sample"] = np.stack([fe.cloud_host(l, int(b)) for b in sample]).astype(np.float32)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes"
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    print(f"bench: {len(arrays)} arrays, {total / 1e6:.1f} MB written to {dirname}", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512, help="independent camera streams per rank per step")
    ap.add_argument("--points", type=int, default=2000, help="candidate points per frame (SURVEY 8d config 2)")
    ap.add_argument("--pairs", type=int, default=32, help="distinct (previous, current) frame pairs with different motions dealt to the streams")
    ap.add_argument("--full-batch", type=int, default=64, help="streams per launch of the full-resolution dense tracker row (BASELINE config 5)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--dry-launch", action="store_true", help="launcher check (tests, no GPU): bring up --gpus ranks over gloo, exchange one message, print who answered")
    ap.add_argument("--quick", action="store_true", help="kernel A/B runs: the front-end headline, its stage times and the accept-test rows only (not the contract's line)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: stage times, accept-test and schedule A/Bs, stereo input, latency mode, "
                                                        "other batches and frame sizes, full-resolution tracker, Schur rows, rooflines, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # `python bench.py --gpus N` IS the multi-GPU command: when no launcher has set the rank environment, this process becomes the launcher and starts one rank per
    # GPU through torch.distributed.run (the driver's explicit `python -m torch.distributed.run ... bench.py --gpus N` finds WORLD_SIZE set and falls through)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args)

    import torch
    import torch.distributed as dist
    from scavislam_amd import capi, synth
    from scavislam_amd.backend import Communicator, SlamGraphOptimizer, shard_problem
    from scavislam_amd.ctypes_types import BaParams, Cam
    from scavislam_amd.frontend import DenseTracker, FastGrid, FramePyramid, GuidedMatcher, StereoMatcher

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:      # never report a 1-GPU line for an N-GPU request
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); use `python bench.py --gpus {args.gpus}` (it launches the ranks itself) "
                         f"or torch.distributed.run --nproc-per-node {args.gpus}")
    if args.dry_launch:
        return dry_launch(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU fallback")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or "RANK" in os.environ          # launched by torch.distributed.run (even with 1 rank)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        with _stdout_to_stderr():
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            dist.barrier()                                   # creates torch's communicator now (banner goes to stderr)
    ctx, stream = capi.torch_context(local_rank)

    def _probe_windows(tag):      # SVS_BENCH_DEBUG: the windows-in-flight figure at several points of the run (what in this process halves it?)
        if not os.environ.get("SVS_BENCH_DEBUG"):
            return
        from scavislam_amd.backend import optimize_batch as _ob
        _prob = synth.ba_window(50, 20000, seed=2012)
        _cm = Cam(*(_prob["cam"][k] for k in ("f", "cx", "cy", "b", "w", "h")))
        _ctxs = [capi.Context(local_rank) for _ in range(32)]
        _opts = []
        for _c in _ctxs:
            _o = SlamGraphOptimizer(_c, None)
            _o.copyDataToG2o(_prob["poses"], _prob["psi"], _prob["edges"], _prob["cons"], _cm, BaParams.reference_defaults())
            _opts.append(_o)
        _tt = []
        for _ in range(6):
            for _o in _opts:
                _o.reset_state(_prob["poses"], _prob["psi"])
            torch.cuda.synchronize()
            _t0 = time.perf_counter()
            _ob(_opts)
            _tt.append(time.perf_counter() - _t0)
        print(f"[bench] probe {tag}: 32 windows {[round(t * 1e3, 2) for t in _tt]} ms", file=sys.stderr)
        for _o in _opts:
            _o.close()
        for _c in _ctxs:
            _c.close()
    _probe_windows('start')
    for kv in os.environ.get("SVS_CTX_OPTIONS", "").split(","):      # kernel A/B runs only ("trk_flat=0,trk_split=0"): context options of the library, never set by the driver
        if "=" in kv:
            ctx.set_option(kv.split("=")[0].strip(), int(kv.split("=")[1]))
    dev = torch.device("cuda", local_rank)
    K, W, B = args.steps, args.warmup, args.batch

    def barrier_sync():
        ctx.sync()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # ------------------------------------------------------------------ synthetic inputs (8d)
    scene = synth.Scene(2011)
    traj = synth.trajectory(8)
    # NPAIR distinct (previous, current) frame pairs with different inter-frame motions: forward step 2..8 cm, yaw 0.05..0.5 deg,
    # a few mm of lateral drift -- so LM pass counts, FAST thresholds and candidate lists differ between the streams of a batch
    NPAIR = args.pairs
    NRIGHT = min(NPAIR, 4)
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)

    def make_inputs(cam_, npair, with_right=True):
        from concurrent.futures import ThreadPoolExecutor
        mrng = np.random.default_rng(77)
        T_prev_l, T_cur_l = [], []
        for p in range(npair):
            T_p = traj[4 + p % 4]
            step, yaw = mrng.uniform(0.02, 0.08), np.deg2rad(mrng.uniform(0.05, 0.5)) * mrng.choice([-1, 1])
            R_rel = synth.so3_exp(np.array([mrng.normal(0, 0.0005), yaw, mrng.normal(0, 0.0005)]))
            T_rel_p = synth.pose(R_rel, np.array([mrng.normal(0, 0.003), mrng.normal(0, 0.002), -step]))     # camera moves forward: points come closer
            T_prev_l.append(T_p)
            T_cur_l.append(synth.pose_mul(T_rel_p, T_p))
        T_right = synth.pose(np.eye(3), np.array([-cam_["b"], 0.0, 0.0]))      # right camera of the stereo rig (for the block matcher)
        nr = min(npair, 4) if with_right else 0
        # every render is a pure function of (pose, seed): rendered on a few host threads (NumPy releases the GIL), the same bytes as one after the other
        jobs = ([(T_prev_l[p], 100 + p) for p in range(npair)] + [(T_cur_l[p], 200 + p) for p in range(npair)] +
                [(synth.pose_mul(T_right, T_cur_l[p]), 1000 + p) for p in range(nr)] + [(synth.pose_mul(T_right, T_prev_l[p]), 1100 + p) for p in range(nr)])
        with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
            rend = list(ex.map(lambda j: scene.render(cam_, j[0], seed=j[1]), jobs))
        rp, rc = rend[:npair], rend[npair:2 * npair]
        rr = [r[0] for r in rend[2 * npair:2 * npair + nr]]
        rrp = [r[0] for r in rend[2 * npair + nr:]]
        return dict(cam=cam_, npair=npair, T_prev_list=T_prev_l, T_cur_list=T_cur_l, rend_prev=rp, rend_cur=rc, rend_right=rr, rend_right_prev=rrp,
                    T_AB=[synth.pose_mul(T_cur_l[p], synth.pose_inv(T_prev_l[p])) for p in range(npair)],      # T_B_from_A: the motion between a stream's two frames
                    pts_of_pair={})

    extended = args.full or args.quick                       # a plain run does only what the headline needs (the right images feed the stereo-input rows)
    INP = make_inputs(synth.CAM_DEFAULT, NPAIR, with_right=extended)
    cam, T_prev_list, T_cur_list, rend_prev, rend_cur, rend_right, rend_right_prev, T_AB, pts_of_pair = (INP[k] for k in (
        "cam", "T_prev_list", "T_cur_list", "rend_prev", "rend_cur", "rend_right", "rend_right_prev", "T_AB", "pts_of_pair"))
    n_per_level = (int(args.points * 0.6), int(args.points * 0.3), args.points - int(args.points * 0.6) - int(args.points * 0.3))
    def candidates_from_corners(p, corners, inp=None):
        """candidate points of a stream = FAST corners of its active keyframe with their stereo depth (what addNewPoints seeds from the keyframe's
        feature_tree, stereo_frontend.cpp:680-830): up to n_per_level per level, the rest of the quota from level 0 (2000 points)"""
        from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
        inp = inp or INP
        cam = inp["cam"]
        rng = np.random.default_rng(2011 + p)
        disp = inp["rend_prev"][p][1]
        per_level = []
        for l in range(3):
            xy = corners[l].astype(np.int64)
            u0, v0 = xy[:, 0] << l, xy[:, 1] << l
            d = disp[v0, u0]
            keep = np.nonzero(d > 0.5)[0]
            per_level.append((l, xy[keep], d[keep].astype(np.float64), rng.permutation(len(keep))))
        take = [min(n_per_level[l], len(per_level[l][3])) for l in range(3)]
        take[0] = min(len(per_level[0][3]), take[0] + (args.points - sum(take)))
        rows = []
        for (l, xy, d, perm), n in zip(per_level, take):
            sel = perm[:n]
            s_ = float(1 << l)
            u0, v0 = xy[sel, 0] * s_, xy[sel, 1] * s_
            z = cam["f"] * cam["b"] / d[sel]
            r = np.zeros(n, CANDIDATE_DTYPE)
            r["xyz_anchor"] = np.stack([(u0 - cam["cx"]) / cam["f"] * z, (v0 - cam["cy"]) / cam["f"] * z, z], 1)
            r["anchor_obs_pyr"] = np.stack([u0 / s_, v0 / s_, (u0 - d[sel]) / s_], 1)
            r["anchor_level"] = l
            rows.append(r)
        pts = np.concatenate(rows)
        pts = pts[rng.permutation(len(pts))]                    # new-feature list and neighbourhood list both hold all levels
        if os.environ.get("SVS_BENCH_SORT_PTS"):                # experiment: the two lists in image order (level, row, column) instead of hash order
            h = len(pts) // 2
            key = lambda q: np.lexsort((q["anchor_obs_pyr"][:, 0], q["anchor_obs_pyr"][:, 1], q["anchor_level"]))
            pts = np.concatenate([pts[:h][key(pts[:h])], pts[h:][key(pts[h:])]])
        pts["kf_index"] = 0
        pts["point_id"] = np.arange(len(pts))
        return pts

    from scavislam_amd.frontend import StereoFrontend

    class OneCall:
        """B camera streams through the one-call front end (svs_frontend_process_frames): every stream owns two resident frames A, B of a
        ping-pong sequence A B A B ... (A = its active keyframe, world = A's pose), the frames stay in HBM (svs_frames_dev pointers), a step =
        StereoFrontend::processFrame for all B streams: copy-in + pyramid, dense tracking, [block matching], grid FAST (6 trials), guided matching of
        `points` candidates (half of them "new features"), calcFastMotionOnly, processMatchedPoints' gate, dense cloud.  Guess = the pose of the
        frame before (one inter-frame motion to recover each step, in alternating directions)."""

        def __init__(self, B, block_matching=False, cuda_build=False, inp=None, ctx=ctx, pair_offset=0):
            self.B, self.bm = B, block_matching
            inp = inp or INP
            cam, NPAIR, pts_of_pair = inp["cam"], inp["npair"], inp["pts_of_pair"]
            rend_prev, rend_cur, rend_right, rend_right_prev, T_prev_list, T_AB = (inp[k] for k in ("rend_prev", "rend_cur", "rend_right", "rend_right_prev", "T_prev_list", "T_AB"))
            NRIGHT = len(rend_right)
            prm = capi.FrontendParams.reference(use_block_matching=block_matching, cuda_build=cuda_build)
            self.fe = StereoFrontend(ctx, cam, max_points=max(args.points, 1), max_keyframes=1, params=prm, n_streams=B)
            pair = [(b + pair_offset) % NPAIR for b in range(B)]
            if os.environ.get("SVS_BENCH_SHUFFLE"):      # experiment (profiles/r4_notes.md): the same multiset of pairs dealt to the streams in a shuffled order
                pair = [int(x) for x in np.random.default_rng(5).permutation(pair)]
            if block_matching:      # only NRIGHT pairs have a rendered right image
                pair = [p % NRIGHT for p in pair]
            self.pair = pair
            with torch.cuda.stream(stream):
                self.left = [torch.as_tensor(np.stack([(rend_prev if k == 0 else rend_cur)[p][0] for p in pair])).to(dev) for k in range(2)]
                if block_matching:
                    self.right = [torch.as_tensor(np.stack([(rend_right_prev if k == 0 else rend_right)[p] for p in pair])).to(dev) for k in range(2)]
                    self.disp = [None, None]
                else:
                    self.right = [None, None]
                    self.disp = [torch.as_tensor(np.stack([(rend_prev if k == 0 else rend_cur)[p][1] for p in pair]).astype(np.float32)).to(dev) for k in range(2)]
            stream.synchronize()
            self.ready = torch.cuda.Event()               # svs_frames_dev::ready_event: these frames are complete from here on (they are never rewritten), which is what
            with torch.cuda.stream(stream):               # lets the library build a frame's pyramid beside the previous frame's pose refinement
                self.ready.record(stream)
            self.T_act = np.stack([T_prev_list[p].reshape(12) for p in pair])
            self.T_pose = [np.tile(I34, (B, 1)), np.stack([T_AB[p].reshape(12) for p in pair])]      # true pose of frame A / B relative to the active keyframe
            self.fe.processFirstFrames(left=self.left[0], right=self.right[0], disp=self.disp[0])     # frame A: the active keyframe, cloud at the identity
            self.fe.keepKeyframes(0, np.stack([T_prev_list[pair[b]].reshape(12) for b in range(B)]))      # one call for all streams
            for b in range(B):
                if pair[b] not in pts_of_pair:                  # the keyframe's own FAST corners (this front end's, first frame: 5 trials)
                    pts_of_pair[pair[b]] = candidates_from_corners(pair[b], [self.fe.corners(b, l)[0] for l in range(3)], inp)
            self.fe.setCandidateListsAll([pts_of_pair[pair[b]] for b in range(B)],
                                         [[len(pts_of_pair[pair[b]]) // 2, len(pts_of_pair[pair[b]])] for b in range(B)])      # one staged upload
            self.k = 0

        def step(self):
            self.k += 1
            f = self.k & 1                                        # 1: frame B (guess: A's pose), 0: frame A (guess: B's pose)
            self.fe.processFrames(self.T_pose[1 - f], self.T_act, left=self.left[f], right=self.right[f], disp=self.disp[f], ready_event=self.ready)

        def close(self):
            self.fe.close()

    def timed_steps(oc, warm, steps):
        with torch.cuda.stream(stream):
            for _ in range(warm):
                oc.step()
            barrier_sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                oc.step()
            barrier_sync()
            return time.perf_counter() - t0

    def run_groups(n_groups, streams, reps=10):
        """n_groups batched front ends of `streams` camera streams each, every group on a context and HIP stream of its own, stepped in turn: a group's matcher,
        refinement and FAST run in the tail of another group's tracker (one workgroup per stream there: its last workgroups leave most CUs idle)."""
        nonlocal ctx, stream
        grp = [capi.torch_context(local_rank) for _ in range(n_groups)]
        ctx_main, stream_main = ctx, stream
        ocs = []
        for cg, sg in grp:
            ctx, stream = cg, sg                                 # OneCall builds on the enclosing ctx / stream
            ocs.append(OneCall(streams, ctx=cg))
        ctx, stream = ctx_main, stream_main
        for _ in range(2):
            for o in ocs:
                o.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            for o in ocs:
                o.step()
        torch.cuda.synchronize()
        t_ov = (time.perf_counter() - t0) / reps
        for o in ocs:
            o.close()
        for cg, _ in grp:
            cg.close()
        return {"groups": n_groups, "streams_per_group": streams, "ms_per_step_of_all_groups": round(t_ov * 1e3, 4), "frames_per_s": round(n_groups * streams / t_ov, 1)}

    _probe_windows('before the first front end')
    oc = OneCall(B)
    _probe_windows('front end created')
    t_front = max_over_ranks(timed_steps(oc, W + (W & 1), K))          # even warm-up: the timed region starts with a frame-B step
    fps = world * B * K / t_front
    headline = {
        "metric": "stereo frames/sec + DWO Schur ms @ 50 KF / 20k pts",
        "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": round(t_front / K * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u8/int32 (FAST, ZNSSD), f32+f64 (dense tracking), f64 (Schur)",
        "data": "synthetic",
    }
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, oc.fe, B)
    if os.environ.get("SVS_BENCH_REPEAT"):          # run-to-run spread of the headline inside ONE process: the same K steps again, N times
        print(json.dumps({"repeat_ms_per_step": [round(t_front / K * 1e3, 4)] + [round(timed_steps(oc, 0, K) / K * 1e3, 4) for _ in range(int(os.environ["SVS_BENCH_REPEAT"]))]}), flush=True)
    if os.environ.get("SVS_BENCH_TRACE_STOP"):      # kernel timelines (tools/timeline.py over a rocprofv3 trace): the trace ends with the headline's own steps
        print(json.dumps({"trace_stop": True, "ms_per_step": round(t_front / K * 1e3, 4)}))
        oc.close()
        return
    if not extended:                                # the plain run: the headline line and nothing else (the rows below are behind --full)
        oc.close()
        if rank == 0:
            print(json.dumps(headline))
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return
    # the tracker's accept test: by default it takes the reference's decisions -- f64 sums where they can decide `float chi2 - float new_chi2 > 0`,
    # the reference's sequential float sums (formed bit for bit, in parallel: csrc/seqsum.h) where they cannot.  How many such sums a frame needs, and what the same
    # steps cost with the f64 sums alone (rounds 1-4: not the reference's decisions near convergence)
    n_exact0 = ctx.get_stat("trk_exact_sums")
    timed_steps(oc, 0, 2)
    exact_sums_per_frame = (ctx.get_stat("trk_exact_sums") - n_exact0) / (2.0 * B)
    exact_fallbacks = ctx.get_stat("trk_exact_fallbacks")
    ctx.set_option("trk_lazy_chi2", 0)
    t_front_f64_accept = max_over_ranks(timed_steps(oc, 2, K))
    t_front_terms_only = None
    if args.quick:
        ctx.set_option("trk_lazy_chi2", 2)
        t_front_terms_only = max_over_ranks(timed_steps(oc, 2, K))
    ctx.set_option("trk_lazy_chi2", 1)
    timed_steps(oc, 2, 0)
    # A/B of the tracker's grid order (context option "trk_balance", dense.hip): 0 = workgroups in stream order, 1 (default) = by the LM work of each stream's
    # last frame, dealt round-robin to the XCDs.  Same K steps; the results of a stream do not depend on the order (one workgroup per stream either way).
    ctx.set_option("trk_balance", 0)
    t_front_stream_order = max_over_ranks(timed_steps(oc, 2, K))
    ctx.set_option("trk_balance", 1)
    timed_steps(oc, 2, 0)
    # what the last step left: poses, matches, dense sweeps (checked against the true motion: the bench is not timing a diverged tracker)
    T_all, ok_all = oc.fe.poses()
    f_last = oc.k & 1
    track_err = float(max(np.abs(T_all[b] - oc.T_pose[f_last][b].reshape(3, 4)).max() for b in range(min(B, NPAIR))))
    res0 = [oc.fe.results(b)[0] for b in range(min(B, NPAIR))]
    n_matched = int(np.mean([r.n_matched for r in res0]))
    n_points = int(np.mean([r.n_points for r in res0]))
    n_accepted = int(np.mean([r.point_stats.num_track_points for r in res0]))
    passes_all = np.array([r.dense_passes for r in res0])
    passes = float(passes_all.mean())
    n_corners = int(np.mean([sum(len(oc.fe.corners(b, l)[0]) for l in range(3)) for b in range(min(B, 4))]))
    tracking_ok_frac = float(ok_all.mean())
    # the same steps with every stage on ONE stream (by default the library enqueues FAST / block matching on a side stream beside the dense tracker):
    # this is the figure the stage times below add up to
    ctx.set_option("fe_overlap", 0)
    t_front_one = timed_steps(oc, 2, K + (K & 1))
    ctx.set_option("fe_overlap", 1)
    ms_one_stream = t_front_one / (K + (K & 1)) * 1e3
    # per-stage times: the same K steps again with event brackets between the stages inside the library (9 events per step)
    oc.fe.setTiming(True)
    stage_acc = {}
    with torch.cuda.stream(stream):
        for _ in range(K + (K & 1)):
            oc.step()
            for k_, v_ in oc.fe.stageTimes().items():
                stage_acc.setdefault(k_, []).append(v_)
    oc.fe.setTiming(False)
    stage_ms = {k_: float(np.mean(v_)) for k_, v_ in stage_acc.items()}
    if args.quick:
        lat_quick = {}
        oc1 = OneCall(1)
        oc1.fe.setTiming(True)
        for mode_, name_ in ((1, "parity"), (2, "terms_stored_f64_accept"), (0, "f64_accept")):
            ctx.set_option("trk_lazy_chi2", mode_)
            acc_ = []
            with torch.cuda.stream(stream):
                for _ in range(12):
                    oc1.step()
                    acc_.append(oc1.fe.stageTimes()["dense_tracking"])
            lat_quick[name_ + "_tracker_ms"] = round(float(np.mean(acc_[2:])), 4)
        ctx.set_option("trk_lazy_chi2", 1)
        with torch.cuda.stream(stream):
            oc1.step(); oc1.step()
            lat_quick["stage_ms"] = {k_: round(v_, 4) for k_, v_ in oc1.fe.stageTimes().items()}
        oc1.close()
        print(json.dumps({"quick": True, "latency_B1_ms": lat_quick, "lib": os.path.basename(capi.LIB_PATH), "value": round(fps, 1), "ms_per_step": round(t_front / K * 1e3, 4),
                          "ms_per_step_f64_accept": round(t_front_f64_accept / K * 1e3, 4), "ms_per_step_terms_stored_f64_accept": round(t_front_terms_only / K * 1e3, 4), "ms_per_step_stream_order": round(t_front_stream_order / K * 1e3, 4),
                          "ms_one_stream": round(ms_one_stream, 4), "exact_sums_per_frame": round(exact_sums_per_frame, 2), "fallbacks": exact_fallbacks,
                          "stage_ms": {k_: round(v_, 4) for k_, v_ in stage_ms.items()}, "track_err": track_err, "passes": passes}))
        if os.environ.get("SVS_BENCH_GROUPS"):                  # experiment: "2x512,4x512"
            for spec in os.environ["SVS_BENCH_GROUPS"].split(","):
                g_, s_ = (int(v) for v in spec.split("x"))
                print(json.dumps(run_groups(g_, s_)), flush=True)
        oc.close()
        return
    # dense-tracker bytes from the per-level record of the LM loop (sweeps per level, per stream), SURVEY 8d: 33 B per quarter-grid sample and sweep
    lvl_px = [(cam["w"] >> l) * (cam["h"] >> l) for l in range(3)]
    sweeps_lvl = np.zeros(3)
    for b in range(min(B, NPAIR)):
        rec = oc.fe.denseRecords(b)
        for l in range(3):
            sweeps_lvl[l] += int((rec["level"] == l).sum())
    sweeps_lvl /= min(B, NPAIR)
    # serial work of each stream's tracker (one workgroup per stream in throughput mode): sweeps x samples per level, in units of one level-0 sweep
    cost_units = []
    cost_prev = []
    for b in range(min(B, NPAIR)):
        rec = oc.fe.denseRecords(b)
        cost_units.append(round(float(sum(int((rec["level"] == l).sum()) * (lvl_px[l] // 16) for l in range(3))) / (lvl_px[0] // 16), 2))
    # the same one step further (the other direction of the ping-pong): how well one frame's work predicts the next frame's (the balanced launch relies on it)
    oc.step(); ctx.sync()
    for b in range(min(B, NPAIR)):
        rec = oc.fe.denseRecords(b)
        cost_prev.append(round(float(sum(int((rec["level"] == l).sum()) * (lvl_px[l] // 16) for l in range(3))) / (lvl_px[0] // 16), 2))
    oc.step(); ctx.sync()                                # back to the parity the rest of the bench expects
    work_corr = float(np.corrcoef(cost_units, cost_prev)[0, 1]) if len(cost_units) > 2 else None
    px = sum(lvl_px)
    alg = {
        "preprocess": lvl_px[0] + lvl_px[1] + lvl_px[2],      # W H read + W H / 4 + W H / 16 written = 403 200 B per 640 x 480 frame (the caller's frame is read ONCE:
                                                               # the first pyramid step also stores it into the library's level-0 buffer -- that copy-through, W H more bytes written, is not algorithmic)
        "dense_tracking": int(sum(sweeps_lvl[l] * (lvl_px[l] // 16) * (16 + 1 + 16) for l in range(3))),   # cloud float4 + prev u8 + 4x4 u8 taps per sample and sweep
        "fast": px + 4 * n_corners + 22 * 4,
        "match": n_points * (60 + 121 + 20) + n_points * 10 * 64,
        "pose_refinement": 64 * n_matched,                      # the matched records, read once (they stay in registers for all LM trials)
        "process_points": n_points * (64 + 64 + 40),
        "pointcloud": (px // 16) * 20,
    }
    oc.close()
    # the stereo-input path (New College: no disparity image, calcDisparityCpu = cv::StereoBM inside the step)
    ocs = OneCall(B, block_matching=True)
    t_stereo = max_over_ranks(timed_steps(ocs, 2, max(4, K // 2 * 2)))
    fps_stereo = world * B * max(4, K // 2 * 2) / t_stereo
    ocs.fe.setTiming(True)
    st_acc = {}
    with torch.cuda.stream(stream):
        for _ in range(4):
            ocs.step()
            for k_, v_ in ocs.fe.stageTimes().items():
                st_acc.setdefault(k_, []).append(v_)
    stage_ms_stereo = {k_: float(np.mean(v_)) for k_, v_ in st_acc.items()}
    ocs.close()
    alg["stereo"] = lvl_px[0] * (2 + 4)                          # left + right u8 in, f32 disparity out
    stage_ms_roof = dict(stage_ms, stereo=stage_ms_stereo["stereo"])
    roofline_frontend = {k: {"ms": round(stage_ms_roof[k], 4), "alg_bytes_per_frame": int(alg[k]),
                             "achieved_GBs": round(alg[k] * B / (stage_ms_roof[k] * 1e-3) / 1e9, 2),
                             "frac": round(alg[k] * B / (stage_ms_roof[k] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)} for k in alg}
    # block matcher quality on one pair (its disparity against the renderer's), through the staged API
    cur = FramePyramid(ctx, stream, cam, batch=1, with_float=False)
    cur.upload(rend_cur[0][0][None])
    stereo = StereoMatcher(ctx, cur)
    stereo.upload_right(rend_right[0][None])
    stereo.calcDisparityCpu()
    d_bm = stereo.disparity_host(0)
    d_gt = rend_cur[0][1]
    bm_valid = d_bm >= 0
    stereo_info = {"valid_fraction": round(float(bm_valid.mean()), 4),
                   "median_abs_err_px_vs_true_disparity": round(float(np.median(np.abs(d_bm - d_gt)[bm_valid])), 4)}
    stereo.close()

    # latency mode: one camera stream per call, frames resident (same one-call path, B = 1)
    oc1 = OneCall(1)
    lat_ms = timed_steps(oc1, 4, 20) / 20 * 1e3
    oc1.fe.setTiming(True)
    with torch.cuda.stream(stream):
        oc1.step(); oc1.step()
        lat_stages = {k_: round(v_, 4) for k_, v_ in oc1.fe.stageTimes().items()}
    oc1.close()
    # the drop-in call: StereoFrontend::processFrame for one stream, HOST image + disparity in, HOST pose / match records / gate records /
    # statistics out (svs_frontend_process_frame: pinned staging, one upload, the same kernels, one download) -- PCIe-inclusive latency
    T_kf = T_prev_list[0]
    pts = pts_of_pair[0]
    sfe = StereoFrontend(ctx, cam, max_points=max(args.points, 1), max_keyframes=1)
    sfe.processFirstFrame(rend_prev[0][0], disp=rend_prev[0][1])
    sfe.keepKeyframe(0, T_kf)
    sfe.setCandidates(pts, len(pts) // 2)
    seq = [(rend_cur[0], I34, T_AB[0]), (rend_prev[0], T_AB[0].reshape(12), np.hstack([np.eye(3), np.zeros((3, 1))]))]      # B, A, B, A ...: (frame, guess, true pose)
    host_ms = []
    for it in range(16):
        (img_, disp_), guess_, true_ = seq[it & 1]
        t0 = time.perf_counter()
        fres, fm, fg = sfe.processFrame(img_, guess_, T_kf, disp=disp_)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    host_io_ms = float(np.median(host_ms[4:]))
    host_dev = float(np.abs(np.array(fres.T_cur_from_actkey).reshape(3, 4) - np.asarray(true_).reshape(3, 4)).max())
    # the same with the next frame's upload overlapped (svs_frontend_prefetch_frame between submit and wait): the reference's FrameData double buffer
    ov_ms = []
    sfe.prefetchFrame(seq[0][0][0], disp=seq[0][0][1])
    for it in range(16):
        (img_, disp_), guess_, true_ = seq[it & 1]
        nxt = seq[(it + 1) & 1][0]
        t0 = time.perf_counter()
        sfe.submitFrame(None, guess_, T_kf)
        sfe.prefetchFrame(nxt[0], disp=nxt[1])
        fres2, _, _ = sfe.waitFrame()
        ov_ms.append((time.perf_counter() - t0) * 1e3)
    sfe.processFrame(None, seq[0][1], T_kf)      # consume the last prefetch
    host_ov_ms = float(np.median(ov_ms[4:]))
    host_io = {"ms_per_frame": round(host_io_ms, 4), "frames_per_s": round(1e3 / host_io_ms, 1),
               "ms_per_frame_next_upload_overlapped": round(host_ov_ms, 4), "matched": int(fres.n_matched),
               "dense_passes": int(fres.dense_passes), "bytes_in": int(cam["w"] * cam["h"] * 5), "bytes_out": int(len(pts) * (64 + 40) + 600),
               "pose_dev_from_true_motion": host_dev}
    sfe.close()
    # the reference's other shipped configuration: New College 512 x 384 (data/newcollege.cfg:1-6), the same step at the same batch
    nc_row = None
    if world == 1:
        INP_NC = make_inputs(synth.CAM_NEWCOLLEGE, min(NPAIR, 16), with_right=False)
        ocn = OneCall(B, inp=INP_NC)
        t_nc = timed_steps(ocn, 2, K + (K & 1))
        Tn, okn = ocn.fe.poses()
        fl = ocn.k & 1
        nc_err = float(max(np.abs(Tn[b] - np.asarray([I34, INP_NC["T_AB"][b % INP_NC["npair"]].reshape(12)][fl]).reshape(3, 4)).max() for b in range(min(B, INP_NC["npair"]))))
        ocn.fe.setTiming(True)
        acc = {}
        with torch.cuda.stream(stream):
            for _ in range(4):
                ocn.step()
                for k_, v_ in ocn.fe.stageTimes().items():
                    acc.setdefault(k_, []).append(v_)
        ocn.fe.setTiming(False)
        nc_row = {"frame": "512x384 (data/newcollege.cfg:1-6: f 389.956, c (254.903, 201.899), b 0.120005)", "batch_streams": B,
                  "frames_per_s": round(B * (K + (K & 1)) / t_nc, 1), "ms_per_step": round(t_nc / (K + (K & 1)) * 1e3, 4),
                  "stage_ms_per_batch": {k_: round(float(np.mean(v_)), 4) for k_, v_ in acc.items()}, "tracking_ok_fraction": float(okn.mean()),
                  "refined_pose_err_vs_true_motion": nc_err}
        ocn.close()
        del INP_NC
    # the reference's concurrency (stereo_slam.cpp:196, backend.cpp:157-224,735-779): processFrame loop on one thread, optimize + re-registration on another,
    # separate contexts, one GPU (tools/two_threads.py; tests/test_gpu_concurrency.py holds the results equal to the serial runs)
    two_threads = None
    if world == 1:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import two_threads as TT
        sf_, sb_, cf_, cb_, errs_, wall_ = TT.run_serial_and_concurrent(n_frames=600, n_rounds=96, device=local_rank)
        two_threads = dict(TT.summarize(sf_, sb_, cf_, cb_, wall_), errors=errs_,
                           note="latency-mode svs_frontend_process_frame (host buffers in and out) on thread A; svs_ba_optimize of the 50 KF / 20 k window every round and of "
                                "the 230-pose double window with loop closures + 180-observation landmarks (multi-workgroup Cholesky) every 4th round, plus FastGrid::detect "
                                "+ GuidedMatcher::match per round on thread B; 'alone' = each loop run by itself first")
    # batched modes in between (B in {1, 8, 64}): same step, B independent streams per call
    batch_sweep = {"1": round(1e3 / lat_ms, 1), str(B): round(fps / world, 1)}
    for Bs in (8, 64, 256):
        if Bs >= B:
            continue
        ocb = OneCall(Bs)
        batch_sweep[str(Bs)] = round(Bs * 10 / timed_steps(ocb, 2, 10), 1)
        ocb.close()
    # several batched front ends in flight on their own HIP streams (run_groups above): the stage kernels of different groups overlap -- the mode a
    # multi-camera server would run; `value` stays the single batch, whose stage times add up
    overlapped = None
    if B >= 512 and world == 1:
        overlapped = run_groups(2, B)
    # the reference's CUDA build of the same path (full-resolution tracker, matcher radius 4) through the same call
    FBc = min(B, 64)
    occ = OneCall(FBc, cuda_build=True)
    t_cuda = timed_steps(occ, 2, 6)
    cuda_path = {"streams_per_call": FBc, "ms_per_step": round(t_cuda / 6 * 1e3, 4), "frames_per_s": round(FBc * 6 / t_cuda, 1)}
    occ.close()

    # ------------------------------------------------------------------ BASELINE config 5: RGB-D full-resolution dense tracking
    # DenseTracker::denseTrackingGpu (dense_tracking.cpp:60-193) for FB independent 640x480 RGB-D streams per launch: CUDA-branch
    # preprocessing done, clouds resident; a step = the whole coarse-to-fine damped LM.  Algorithmic bytes per SURVEY 8d: 32 B per
    # pixel per sweep of a level (the fused sweep yields chi2 AND H,b; the reference reads 24 + 32 B/px for the same pair).
    from scavislam_amd.frontend import DenseTrackerGpu, GpuFrameData
    FB = args.full_batch
    camd = synth.CAM_RGBD
    NFP = min(NPAIR, 8)
    hrng = np.random.default_rng(2013)
    fprev = GpuFrameData(ctx, stream, camd, FB)
    fcur = GpuFrameData(ctx, stream, camd, FB)
    fr_prev = [scene.render(camd, T_prev_list[p], seed=300 + p) for p in range(NFP)]
    fr_cur = [scene.render(camd, T_cur_list[p], seed=400 + p) for p in range(NFP)]
    disp_holes = [synth.depth_holes(fr_prev[p][1], hrng) for p in range(NFP)]          # 10 % invalid depth in blobs
    fprev.upload(np.stack([fr_prev[b % NFP][0] for b in range(FB)]))
    fcur.upload(np.stack([fr_cur[b % NFP][0] for b in range(FB)]))
    fprev.preprocessing(); fcur.preprocessing()
    dfull = DenseTrackerGpu(ctx, fcur)
    clouds_full = [[synth.cloud_full_level(disp_holes[p], camd, l) for l in range(3)] for p in range(NFP)]
    with torch.cuda.stream(stream):
        for l in range(3):
            dfull.dev_ref_dense_points[l].copy_(torch.as_tensor(np.stack([clouds_full[b % NFP][l] for b in range(FB)])))
    fargs = dfull.track_args(fprev)
    T_f, sweeps_f, rec_f = dfull.denseTrackingGpu(fprev, I34, args=fargs)
    full_err = float(max(np.abs(T_f[b] - synth.pose_mul(T_cur_list[b % NFP], synth.pose_inv(T_prev_list[b % NFP]))).max() for b in range(min(FB, NFP))))
    full_bytes = sum(32 * (camd["w"] >> l) * (camd["h"] >> l) * int((rec_f[b]["level"] == l).sum()) for b in range(FB) for l in range(3))
    with torch.cuda.stream(stream):
        d_T0f = torch.as_tensor(np.tile(I34, (FB, 1))).to(dev)
        ms_full = []
        for _ in range(2 + min(K, 10)):
            dfull.d_T.copy_(d_T0f)
            ctx.sync()
            ctx.timer_start()
            dfull.denseTrackingGpu(fprev, None, args=fargs, download=False)
            ms_full.append(ctx.timer_stop_ms())
        ms_full = float(np.median(ms_full[2:]))
        # latency mode: one stream per launch
        f1p, f1c = GpuFrameData(ctx, stream, camd, 1), GpuFrameData(ctx, stream, camd, 1)
        f1p.upload(fr_prev[0][0][None]); f1c.upload(fr_cur[0][0][None])
        f1p.preprocessing(); f1c.preprocessing()
        d1 = DenseTrackerGpu(ctx, f1c)
        for l in range(3):
            d1.dev_ref_dense_points[l].copy_(torch.as_tensor(clouds_full[0][l][None]))
        a1 = d1.track_args(f1p)
        ms1 = []
        for _ in range(12):
            d1._set_T(I34)
            ctx.sync()
            ctx.timer_start()
            d1.denseTrackingGpu(f1p, None, args=a1, download=False)
            ms1.append(ctx.timer_stop_ms())
        ms_full_b1 = float(np.median(ms1[2:]))
    dense_full = {"workload": "configs[4]: RGB-D dense_tracking, 640x480 depth frames, full resolution, 3 levels, damped LM (denseTrackingGpu)",
                  "streams_per_launch": FB, "ms_per_launch": round(ms_full, 4), "frames_per_s": round(world * FB / (ms_full * 1e-3), 1),
                  "sweeps_per_frame": {"mean": round(float(sweeps_f.mean()), 2), "min": int(sweeps_f.min()), "max": int(sweeps_f.max())},
                  "reference_kernel_passes_for_the_same_trajectories": round(float(np.mean([6 + 2 * int((r["accepted"] < 2).sum()) for r in rec_f])), 1),
                  "pose_err_vs_true_motion": full_err,
                  "latency_mode_B1_ms_per_frame": round(ms_full_b1, 4),
                  "roofline": {"bound": "hbm", "kernel": "dense_track_full_kernel (whole LM in one launch; 32 B/px per fused chi2+H,b sweep)",
                               "alg_bytes_per_launch": int(full_bytes), "avg_launch_ms": round(ms_full, 4),
                               "achieved": round(full_bytes / (ms_full * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(full_bytes / (ms_full * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}
    del dfull, fprev, fcur, d1, f1p, f1c
    torch.cuda.empty_cache()

    _probe_windows('before the back-end region')
    # ------------------------------------------------------------------ back-end (Schur) region
    P_, L_ = 50, 20000
    prob = synth.ba_window(P_, L_, seed=2012)
    camc = Cam(*(prob["cam"][k] for k in ("f", "cx", "cy", "b", "w", "h")))
    prm = BaParams.reference_defaults()
    sh = shard_problem(prob, rank, world) if world > 1 else dict(prob, add_pose_terms=True)
    opt = SlamGraphOptimizer(ctx, stream)
    opt.copyDataToG2o(sh["poses"], sh["psi"], sh["edges"], sh["cons"], camc, prm, add_pose_terms=sh["add_pose_terms"])
    # sharded runs: the library's own RCCL communicator (ncclAllReduce on the ctx stream inside svs_ba_optimize); torch.distributed
    # only carries the 128-byte unique id to the other ranks.  Also exercised at one rank when launched through torch.distributed.run.
    comm, allreduce, comm_error = None, None, None
    if use_dist:
        try:
            with _stdout_to_stderr():
                comm = Communicator(ctx, rank, world, device=dev)
        except Exception as e:                                # e.g. librccl cannot be bound in this environment
            comm_error = repr(e)
        ok = torch.tensor([0 if comm is None else 1], dtype=torch.int32, device=dev)
        if world > 1:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)        # every rank takes the same path
        if int(ok.item()) == 1:
            opt.set_comm(comm)
        else:                                                 # safety net: the collective through torch.distributed (also RCCL), as a callback
            if comm is not None:
                comm.close()
                comm = None
            from scavislam_amd.backend import make_allreduce
            allreduce = make_allreduce(stream, local_rank)
            print("bench: library communicator unavailable (%s); all-reduce through torch.distributed" % comm_error, file=sys.stderr)
    E_total, E_local = len(prob["edges"]), len(sh["edges"])
    stats = None
    t_red = t_sol = t_bs = 0.0
    n_tr = 0
    with torch.cuda.stream(stream):
        for _ in range(W):
            opt.reset_state(sh["poses"], sh["psi"])
            opt.optimize(allreduce)
        barrier_sync()
        t_ba = 0.0
        for _ in range(K):
            opt.reset_state(sh["poses"], sh["psi"])        # untimed: restore the window
            barrier_sync()
            t0 = time.perf_counter()
            stats = opt.optimize(allreduce)
            barrier_sync()
            t_ba += time.perf_counter() - t0
        # second pass over the same K calls with hipEvent brackets around the Schur / solve / back-substitution kernels
        # (the roofline's launch duration).  Kept out of the first pass: an event record costs ~4 us of stream time,
        # 12 of them are ~15 % of an optimize() at this size.
        opt.set_timing(True)
        t_ba_ev = 0.0
        for _ in range(K):
            opt.reset_state(sh["poses"], sh["psi"])
            barrier_sync()
            t0 = time.perf_counter()
            opt.optimize(allreduce)
            barrier_sync()
            t_ba_ev += time.perf_counter() - t0
            kt = opt.kernel_times()
            t_red += kt["reduce_ms"]; t_sol += kt["solve_ms"]; t_bs += kt["backsub_ms"]; n_tr += kt["n_trials"]
        opt.set_timing(False)
    # the same K optimizes over the second transport of svs_comm: the one-shot P2P exchange (peer-mapped mailboxes, comm.hip) instead of RCCL's ring.
    # One rank per GPU here, so this row is only comparable with the RCCL row on a multi-GPU node; at one rank both transports are identities.
    ba_p2p = None
    if use_dist and comm is not None:
        comm2, p2p_error = None, None
        try:
            with _stdout_to_stderr():
                comm2 = Communicator.p2p(ctx, rank, world, capacity_doubles=1 << 17, device=dev)      # the 64-byte IPC handles travel over the default (nccl) group
                                                                                                     # (succeeds or raises on ALL ranks together)
        except Exception as e:
            p2p_error = repr(e)
        ok = torch.tensor([0 if comm2 is None else 1], dtype=torch.int32, device=dev)
        if world > 1:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            opt.set_comm(comm2)
            with torch.cuda.stream(stream):
                for _ in range(2):
                    opt.reset_state(sh["poses"], sh["psi"])
                    opt.optimize()
                t_p2p = 0.0
                for _ in range(K):
                    opt.reset_state(sh["poses"], sh["psi"])
                    barrier_sync()
                    t0 = time.perf_counter()
                    st2 = opt.optimize()
                    barrier_sync()
                    t_p2p += time.perf_counter() - t0
            ba_p2p = {"ms_per_optimize": round(max_over_ranks(t_p2p) / K * 1e3, 4), "same_lm_trajectory_as_rccl": bool((st2.trials, st2.accepted) == (stats.trials, stats.accepted)),
                      "chi2_final": st2.chi2_final, **comm2.transport(), **{k: v for k, v in comm2.stats().items() if k in ("n_calls", "n_doubles")}}
            opt.set_comm(comm)
        else:
            ba_p2p = {"error": p2p_error or "unavailable on another rank"}
        if comm2 is not None:
            barrier_sync()
            comm2.close()
    t_ba = max_over_ranks(t_ba)
    ms_opt = t_ba / K * 1e3
    ms_opt_ev = max_over_ranks(t_ba_ev) / K * 1e3
    _probe_windows('after the main optimize rows (communicators)')
    # the drop-in call pattern: host arrays in (marshalling + upload), optimize, host arrays out -- what SlamGraph::optimize costs a caller
    e2e_ms = None
    if world == 1:
        with torch.cuda.stream(stream):
            for rep in range(2 + min(K, 10)):
                if rep == 2:
                    ctx.sync()
                    t0 = time.perf_counter()
                opt.copyDataToG2o(sh["poses"], sh["psi"], sh["edges"], sh["cons"], camc, prm, add_pose_terms=True)
                opt.optimize(None)
                opt.restoreDataFromG2o()
            e2e_ms = (time.perf_counter() - t0) / min(K, 10) * 1e3
    # other window shapes + throughput mode (rank 0 at N = 1 only; each is one optimize() of a resident window, state restored untimed)
    schur_rows = None
    if world == 1:
        from scavislam_amd.backend import optimize_batch
        schur_rows = {}

        def time_window(name, pr, reps=10):
            o = SlamGraphOptimizer(ctx, stream)
            cm = Cam(*(pr["cam"][k] for k in ("f", "cx", "cy", "b", "w", "h")))
            t_e2e = []
            with torch.cuda.stream(stream):
                for rep in range(reps + 2):
                    t0 = time.perf_counter()
                    o.copyDataToG2o(pr["poses"], pr["psi"], pr["edges"], pr["cons"], cm, prm)
                    st_ = o.optimize()
                    o.restoreDataFromG2o()
                    t_e2e.append(time.perf_counter() - t0)
                t_opt = []
                for rep in range(reps):
                    o.reset_state(pr["poses"], pr["psi"])
                    ctx.sync()
                    t0 = time.perf_counter()
                    o.optimize()
                    ctx.sync()
                    t_opt.append(time.perf_counter() - t0)
            row = dict(keyframes=len(pr["poses"]), landmarks=int(np.unique(pr["edges"]["point"]).size), edges=len(pr["edges"]), constraints=len(pr["cons"]),
                       ms_per_optimize=round(float(np.median(t_opt)) * 1e3, 4),
                       ms_per_call_incl_host_marshalling_and_copies=round(float(np.median(t_e2e[2:])) * 1e3, 4),
                       lm_trials=int(st_.trials), **o.info())
            o.close()
            schur_rows[name] = row
        other_probs = {"15KF_3k (configs[2])": synth.ba_window(15, 3000, seed=2012),
                       "double_window_30_inner_200_outer": synth.double_window(n_inner=30, n_outer=200, L=12000, seed=2014, n_long=(100, 180, 70), n_loops=2),
                       "double_window_30_inner_200_outer_loop_closures_only": synth.double_window(n_inner=30, n_outer=200, L=12000, seed=2014, n_long=(), n_loops=2),
                       "double_window_30_inner_200_outer_no_loop_closure": synth.double_window(n_inner=30, n_outer=200, L=12000, seed=2014, n_long=(), n_loops=0)}
        for name_, pr_ in other_probs.items():
            time_window(name_, pr_)
        # throughput mode: W independent 50 KF / 20k windows in flight (svs_ba_optimize_batch, one context = one stream per window)
        by_w = {"1": round(1e3 / ms_opt, 1)}
        for Wn in (8, 32):
            # library-owned streams (hipStreamCreate): torch hands out its streams from a pool of 32 per device, so a 33rd torch stream IS an earlier one and two
            # windows would share (and serialise on) it -- that, not the library, was the batch-32 figure of round 3 (5.8 k windows/s)
            ctxs_w = [(capi.Context(local_rank), None) for _ in range(Wn)]
            opts_w = []
            for cw, sw in ctxs_w:
                ow = SlamGraphOptimizer(cw, sw)
                ow.copyDataToG2o(prob["poses"], prob["psi"], prob["edges"], prob["cons"], camc, prm)
                opts_w.append(ow)
            tt = []
            # 16 repetitions, the median of the last 8.  The figure depends on how the runtime maps these 32 streams onto its hardware queues (4 per process by
            # default): 10.4-11.5 k windows/s in a fresh process or when the streams are created before the front end's (which then loses a fifth of ITS throughput), 6-8 k
            # created here, 8.7 k with GPU_MAX_HW_QUEUES=16 -- same library, same kernels (profiles/r6_notes.md section 5)
            for rep in range(16):
                for ow in opts_w:
                    ow.reset_state(prob["poses"], prob["psi"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                optimize_batch(opts_w)
                tt.append(time.perf_counter() - t0)
            by_w[str(Wn)] = round(Wn / float(np.median(tt[8:])), 1)
            if os.environ.get("SVS_BENCH_DEBUG"):
                print(f"[bench] windows in flight {Wn}: ms per batch {[round(t * 1e3, 3) for t in tt]}, graph stats {opts_w[0].graph_stats()}, {opts_w[0].info()}", file=sys.stderr)
            for ow in opts_w:
                ow.close()
            for cw, _ in ctxs_w:
                cw.close()
        schur_rows["windows_per_s_by_batch_50KF_20k"] = by_w
    # the persistent window: the steady-state call of a sliding window -- the library already holds the observations of
    # the 49 older keyframes; the call brings ids, current values, the newest keyframe's observations, then optimize + read-back
    persistent_ms = None
    if world == 1:
        ow = SlamGraphOptimizer(ctx, stream)
        pe = prob["edges"]
        newest = pe["pose"] == pe["pose"].max()              # the newest keyframe that observes points (the last three are outer-window poses)
        anchor_of = np.zeros(len(prob["psi"]), np.int32)
        anchor_of[pe["point"]] = pe["anchor"]
        seen = np.zeros(len(prob["psi"]), bool)
        seen[pe["point"]] = True
        act = np.nonzero(seen)[0].astype(np.int32)
        ids_p = np.arange(P_, dtype=np.int32)
        # the caller's arrays exist before the call (as for the drop-in row above): no NumPy gathers inside the timed region
        psi_act, anch_act = np.ascontiguousarray(prob["psi"][act]), np.ascontiguousarray(anchor_of[act])
        obs_hist, obs_new = np.ascontiguousarray(pe[~newest]), np.ascontiguousarray(pe[newest])
        tt = []
        with torch.cuda.stream(stream):
            for rep in range(8):
                ow.windowReset()
                ow.windowUpdate(ids_p, prob["poses"], act, psi_act, anch_act, obs_hist, prob["cons"], camc, prm)    # untimed: history
                ctx.sync()
                t0 = time.perf_counter()
                ow.windowUpdate(ids_p, prob["poses"], act, psi_act, anch_act, obs_new, prob["cons"], camc, prm)
                st_w = ow.optimize()
                ow.restoreDataFromG2o()
                tt.append(time.perf_counter() - t0)
        persistent_ms = float(np.median(tt[2:])) * 1e3
        persistent_info = dict(ow.info(), new_observations=int(newest.sum()), lm_trials=int(st_w.trials), chi2_final=st_w.chi2_final)
        ow.close()
    # weak-scaling row: every rank optimises its own complete 50 KF / 20k window, no collective
    schur_weak = None
    if world > 1:
        optw = SlamGraphOptimizer(ctx, stream)
        optw.copyDataToG2o(prob["poses"], prob["psi"], prob["edges"], prob["cons"], camc, prm, add_pose_terms=True)
        with torch.cuda.stream(stream):
            for _ in range(W):
                optw.reset_state(prob["poses"], prob["psi"])
                optw.optimize(None)
            t_w = 0.0
            for _ in range(K):
                optw.reset_state(prob["poses"], prob["psi"])
                barrier_sync()
                t0 = time.perf_counter()
                optw.optimize(None)
                barrier_sync()
                t_w += time.perf_counter() - t0
        t_w = max_over_ranks(t_w)
        schur_weak = {"windows_per_s_all_gpus": round(world * K / t_w, 1), "ms_per_optimize_per_gpu": round(t_w / K * 1e3, 4),
                      "scaling": "weak", "note": "one full 50 KF / 20k window per GPU, no collective"}
    # ... and SURVEY 8e's row proper: ONE window that grows with the node -- 50 keyframes, 20 k landmarks PER GPU, sharded, the reduced system all-reduced by the
    # library's communicator (RCCL) as in the strong-scaling run above
    if world > 1 and comm is not None:
        prob_g = synth.ba_window(P_, L_ * world, seed=2012)
        sh_g = shard_problem(prob_g, rank, world)
        optg = SlamGraphOptimizer(ctx, stream)
        optg.copyDataToG2o(sh_g["poses"], sh_g["psi"], sh_g["edges"], sh_g["cons"], camc, prm, add_pose_terms=sh_g["add_pose_terms"])
        optg.set_comm(comm)
        with torch.cuda.stream(stream):
            for _ in range(W):
                optg.reset_state(sh_g["poses"], sh_g["psi"])
                optg.optimize(None)
            t_g = 0.0
            for _ in range(K):
                optg.reset_state(sh_g["poses"], sh_g["psi"])
                barrier_sync()
                t0 = time.perf_counter()
                st_g = optg.optimize(None)
                barrier_sync()
                t_g += time.perf_counter() - t0
        t_g = max_over_ranks(t_g)
        schur_weak["sharded_window"] = {"keyframes": P_, "landmarks": L_ * world, "landmarks_per_gpu": L_, "edges": len(prob_g["edges"]), "edges_this_rank": len(sh_g["edges"]),
                                        "ms_per_optimize": round(t_g / K * 1e3, 4), "lm_trials": int(st_g.trials), "chi2_final": st_g.chi2_final,
                                        "transport": "RCCL ncclAllReduce(ncclDouble) issued by the library"}
        optg.close()
        del prob_g, sh_g
    red_ms = t_red / max(n_tr, 1)
    # algorithmic bytes of the Schur (landmark) kernel: edges + psi read once, packed system written once
    nblk = P_ * (P_ + 1) // 2
    n_lm_local = int(np.unique(sh["edges"]["point"]).size)
    alg_schur = 64 * E_local + 24 * n_lm_local + 8 * (36 * nblk + 12 * P_ + 1)
    achieved = alg_schur / (red_ms * 1e-3) / 1e9 if red_ms > 0 else 0.0
    # SURVEY.md 8(d), "Schur step" row: one LM trial = linearise + accumulate + reduce + back-substitute: 2 (64 E + 24 L) + 24 L + 8 (36 P(P+1)/2 + 6 P)  (14.6 MB at 50 / 20 k)
    schur_step_bytes = 2 * (64 * E_local + 24 * n_lm_local) + 24 * n_lm_local + 8 * (36 * nblk + 6 * P_)
    roofline = {"bound": "hbm", "kernel": "ba_landmark_kernel<0> (linearise + 3x3 inverse + Schur outer products)",
                "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5), "frac_of_measured_copy_ceiling": round(achieved / 6290.0, 5),
                "alg_bytes_per_launch": int(alg_schur), "avg_launch_ms": round(red_ms, 5),
                "traffic": None, "traffic_source": None}
    # HBM bytes per launch come from rocprofv3 PMC passes (they cannot be collected inside this process): profiles/pmc_latest.json holds
    # them per kernel together with the hash of the kernel's source at profiling time -- reported only while that source is unchanged
    # and the workload is the profiled one.
    def pmc_traffic(key, workload_ok):
        import hashlib
        try:
            pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))["kernels"][key]
            cur = hashlib.sha256(open(os.path.join(ROOT, pj["source"]), "rb").read()).hexdigest()[:16]
            if cur == pj["source_sha16"] and workload_ok(pj["workload"]):
                return pj["traffic"], f"profiles/pmc_latest.json ({pj['correction']})"
        except Exception:
            pass
        return None, "profiles/pmc_latest.json is missing, or the kernel source / workload changed since it was taken"
    roofline["traffic"], roofline["traffic_source"] = pmc_traffic("ba_landmark_kernel<0>", lambda wl: world == 1 and wl.get("edges") == E_local)
    df_traffic, df_src = pmc_traffic("dense_track_full_kernel", lambda wl: wl.get("streams_per_launch") == FB)
    if df_traffic is not None:      # measured on the same kernel at the same batch but other frames: carried over as the ratio to algorithmic bytes
        ratio = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))["kernels"]["dense_track_full_kernel"].get("traffic_over_algorithmic")
        df_traffic = int(ratio * dense_full["roofline"]["alg_bytes_per_launch"]) if ratio else None
    dense_full["roofline"]["traffic"], dense_full["roofline"]["traffic_source"] = df_traffic, df_src
    # the front-end stages: raw FETCH_SIZE + WRITE_SIZE of each stage's dominant kernel in the launch over the whole batch (same file, same rule: only while the
    # kernel's source is unchanged and the batch is the profiled one).  Raw counters -- 16 B/lane loads count half there (MI355X_MICROARCH.md), so this is a lower
    # bound of the bytes moved; `traffic_over_alg` = that / the stage's algorithmic bytes.
    try:
        import hashlib
        pk = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))["kernels"]
        for stage_, key_ in (("preprocess", "pyr_down_u8_kernel"), ("dense_tracking", "dense_track_cpu_sem_kernel"), ("fast", "fast_score_kernel"), ("match", "match_kernel3"),
                             ("pose_refinement", "motion_only_fused_kernel"), ("stereo", "stereo_bm_kernel")):
            pj = pk.get(key_)
            if not pj or pj["workload"].get("batch_streams_per_gpu") != B:
                continue
            if hashlib.sha256(open(os.path.join(ROOT, pj["source"]), "rb").read()).hexdigest()[:16] != pj["source_sha16"]:
                continue
            raw = int(pj["fetch_raw"] + pj["write_raw"])
            roofline_frontend[stage_]["dominant_kernel"] = pj["kernel"]
            roofline_frontend[stage_]["dominant_kernel_fetch_plus_write_raw_bytes_per_batch"] = raw
            alg_ = roofline_frontend[stage_]["alg_bytes_per_frame"]
            if stage_ == "pose_refinement":      # in the default schedule this kernel also runs the gate and writes the three dense clouds (fe_fuse_tail): their bytes belong to it
                alg_ += roofline_frontend["process_points"]["alg_bytes_per_frame"] + roofline_frontend["pointcloud"]["alg_bytes_per_frame"]
                roofline_frontend[stage_]["dominant_kernel_note"] = "the fused kernel = refinement + gate + clouds: ratio against the three stages' algorithmic bytes"
            roofline_frontend[stage_]["dominant_kernel_raw_traffic_over_stage_alg"] = round(raw / (alg_ * B), 3)
    except Exception:
        pass

    # ------------------------------------------------------------------ CPU baseline (oracle, rank 0, N=1)
    cpu = None
    cpu_schur_ms = None
    if rank == 0 and world == 1 and not args.no_cpu:      # the contract: rank 0 at N=1 only
        import oracle as O
        from scavislam_amd.ctypes_types import PoseOptParams, level_cams as level_cams_c
        cams_c = level_cams_c(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
        lw, lh = [cam["w"] >> l for l in range(3)], [cam["h"] >> l for l in range(3)]
        grids = [O.fastgrid_for_level(lw[l], lh[l], l) for l in range(3)]
        # state the reference also carries over from the previous frame (not timed): the active keyframe = frame A, its pyramid and cloud
        pyr_p_cache = {p: O.build_pyramid(rend_prev[p][0]) for p in range(NPAIR)}
        clouds_cache = {p: [O.pointcloud_cpu(rend_prev[p][1], cams_c[l], l, I34.reshape(3, 4)) for l in range(3)]
                        for p in range(NPAIR)}
        t0 = time.perf_counter()
        nfr = 0
        while nfr < 3 or (time.perf_counter() - t0 < 8.0 and nfr < 200):      # BASELINE configs[0]: 200 frames
            p = nfr % NPAIR
            img_c, disp_c = rend_cur[p]
            T_kfp = T_prev_list[p]
            pyr_c = O.build_pyramid(img_c)                                      # "preprocess"
            fl = [O.convert_sobel(x) for x in pyr_c]
            Tt, _ = O.dense_tracking_cpu(clouds_cache[p], pyr_p_cache[p], [f[0] for f in fl], [f[1] for f in fl],
                                         [f[2] for f in fl], cams_c, I34.reshape(3, 4))     # "dense tracking"
            trees = []
            for l in range(3):                                                  # "fast"
                xy, cc, et = O.fastgrid_detect_adaptively(grids[l], pyr_c[l], 6)
                trees.append(O.quadtree_from_corners(xy, cc, lw[l], lh[l]))
            mres_c = O.match([pyr_p_cache[p]], [T_kfp.reshape(12)], Tt, T_kfp, pyr_c, disp_c, trees, cams_c, pts_of_pair[p])   # "match"
            if (mres_c["status"] == 0).sum() >= 20:
                Tm, _ = O.motion_only(mres_c, cams_c[0], Tt, PoseOptParams.reference())                                        # calcFastMotionOnly
                O.process_matched_points(mres_c, pts_of_pair[p], len(pts_of_pair[p]) // 2, cams_c[0], Tm, 2.0)                            # "process points"
            else:
                Tm = Tt
            [O.pointcloud_cpu(disp_c, cams_c[l], l, Tm) for l in range(3)]      # "dense point cloud"
            nfr += 1
        t_cpu = time.perf_counter() - t0
        cpu_fps = nfr / t_cpu
        t0 = time.perf_counter()
        nba = 0
        while nba < 2 or (time.perf_counter() - t0 < 6.0 and nba < 100):
            O.ba_optimize(prob["poses"], prob["psi"], prob["edges"], prob["cons"], camc, prm)
            nba += 1
        cpu_schur_ms = (time.perf_counter() - t0) / nba * 1e3
        # the other window shapes of the Schur table: every BA row gets its CPU time (bounded: >= 2 calls, <= 3 s each)
        for name_, pr_ in (other_probs.items() if schur_rows is not None else ()):
            cm_ = Cam(*(pr_["cam"][k] for k in ("f", "cx", "cy", "b", "w", "h")))
            t0 = time.perf_counter()
            nb_ = 0
            while nb_ < 2 or (time.perf_counter() - t0 < 3.0 and nb_ < 30):
                O.ba_optimize(pr_["poses"], pr_["psi"], pr_["edges"], pr_["cons"], cm_, prm)
                nb_ += 1
            ms_ = (time.perf_counter() - t0) / nb_ * 1e3
            schur_rows[name_]["cpu_port_ms_per_optimize"] = round(ms_, 2)
            schur_rows[name_]["speedup_vs_cpu_port"] = round(ms_ / schur_rows[name_]["ms_per_optimize"], 1)
            schur_rows[name_]["speedup_vs_cpu_port_drop_in_call"] = round(ms_ / schur_rows[name_]["ms_per_call_incl_host_marshalling_and_copies"], 1)
        # context: one build + Schur accumulation of the same window from 1 and from 8 host threads
        acc_ms = {}
        for nthr in (1, 8):
            O.ba_reduced_system_mt(nthr, prob["poses"], prob["psi"], prob["edges"], prob["cons"], camc, prm, 50.0)
            t0 = time.perf_counter()
            for _ in range(5):
                O.ba_reduced_system_mt(nthr, prob["poses"], prob["psi"], prob["edges"], prob["cons"], camc, prm, 50.0)
            acc_ms[str(nthr)] = round((time.perf_counter() - t0) / 5 * 1e3, 2)
        t0 = time.perf_counter()
        nst = 0
        while nst < 2 or (time.perf_counter() - t0 < 4.0 and nst < 12):     # "stereo" (cv::StereoBM restatement), timed on its own like the GPU stage
            O.stereo_bm(rend_cur[nst % NRIGHT][0], rend_right[nst % NRIGHT])
            nst += 1
        cpu_stereo_ms = (time.perf_counter() - t0) / nst * 1e3
        # the reference's OWN code timed beside it, as far as this image allows: oracle/_ref/libsvs_ref_seq.so is the reference's front-end loop compiled from
        # /root/reference (stereo_frontend.cpp:39-528,656-1065 + matcher + dense tracker + FastGrid; built where the reference exists, travels prebuilt) -- processFrame
        # per frame over the first frames of the BASELINE configs[0] sequence.  Its third-party calls (Eigen, Sophus, OpenCV FAST, VisionTools) are the oracle's
        # stand-ins, so this is the reference's control flow and data structures on stand-in algebra, not a build against the real libraries (absent).  The back end's
        # SlamGraph::optimize cannot be timed this way: its solver IS g2o, which is absent (libsvs_ref_slamgraph.so records the graph, it does not solve it).
        ref_compiled = None
        try:
            if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvs_ref_seq.so")):
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import seq_common as SQ
                rs = O.RefSequence(cams_c)
                ts = []
                t0 = time.perf_counter()
                for i_, (img_, disp_) in enumerate(SQ.frames("default", 200)):
                    r_ = rs.step(img_, disp_)
                    if i_ > 0:
                        ts.append(rs.last_step_s)
                    if not r_["ok"] or (time.perf_counter() - t0 > 10.0 and i_ >= 8):
                        break
                rs.close()
                ref_compiled = {"ms_per_processFrame": round(float(np.mean(ts)) * 1e3, 2), "frames": len(ts), "cores": 1,
                                "what": "StereoFrontend::processFrame of the reference compiled here from its own sources (oracle/_ref/libsvs_ref_seq.so; disparity given; "
                                        "FrameGrabber::preprocessing not included), third-party algebra = the oracle's stand-ins",
                                "gpu_frames_per_s_over_this": round(fps * float(np.mean(ts)), 1)}
        except Exception as e:
            ref_compiled = {"error": repr(e)}
        cpu = {"value": round(cpu_fps, 3), "unit": "frames/s", "cores": 1, "kind": "port", "reference_compiled": ref_compiled,
               "sample": f"{nfr} frames 640x480 through the CPU oracle (the same eight stages minus block matching, same inputs, disparity given)"
                         f" + {nba} x BA optimize 50KF/20k ({cpu_schur_ms:.1f} ms each); host has {os.cpu_count()} cores, 1 used",
               "schur_ms_per_optimize": round(cpu_schur_ms, 2), "stereo_bm_ms_per_frame": round(cpu_stereo_ms, 1),
               "stereo_bm_note": "naive scalar restatement of cv::StereoBM, NOT OpenCV's SIMD implementation (30-50x faster): no speed-up claim for this stage",
               "schur_accumulate_ms_by_host_threads": acc_ms}

    if rank == 0:
        out = {
            **headline,
            "value_stereo_input": round(fps_stereo, 2),
            "config": {"workload": "configs[1]+[3]: `value` = frames/s WITH THE DISPARITY IMAGE GIVEN (have_disp_img, RGB-D style input); with stereo input -- cv::StereoBM "
                                   "block matching inside the step -- it is `value_stereo_input` (about half).  StereoFrontend::processFrame as ONE library call for a "
                                   "batch of camera streams on 640x480 stereo frames resident in HBM -- all eight stages: preprocess (copy-in + pyramid), dense tracking (fused f32 + Sobel taps), stereo "
                                   "(disparity given for `value`; cv::StereoBM block matching inside the step for `value_stereo_input`), grid FAST, guided "
                                   "ZNSSD match, pose refinement (calcFastMotionOnly), process points (reprojection gate), dense point cloud -- and DWO "
                                   "inner-window Schur solve 50 KF / 20k landmarks",
                       "api": "svs_frontend_process_frames (frames by device pointer, poses from the host, results stay on the device)",
                       "stages": list(stage_ms.keys()),
                       "frame": "640x480", "batch_streams_per_gpu": B, "candidate_points": n_points,
                       # the metric's second half and its comparison, where the driver keeps them (`config` survives its summary; `schur` below is the full record)
                       "schur_ms_per_optimize": round(ms_opt, 4),
                       # the literal metric and the reference's real operating point: stereo frames/s ON STEREO INPUT (block matching inside the
                       # step), the one-camera latency mode stereo_slam runs (device time per frame / host images in, records out), the full-resolution tracker of
                       # configs[4], and the whole Schur step against HBM on SURVEY 8(d)'s own definition of its bytes
                       "value_stereo_input": round(fps_stereo, 2),
                       "latency_mode_B1_ms": round(lat_ms, 4),
                       "latency_mode_B1_host_io_ms": host_io["ms_per_frame"],
                       "dense_full_frames_per_s": dense_full["frames_per_s"],
                       "schur_step_frac_of_hbm": round(schur_step_bytes / (ms_opt / max(n_tr / K, 1) * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                       "schur_step_alg_bytes": int(schur_step_bytes),
                       "schur_speedup_vs_cpu_port": round(cpu_schur_ms / ms_opt, 2) if cpu_schur_ms else None,
                       "schur_ms_per_optimize_one_shot_p2p": (ba_p2p or {}).get("ms_per_optimize"),
                       "schur_weak_scaling_ms_per_optimize_per_gpu": (schur_weak or {}).get("ms_per_optimize_per_gpu"),
                       "schur_weak_scaling_sharded_window_ms_per_optimize": ((schur_weak or {}).get("sharded_window") or {}).get("ms_per_optimize"),
                       "tracker_accept_test": "the reference's decisions (float chi2 sums reproduced where f64 cannot decide); the mode tests/test_gpu_sequence.py holds identical over 200 frames",
                       "parallelism": f"front-end replicas x{world}; Schur landmarks sharded x{world} + all-reduce of reduced system",
                       "collective": (dict(comm.stats(), transport="RCCL ncclAllReduce(ncclDouble) issued by the library on its stream") if comm is not None
                                      else ({"transport": "torch.distributed all_reduce callback (library communicator unavailable)"} if allreduce is not None else None))},
            "schur": {"ms_per_optimize": round(ms_opt, 4), "lm_trials_per_optimize": n_tr / K,
                      "ms_per_call_incl_host_marshalling_and_copies": round(e2e_ms, 4) if e2e_ms else None,
                      "ms_per_schur_step": round(ms_opt / max(n_tr / K, 1), 4), "scaling": "strong",
                      "keyframes": P_, "landmarks": L_, "edges": E_total, "edges_this_rank": E_local,
                      "ms_per_optimize_with_event_brackets": round(ms_opt_ev, 4),
                      "one_shot_p2p_transport": ba_p2p,
                      "kernel_ms": {"landmark_reduce": round(red_ms, 5), "solve_cholesky": round(t_sol / max(n_tr, 1), 5),
                                    "backsub_chi2": round(t_bs / max(n_tr, 1), 5)},
                      "chi2_init": stats.chi2_init, "chi2_final": stats.chi2_final,
                      "speedup_vs_cpu_port": round(cpu_schur_ms / ms_opt, 2) if cpu_schur_ms else None,
                      "speedup_vs_cpu_port_drop_in_call": round(cpu_schur_ms / e2e_ms, 2) if (cpu_schur_ms and e2e_ms) else None,
                      "persistent_window": ({"ms_per_call_incl_update_optimize_readback": round(persistent_ms, 4),
                                             "speedup_vs_cpu_port": round(cpu_schur_ms / persistent_ms, 2) if cpu_schur_ms else None, **persistent_info}
                                            if persistent_ms else None),
                      "solve_kernel": opt.info()["solve_kernel"],
                      "other_windows": schur_rows,
                      "weak_scaling": schur_weak},
            "frontend": {"stage_ms_per_batch": {k: round(v, 4) for k, v in stage_ms.items()},
                         "stage_ms_sum": round(sum(stage_ms.values()), 4),
                         "ms_per_step_one_stream": round(ms_one_stream, 4),
                         "stage_ms_note": "measured inside the library with 9 events per step in a second pass over the same steps, every stage alone on the chain's stream: "
                                          "they add up to ms_per_step_one_stream; ms_per_step (= value) is measured without the events and with the library's default "
                                          "schedule, where FAST (and block matching) run on a side stream beside the dense tracker and fill its tail",
                         "dense_passes_per_frame": round(passes, 2),
                         "dense_sweeps_per_level": [round(float(x), 2) for x in sweeps_lvl],
                         "ms_per_step_tracker_grid_in_stream_order": round(t_front_stream_order / K * 1e3, 4),
                         "accept_test": {"mode": "reference's decisions (f64 sums outside the float sums' rigorous error band, the sequential float sums inside it, formed in parallel bit for bit)",
                                         "exact_float_sums_per_frame": round(exact_sums_per_frame, 2), "fallbacks_to_the_sequential_chain": exact_fallbacks,
                                         "ms_per_step_with_f64_sums_alone": round(t_front_f64_accept / K * 1e3, 4),
                                         "cost_of_parity_frac": round(t_front / t_front_f64_accept - 1.0, 4)},
                         "dense_serial_work_per_stream_in_level0_sweeps": {"min": min(cost_units), "mean": round(float(np.mean(cost_units)), 2), "max": max(cost_units), "correlation_with_the_next_frame": round(work_corr, 3) if work_corr is not None else None, "next_frame": cost_prev, "this_frame": cost_units,
                                                                           "note": "the tracker launch lasts as long as its longest stream"},
                         "dense_passes_per_frame_spread": {"min": int(passes_all.min()), "max": int(passes_all.max()), "distinct_frame_pairs": NPAIR},
                         "corners_per_frame": n_corners, "matches_per_frame": n_matched, "accepted_points_per_frame": n_accepted,
                         "tracking_ok_fraction": tracking_ok_frac,
                         "refined_pose_err_vs_true_motion": track_err,
                         "latency_mode_B1": {"ms_per_frame": round(lat_ms, 4), "frames_per_s": round(1e3 / lat_ms, 1), "stage_ms": lat_stages},
                         "latency_mode_B1_host_io": host_io,
                         "frames_per_s_per_gpu_by_batch": batch_sweep,
                         "stereo_input_path": dict(stereo_info, ms_per_step=round(t_stereo / max(4, K // 2 * 2) * 1e3, 4), frames_per_s=round(fps_stereo, 1),
                                                   stage_ms_per_batch={k: round(v, 4) for k, v in stage_ms_stereo.items()}),
                         "new_college_512x384": nc_row,
                         "two_threads_one_gpu": two_threads,
                         "cuda_build_path": cuda_path,
                         "overlapped_batches": overlapped,
                         "speedup_vs_cpu_port": round(fps / cpu["value"], 2) if cpu else None},
            "dense_full": dense_full,
            "roofline": roofline,
            "roofline_frontend": roofline_frontend,
            "cpu_baseline": cpu,
        }
        print(json.dumps(out))
    if use_dist:
        dist.barrier()          # ranks > 0 wait here while rank 0 times the CPU baseline
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
