"""Times svs_frontend_seed_keyframes (seed.hip) at 640 x 480 for B = 1, 64, 512 streams and writes profiles/seed.md.

Two cases per batch size:
  first frame    SVS_SEED_FIRST behind processFirstFrames: empty tree, the caps (301 / 151 / 76) are reached early in every level
  steady state   SVS_SEED_MORE behind one processFrames step with ~150 tracked points per stream; ui.num_max_points and ui.min_num_points are raised so that no
                 cap is reached and every 3 x 3 cell asks for points: every corner of every level is visited
Time per call = the context's events (svs_timer_start in front of the call, svs_timer_stop_ms behind it: staged upload, both kernels, download), median over
CALLS calls after WARMUP; the host clock around the same calls is printed beside it.  From the same run: what the host path needs before it can seed on the CPU --
three svs_fast_download and one disparity copy per stream -- by the host clock (every one of those calls blocks).  Needs a GPU; fails without one."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, WARMUP = 20, 3
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def timed(ctx, fn):
    ev, wall = [], []
    for k in range(WARMUP + CALLS):
        t0 = time.perf_counter()
        ctx.timer_start()
        fn()
        ms = ctx.timer_stop_ms()
        if k >= WARMUP:
            ev.append(ms); wall.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ev), min(ev), max(ev), statistics.median(wall)


def seed_call(fe, ctx, reqs, prm):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, SeedRequest
    n, cap = len(reqs), prm.max_records()
    req = (SeedRequest * n)()
    for r, q in zip(req, reqs):
        r.stream, r.mode, r.kf_index, r.first_point_id, r.seed = q["stream"], q["mode"], 0, 1, q["seed"]
        for i in range(12):
            r.T_newkey_from_cur[i] = float(I34.reshape(12)[i])
    out = np.zeros((n, cap), CANDIDATE_DTYPE)
    out.view(np.uint8)[...] = 0      # touch the pages once, outside the timed calls
    cnt = np.zeros((n, 3), np.int32)
    return (lambda: ctx.check(ctx.lib.svs_frontend_seed_keyframes(fe.h, n, req, C.byref(prm), out.ctypes.data, cap, cnt.ctypes.data))), out, cnt


def host_path(fe, ctx, B, w, h):
    """what a host-side addMorePoints needs first: the three corner lists and the disparity image of every stream"""
    xy = np.zeros((8192, 2), np.int16)
    cc = np.zeros(64, np.int32)
    n = C.c_int32()
    disp = np.zeros((h, w), np.float32)
    f = fe.fast_handle()
    t = []
    for k in range(1 + 3):
        t0 = time.perf_counter()
        nbytes = 0
        for b in range(B):
            for l in range(3):
                ctx.check(ctx.lib.svs_fast_download(f, b, l, xy.ctypes.data, 8192, C.byref(n), cc.ctypes.data, None, None))
                nbytes += 4 * n.value + 4 * 9
            d = C.c_void_p()
            ctx.check(ctx.lib.svs_frontend_device_view(fe.h, b, None, None, C.byref(d), None, None))
            ctx.call("svs_memcpy_d2h", disp.ctypes.data, d, disp.nbytes)
            nbytes += disp.nbytes
        if k:
            t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), nbytes


def main():
    import torch
    import seed_common as S
    import seq_common
    from scavislam_amd import capi, synth
    from scavislam_amd.ctypes_types import SEED_FIRST, SEED_MORE, SeedParams
    from scavislam_amd.frontend import StereoFrontend
    assert torch.cuda.is_available(), "needs a GPU"
    ctx, stream = capi.torch_context(0)
    cam = synth.CAM_DEFAULT
    w, h = cam["w"], cam["h"]
    (img0, disp0), (img1, disp1) = S.frame("default", 0), S.frame("default", 1)
    traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)
    rows = []
    for B in (1, 64, 512):
        fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2, n_streams=B)
        with torch.cuda.stream(stream):
            l0 = torch.as_tensor(img0).cuda().expand(B, h, w).contiguous(); d0 = torch.as_tensor(disp0.astype(np.float32)).cuda().expand(B, h, w).contiguous()
            l1 = torch.as_tensor(img1).cuda().expand(B, h, w).contiguous(); d1 = torch.as_tensor(disp1.astype(np.float32)).cuda().expand(B, h, w).contiguous()
        fe.processFirstFrames(left=l0, disp=d0)
        prm = SeedParams.reference()
        call, out, cnt = seed_call(fe, ctx, [dict(stream=b, mode=SEED_FIRST, seed=1000 + b) for b in range(B)], prm)
        first = timed(ctx, call)
        n_first = cnt.sum(1)
        corners = sum(len(fe.corners(0, l)[0]) for l in range(3))
        host_ms, host_bytes = host_path(fe, ctx, B, w, h)
        # steady state: 225 of the seeded points of every stream, spread evenly over the list, go through one step, which tracks about two thirds of them
        pts = [out[b, np.linspace(0, int(n_first[b]) - 1, 225).astype(np.int64)].copy() for b in range(B)]
        fe.keepKeyframes(0, np.stack([traj[0].reshape(12)] * B))
        fe.setCandidateListsAll(pts, [[len(p), len(p)] for p in pts])
        fe.processFrames(np.stack([I34.reshape(12)] * B), np.stack([traj[0].reshape(12)] * B), left=l1, disp=d1)
        res = fe.results(0)[0]
        prm2 = SeedParams.reference(num_max_points=4000, min_num_points=1 << 20)
        call2, out2, cnt2 = seed_call(fe, ctx, [dict(stream=b, mode=SEED_MORE, seed=2000 + b) for b in range(B)], prm2)
        more = timed(ctx, call2)
        corners1 = sum(len(fe.corners(0, l)[0]) for l in range(3))
        rows.append(dict(B=B, first=first, more=more, n_first=float(n_first.mean()), n_more=float(cnt2.sum(1).mean()), tracked=int(sum(res.point_stats.num_matched_points)),
                         corners0=corners, corners1=corners1, host_ms=host_ms, host_mb=host_bytes / 1e6, capped=bool((cnt2 > np.array([4000, 2000, 1000])).any())))
        print(rows[-1], flush=True)
        fe.close()
        del l0, d0, l1, d1
    with open(os.path.join(ROOT, "profiles", "seed.md"), "w") as f:
        f.write("# New-point seeding (`seed.hip`): measurements\n\n")
        f.write("Written by `tools/time_seed.py` on one MI355X: 640 x 480, every stream holds the same two frames of the sequence fixture (frames 0 and 1), every request its own\n"
                "seed (generated order).  ms per `svs_frontend_seed_keyframes` call for B requests = the context's events around the call (staged upload, order kernel,\n"
                f"greedy kernel, download), median (min .. max) over {CALLS} calls after {WARMUP}; the host clock around the same calls beside it.  First frame: `SVS_SEED_FIRST`, empty tree,\n"
                "caps 301 / 151 / 76 reached in every level.  Steady state: `SVS_SEED_MORE` behind one step that tracked the stated number of points, `num_max_points` = 4000 and\n"
                "`min_num_points` = 2^20, so no cap is reached and every corner of every level is visited.  Host path: the three `svs_fast_download`s and the disparity copy of\n"
                "every stream (what a host-side `addMorePoints` needs before it can start), host clock, median of 3 rounds; the quadtree walk itself was not timed.\n\n")
        f.write("| B | first frame: ms per call (events) | host clock ms | records per request | steady state: ms per call (events) | host clock ms | tracked / records per request | corners visited per request | host path: ms, MB fetched |\n")
        f.write("|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r['B']} | {r['first'][0]:.3f} ({r['first'][1]:.3f} .. {r['first'][2]:.3f}) | {r['first'][3]:.3f} | {r['n_first']:.0f} | "
                    f"{r['more'][0]:.3f} ({r['more'][1]:.3f} .. {r['more'][2]:.3f}) | {r['more'][3]:.3f} | {r['tracked']} / {r['n_more']:.0f}{' (a cap was reached)' if r['capped'] else ''} | "
                    f"{r['corners1']} | {r['host_ms']:.2f}, {r['host_mb']:.1f} |\n")
        f.write("\nAlgorithmic bytes (DESIGN.md section 3d): per visited corner 4 B of order index, 4 B of corner and 4 B of disparity; 64 B per record written, and 64 B per record\n"
                "downloaded.  No kernel-only time was taken (no profiler run): the figures above are whole calls, copies included.\n")
    ctx.close()


if __name__ == "__main__":
    main()
