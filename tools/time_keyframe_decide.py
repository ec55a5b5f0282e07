"""Times svs_frontend_decide_keyframes (keyframe.hip) for B = 1, 64, 512 streams from the recorded step 40 of the 512 x 384 sequence and writes
profiles/keyframe_decide.md.

The state.  The first 41 frames run through the reference's loop with the one-call binding (oracle/_ref/libsvs_hipbranch_seq_onecall.so), as
tests/test_gpu_keyframe_sequence.py runs all 200; a one-stream replay with the decision stage behind every step rebuilds the vertex table of step 40 (poses, feature
sets, strength_to_neighbors of the keyframes dropped so far).  A B-stream front end then replays the same 40 recorded calls for all its streams at once
(keepKeyframes, setCandidateListsAll, processFrames), so every stream holds step 40's records, and gets the same vertex table.

Two paths, timed in the same run, alternating, WARMUP calls first, median (min .. max) of CALLS:
  device   svs_frontend_decide_keyframes(want_lists = 1): one launch, one download of B decision records, the list rows of the dropped streams.  The context's events
           around the call, and the host clock around the same call (it blocks).
  host     what a caller does without the stage, with calls the parent commit already has: svs_frontend_results for every stream (small block + n match records + n
           gate records each), then tests/keyframe_model.py's decide() on the host.  Host clock (every download blocks).  The model is NumPy / Python, so its time is
           an upper bound of a host walk, not a C++ figure; the download time is given on its own.
Bytes moved are counted from the shapes.  Needs a GPU and the oracle library; fails without them."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, WARMUP, STEP = 20, 3, 40
MAX_KEYFRAMES = 8


def spread(v):
    return statistics.median(v), min(v), max(v)


def main():
    import torch
    import keyframe_model as KM
    import oracle as O
    import seq_common as S
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import GATED_POINT_DTYPE, KEYFRAME_DECISION_DTYPE, MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE, MATCH_RESULT_DTYPE, level_cams
    from scavislam_amd.frontend import StereoFrontend
    assert torch.cuda.is_available(), "needs a GPU"
    ctx, stream = capi.torch_context(0)
    cam = S.cam_of("newcollege")
    w, h = cam["w"], cam["h"]
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], w, h)
    frames = list(S.frames("newcollege", STEP + 1))
    seq = O.RefSequence(cams, hip_branch=True, one_call=True)
    loop, recs = [], []
    for img, disp in frames:
        loop.append(seq.step(img, disp))
        recs.append(seq.onecall_record())
    seq.close()
    max_points = max(len(r["pts"]) for r in recs[1:]) + 64

    # one stream, the stage behind every step: the vertex table of step STEP
    fe = StereoFrontend(ctx, cam, max_points=max_points, max_keyframes=MAX_KEYFRAMES)
    fe.processFirstFrame(frames[0][0], disp=frames[0][1])
    vertices, pending, act_id = [], dict(id=loop[0]["actkey_id"], ids=set(), strength=[]), loop[0]["actkey_id"]
    slot_kf = np.full(MAX_KEYFRAMES, -1, np.int32)
    table = None
    for k in range(1, STEP + 1):
        rc, r = recs[k], loop[k]
        if rc["kept_slot"] >= 0:
            fe.keepKeyframe(rc["kept_slot"], rc["kept_pose"])
            slot_kf[rc["kept_slot"]] = pending["id"]
            vertices.append(dict(pending, T=rc["kept_pose"].copy()))
            pending = None
        fe.setCandidateLists(rc["pts"], rc["group_end"])
        fe.processFrame(frames[k][0], rc["T_guess"], rc["T_act"], disp=frames[k][1])
        index = {v["id"]: i for i, v in enumerate(vertices)}
        table = dict(vertex_kf=[v["id"] for v in vertices], vertex_T=np.stack([v["T"] for v in vertices]), sets=[sorted(v["ids"]) for v in vertices], act=index[act_id],
                     neighbors=[index[i] for i in vertices[index[act_id]]["strength"]], slot_kf=slot_kf.copy())
        fe.setVertexTable([dict(table, stream=0)])
        out = fe.decideKeyframes(want_lists=2)[0]
        d = out["dec"]
        assert (d["decision"] == KM.KF_DROP, d["decision"] == KM.KF_SWITCH) == (r["dropped"], r["switched"]), k
        if r["dropped"]:
            pending = dict(id=r["actkey_id"], ids=set(int(i) for i in out["new"]["point_id"]) | set(int(i) for i in out["track"]["global_id"]),
                           strength=[int(i) for i in d["strength_kf"][:d["n_strength"]]])
        if r["dropped"] or r["switched"]:
            act_id = r["actkey_id"]
        if rc["recloud"] and k < STEP:
            fe.recomputeCloud(rc["recloud_pose"])
    fe.close()
    model_table = dict(kf=table["vertex_kf"], T=table["vertex_T"], sets=table["sets"], act=table["act"], neighbors=table["neighbors"], slot_kf=table["slot_kf"])

    rows = []
    for B in (1, 64, 512):
        fe = StereoFrontend(ctx, cam, max_points=max_points, max_keyframes=MAX_KEYFRAMES, n_streams=B)
        def dev(k):      # every stream sees frame k
            with torch.cuda.stream(stream):
                return dict(left=torch.as_tensor(frames[k][0]).cuda().expand(B, h, w).contiguous(),
                            disp=torch.as_tensor(frames[k][1].astype(np.float32)).cuda().expand(B, h, w).contiguous())

        fe.processFirstFrames(**dev(0))
        for k in range(1, STEP + 1):
            rc = recs[k]
            if rc["kept_slot"] >= 0:
                fe.keepKeyframes(rc["kept_slot"], np.stack([rc["kept_pose"]] * B))
            fe.setCandidateListsAll([rc["pts"]] * B, [rc["group_end"]] * B)
            fr = dev(k)
            fe.processFrames(np.stack([rc["T_guess"]] * B), np.stack([rc["T_act"]] * B), **fr)
            ctx.sync()      # (the frames are read in place until the chain has run)
            if rc["recloud"] and k < STEP:
                fe.recomputeCloud(rc["recloud_pose"])
        fe.setVertexTable([dict(table, stream=b) for b in range(B)])
        n = len(recs[STEP]["pts"])
        ev, wall, host_dl, host_all = [], [], [], []
        for it in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            ctx.timer_start()
            out = fe.decideKeyframes(want_lists=1)
            ms = ctx.timer_stop_ms()
            t1 = time.perf_counter()
            got = [fe.results(b) for b in range(B)]
            t2 = time.perf_counter()
            decs = [KM.decide(m, recs[STEP]["pts"], g, dict(num_points_grid2x2=list(res.point_stats.num_points_grid2x2), num_points_grid3x3=list(res.point_stats.num_points_grid3x3),
                                                            sum_track_length=res.point_stats.sum_track_length, num_track_points=res.point_stats.num_track_points),
                              np.array(res.T_cur_from_actkey), res.tracking_ok, model_table)["dec"] for res, m, g in got]
            t3 = time.perf_counter()
            if it >= WARMUP:
                ev.append(ms); wall.append(1e3 * (t1 - t0)); host_dl.append(1e3 * (t2 - t1)); host_all.append(1e3 * (t3 - t1))
        assert all(o["dec"].tobytes() == dm.tobytes() for o, dm in zip(out, decs)), "the device's decision differs from the host model's"
        n_drop = sum(int(o["dec"]["decision"] == KM.KF_DROP) for o in out)
        dev_bytes = B * KEYFRAME_DECISION_DTYPE.itemsize + sum((MAP_NEW_POINT_DTYPE.itemsize + 4) * int(o["dec"]["n_new"]) + (MAP_TRACK_POINT_DTYPE.itemsize + 4) * int(o["dec"]["n_track"])
                                                               for o in out if o["dec"]["decision"] == KM.KF_DROP)
        small = ((8 * 48 + 32 + 88 + 8) * B + 255) // 256 * 256      # the front end's per-stream scalar block, downloaded whole by every svs_frontend_results
        host_bytes = B * (small + n * (MATCH_RESULT_DTYPE.itemsize + GATED_POINT_DTYPE.itemsize))
        rows.append(dict(B=B, n=n, ev=spread(ev), wall=spread(wall), host_dl=spread(host_dl), host_all=spread(host_all), dev_bytes=dev_bytes, host_bytes=host_bytes, n_drop=n_drop,
                         decision=int(out[0]["dec"]["decision"]), n_new=int(out[0]["dec"]["n_new"]), n_track=int(out[0]["dec"]["n_track"]), V=len(table["vertex_kf"])))
        print(rows[-1], flush=True)
        fe.close()
    with open(os.path.join(ROOT, "profiles", "keyframe_decide.md"), "w") as f:
        f.write("# Keyframe decision behind a step (`keyframe.hip`): measurements\n\n")
        f.write(f"Written by `tools/time_keyframe_decide.py` on one MI355X: the 512 x 384 sequence, every stream holds the recorded step {STEP} (records per stream, vertices, decision\n"
                f"and list lengths below).  ms per call, median (min .. max) over {CALLS} calls after {WARMUP}, both paths alternating in one run.  Device: `svs_frontend_decide_keyframes` with\n"
                "`want_lists = 1` -- one launch, one download of the decision records, the list rows of dropped streams -- by the context's events and by the host clock around the\n"
                "blocking call (both around the Python mirror's call, its per-stream bookkeeping included).  Host: `svs_frontend_results` for every stream (calls the parent commit has), then `tests/keyframe_model.py` on the host; the download is given on\n"
                "its own, because the model is NumPy / Python and bounds a host walk from above.  Bytes are counted from the shapes.\n\n")
        f.write("| B | records / vertices | decision (n_new / n_track) | device: events ms | device: host clock ms | device: bytes to the host | host: downloads ms | host: downloads + model ms | host: bytes to the host | bytes ratio |\n")
        f.write("|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r['B']} | {r['n']} / {r['V']} | {('KEEP', 'SWITCH', 'DROP')[r['decision']]} ({r['n_new']} / {r['n_track']}) | {r['ev'][0]:.3f} ({r['ev'][1]:.3f} .. {r['ev'][2]:.3f}) | "
                    f"{r['wall'][0]:.3f} ({r['wall'][1]:.3f} .. {r['wall'][2]:.3f}) | {r['dev_bytes']} | {r['host_dl'][0]:.3f} ({r['host_dl'][1]:.3f} .. {r['host_dl'][2]:.3f}) | "
                    f"{r['host_all'][0]:.3f} ({r['host_all'][1]:.3f} .. {r['host_all'][2]:.3f}) | {r['host_bytes']} | {100.0 * r['dev_bytes'] / r['host_bytes']:.2f} % |\n")
        f.write("\nNo kernel-only time was taken (no profiler run): the device figures are whole calls, the download included.\n")
        f.write("\n## `T_cur_after` against the reference's loop\n\n`tests/test_gpu_keyframe_sequence.py` replays the 200-frame sequence (6 drops, 5 switches) and prints, per frame, the largest element-wise deviation of\n"
                "`T_cur_after` from the pose the reference's loop holds after its keyframe logic.  Measured on one MI355X: 0.0 on every frame, the five switches included -- the\n"
                "loop's `SE3` stand-in forms the products `T_cur_from_actkey * T_act_from_w * T_other_from_w.inverse()` by the same row sums as `pose.h`.  The test's bar is ten times\n"
                "the measured value: equality.\n")
    ctx.close()


if __name__ == "__main__":
    main()
