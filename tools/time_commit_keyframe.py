"""Applying one SVS_KF_DROP decision to the resident map, two ways, in one process on the same inputs:

  one call       svs_frontend_decide_keyframes(want_lists = 0), then svs_frontend_commit_keyframe: the lists stay on the device
  composition    what a caller had before that call: svs_frontend_decide_keyframes(want_lists = 1) with its list download, the pose from svs_frontend_results,
                 the detector's thresholds read back level by level, then svs_map_add_keyframe with the lists from the host

at the reference's scale (12 keyframes, about 300 new and 400 track entries) and at a tenth of it.  A one-stream front end at 640 x 480 holds 12 keyframes (four
poses of the synthetic scene, three slots each) and tracks one frame against candidate lists drawn from all of them; the decision parameters make that step a drop.
The gate accepts a part of the candidates only, so a probing step measures that part and the lists are sized to end near the entry counts aimed at.
A commit changes the map, so every repetition gets a fresh pair of twin maps, built outside the clock; the front end is only read and is decided on again each
time.  A time is the host's wall clock around calls that end in a device synchronise, through the Python binding on both sides.  The first WARMUP repetitions are
left out; median and the 10th .. 90th percentile of the rest.  The two maps of the last repetition are compared.
usage: python tools/time_commit_keyframe.py [out.md]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

REPS, WARMUP = 60, 10
N_KF, COVIS = 12, 15
LONE = 999                # a keyframe without a point: no key of any table
SCALES = (("aimed at the reference's scale, 300 new and 400 track entries", 300, 400), ("aimed at a tenth of it, 30 and 40", 30, 40))      # accepted entries aimed at: new, track
MAX_POINTS = 1 << 15      # of the front end and of the maps: room for the candidates it takes to have that many accepted
PER_KF_CAP = MAX_POINTS // (2 * N_KF) - 8      # candidate records per keyframe and list
PROBE = (200, 280)        # candidate records per keyframe of the probing step that measures how many the gate accepts


def build(ctx, stream, per_new, per_track):
    """the front end after the step, and what a map needs: (fe, device disparity, lists, a function that makes a fresh map)"""
    import torch
    from scavislam_amd import capi, synth
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, KeyframeDecideParams
    from scavislam_amd.frontend import StereoFrontend
    from scavislam_amd.register import ResidentMap, keyframe_table
    cam = synth.CAM_DEFAULT
    sc = synth.Scene(2011)
    traj = synth.trajectory(6)
    frames = [sc.render(cam, traj[i], seed=i) for i in range(6)]
    rng = np.random.default_rng(5)
    fe = StereoFrontend(ctx, cam, max_points=MAX_POINTS, max_keyframes=N_KF + 1, params=capi.FrontendParams.reference())
    ids = [100 + 3 * j for j in range(N_KF)]
    new_parts, track_parts = [], []
    for j in range(N_KF):
        img, disp = frames[j % 4]
        fe.processFirstFrame(img, disp=disp)
        fe.keepKeyframe(j, traj[j % 4])
        n = per_new + per_track
        pts = synth.candidate_points(rng, cam, np.maximum(disp, 0), traj[j % 4], (n - n // 3 - n // 6, n // 3, n // 6), kf_index=j)
        rng.shuffle(pts)
        new_parts.append(pts[:per_new]); track_parts.append(pts[per_new:])
    act = N_KF - 1
    rec = np.concatenate([new_parts[act]] + [p for j, p in enumerate(new_parts) if j != act] + track_parts).astype(CANDIDATE_DTYPE)
    rec["point_id"] = np.arange(len(rec))
    n_new = per_new * N_KF
    T_act = traj[act % 4]
    fe.processFirstFrame(frames[4][0], disp=frames[4][1])
    fe.recomputeCloud(synth.pose_mul(traj[4], synth.pose_inv(T_act)).reshape(12))
    fe.setCandidateLists(rec, [per_new, n_new, len(rec)])
    with torch.cuda.stream(stream):
        d_disp = torch.as_tensor(np.ascontiguousarray(frames[5][1], np.float32)).cuda()
        blank = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ctx.sync()
    # the map in front of the drop: the track records are its points, each seen by its anchor and the two keyframes behind it
    track = rec[n_new:]
    vis = {int(r["point_id"]): sorted({ids[int(r["kf_index"])], ids[(int(r["kf_index"]) + 1) % N_KF], ids[(int(r["kf_index"]) + 2) % N_KF]}) for r in track}
    fe.setVertexTable([dict(stream=0, vertex_kf=ids, vertex_T=[traj[j % 4].reshape(12) for j in range(N_KF)],
                            sets=[sorted(p for p in vis if k in vis[p]) for k in ids], act=act, neighbors=[act - 1, act - 2], slot_kf=ids + [-1])])
    fe.processFrame(frames[5][0], synth.pose_mul(traj[5], synth.pose_inv(T_act)), T_act, disp=frames[5][1])
    prm = KeyframeDecideParams.reference()
    prm.parallax_thr, prm.switch_min_shared, prm.covis_thr = 1e-3, 1 << 30, COVIS      # a drop, never a switch
    kfs = keyframe_table([([blank.data_ptr()] * 3, [16] * 3, traj[j % 4].reshape(12)) for j in range(N_KF)])
    pts = np.array(track, CANDIDATE_DTYPE)
    pts["kf_index"] = [ids[int(k)] for k in track["kf_index"]]
    pp = [p for p in sorted(vis) for _ in vis[p]]
    kk = [k for p in sorted(vis) for k in vis[p]]

    def fresh():
        m = ResidentMap(ctx, max_keyframes=1024, max_points=MAX_POINTS, max_observations=1 << 17)
        m.reserve_edges(256)
        m.add_keyframes(ids + [LONE], np.concatenate([kfs, kfs[:1]]), [(blank.data_ptr(), 4)] * (N_KF + 1), [[[25], [25], [25]]] * (N_KF + 1))
        m.add_points(pts["point_id"], pts)
        m.add_measured_observations(pp, kk, np.ones((len(pp), 3)), np.zeros(len(pp), np.int32))
        m.get_poses(ids[:1])                       # (the map's download block comes with its first read-back: not the insertion's business)
        return m
    return fe, (d_disp.data_ptr(), cam["w"]), prm, ids, fresh, (d_disp, blank), cam


def accepted(ctx, stream, per_new, per_track):
    """(new, track) entries of the decision's lists for these candidate counts per keyframe"""
    fe = build(ctx, stream, per_new, per_track)[0:3]
    d = fe[0].decideKeyframes(params=fe[2], want_lists=0)[0]["dec"]
    fe[0].close()
    return int(d["n_new"]), int(d["n_track"])


def measure(ctx, stream, want_new, want_track):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import KF_DROP
    from scavislam_amd.frontend import fastgrid_for_level
    from scavislam_amd.register import keyframe_table
    # candidate counts per keyframe that make the gate accept about what is aimed at, from one probing step
    got_new, got_track = accepted(ctx, stream, *PROBE)
    per_new = int(min(max(round(want_new / N_KF * PROBE[0] / max(got_new / N_KF, 1e-9)), 1), PER_KF_CAP))
    per_track = int(min(max(round(want_track / N_KF * PROBE[1] / max(got_track / N_KF, 1e-9)), 1), PER_KF_CAP))
    print(f"probe: {PROBE} candidates per keyframe gave {got_new} new and {got_track} track entries; taking {per_new} and {per_track} per keyframe", flush=True)
    fe, disp, prm, ids, fresh, keep, cam = build(ctx, stream, per_new, per_track)
    act, newkey, slot = ids[-1], 500, N_KF
    first = fe.decideKeyframes(params=prm, want_lists=1)[0]
    assert first["dec"]["valid"] == 1 and first["dec"]["decision"] == KF_DROP, "the step is no drop"
    print(f"lists: {len(first['new'])} new, {len(first['track'])} track; new entries anchored in the active keyframe: {int((first['new']['anchor_id'] == ids[-1]).sum())}", flush=True)
    fe.keepKeyframe(slot, first["dec"]["T_newkey_from_w"])
    anchors = first["new"]["anchor_id"]
    if len(anchors) and not (anchors == act).any():      # (a short list may hold no entry of the active keyframe: any anchor is a key of the table)
        act = int(np.bincount(anchors[anchors >= 0]).argmax())
        print(f"no new entry is anchored in the active keyframe: oldkey = {act}", flush=True)
    ncell = [fastgrid_for_level(cam["w"] >> l, cam["h"] >> l, l) for l in range(3)]
    ncell = [g.gx * g.gy for g in ncell]
    blank_kf = keyframe_table([([keep[1].data_ptr()] * 3, [16] * 3, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])])[0]
    fast = fe.fast_handle()

    def thresholds(level):
        """the detector's persistent thresholds of one level, and nothing else of svs_fast_download"""
        n, ts = C.c_int32(), np.zeros(64, np.int32)
        ctx.check(ctx.lib.svs_fast_download(fast, 0, level, None, 0, C.byref(n), None, None, ts.ctypes.data))
        return ts[:ncell[level]].tolist()
    t = dict(one=[], one_commit=[], comp=[], comp_lists=[], comp_insert=[], first=[], second=[])
    last = None
    for r in range(REPS):
        a, b = fresh(), fresh()
        # a map's first device-list call allocates its id sets and scratch row and uploads the sets: once in a map's life, so outside the clock -- a call that is
        # refused behind its first download (LONE is no key) does all of it and leaves the map as it was; timed for the record, beside a second one
        fe.decideKeyframes(params=prm, want_lists=0)
        for key in ("first", "second"):
            ctx.sync()
            t0 = time.perf_counter()
            try:
                fe.commitKeyframe(a, 0, slot, newkey, LONE, disp, COVIS, cam["w"] // 2, cam["h"] // 2)
                raise AssertionError("LONE is a key")
            except capi.SvsError:
                pass
            if r >= WARMUP:
                t[key].append((time.perf_counter() - t0) * 1e3)
        ctx.sync()
        t0 = time.perf_counter()
        fe.decideKeyframes(params=prm, want_lists=0)
        t1 = time.perf_counter()
        got = fe.commitKeyframe(a, 0, slot, newkey, act, disp, COVIS, cam["w"] // 2, cam["h"] // 2)
        t2 = time.perf_counter()
        out = fe.decideKeyframes(params=prm, want_lists=1)[0]
        res = fe.results(0)[0]
        thr = [thresholds(l) for l in range(3)]
        t3 = time.perf_counter()
        want = b.add_keyframe(newkey, act, np.array(res.T_cur_from_actkey), blank_kf, disp, thr, out["new"], out["track"], COVIS, cam["w"] // 2, cam["h"] // 2)
        t4 = time.perf_counter()
        assert got["edges"] == want["edges"] and got["new_kept"].tolist() == want["new_kept"].tolist()
        if r >= WARMUP:
            t["one"].append((t2 - t0) * 1e3); t["one_commit"].append((t2 - t1) * 1e3)
            t["comp"].append((t4 - t2) * 1e3); t["comp_lists"].append((t3 - t2) * 1e3); t["comp_insert"].append((t4 - t3) * 1e3)
        if last:
            for m in last:
                m.close()
        last = (a, b)
    a, b = last
    kfs = ids + [newkey]
    assert a.info() == b.info() and a.edge_info() == b.edge_info() and a.get_poses(kfs).tobytes() == b.get_poses(kfs).tobytes()
    assert all(a.get_feature_table(k)[1].tobytes() == b.get_feature_table(k)[1].tobytes() for k in kfs)
    shape = dict(n_new=int(out["dec"]["n_new"]), n_track=int(out["dec"]["n_track"]), keys=int(got["n_keys"]), edges=len(got["edges"]), kept=int(got["new_kept"].sum()),
                 list_bytes=96 * int(out["dec"]["n_new"]) + 32 * int(out["dec"]["n_track"]))
    for m in last:
        m.close()
    fe.close()
    return t, shape


def main():
    from scavislam_amd import capi
    args = sys.argv[1:]
    ctx, stream = capi.torch_context(0)
    q = lambda v: f"{np.median(v):.3f} ({np.percentile(v, 10):.3f} .. {np.percentile(v, 90):.3f})"
    lines = ["# `svs_frontend_commit_keyframe`: applying one drop, beside the composition it replaces", "",
             __doc__.split("usage:")[0].strip(), ""]
    for name, want_new, want_track in SCALES:
        t, s = measure(ctx, stream, want_new, want_track)
        spread = np.percentile(t["comp"], 90) - np.percentile(t["comp"], 10)
        diff = np.median(t["one"]) - np.median(t["comp"])
        lines += [f"## {name}; reached: {s['n_new']} new and {s['n_track']} track entries ({s['list_bytes']} bytes of list records), {s['keys']} keys, {s['edges']} new edges, "
                  f"{s['kept']} new points kept", "",
                  "| what | wall per drop, ms: median (10th .. 90th percentile) |", "|---|---:|",
                  f"| one call: decide (no lists) + svs_frontend_commit_keyframe | {q(t['one'])} |",
                  f"| - svs_frontend_commit_keyframe alone | {q(t['one_commit'])} |",
                  f"| composition: decide (lists) + results + thresholds + svs_map_add_keyframe | {q(t['comp'])} |",
                  f"| - decide with the list download, the pose, the three threshold read-backs | {q(t['comp_lists'])} |",
                  f"| - svs_map_add_keyframe alone, the lists on the host | {q(t['comp_insert'])} |",
                  f"| outside the clock: a map's FIRST device-list call (refused behind its download): id sets and scratch row allocated, sets uploaded | {q(t['first'])} |",
                  f"| the same refused call a second time | {q(t['second'])} |", "",
                  f"one call minus composition, medians: {diff:+.3f} ms; the composition's own 10th .. 90th percentile spread: {spread:.3f} ms; "
                  f"{REPS - WARMUP} timed repetitions behind {WARMUP} of warm-up", ""]
    text = "\n".join(lines)
    print(text)
    if args and not args[0].startswith("--"):
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        open(args[0], "w").write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
