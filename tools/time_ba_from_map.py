"""the double window's BA problem built from the device-resident map (svs_map_prepare_window + svs_ba_window_from_map + svs_ba_optimize + svs_ba_store_to_map)
beside the two upload forms, in one process, on two maps:
    scene       the test scene (tests/ba_map_model.scene): 14 keyframes, 1 700 points, 13-keyframe final window with 1 340 active points
    large       synth.ba_window(50, 20 000): a 50-keyframe final window (two of them enter as the extension), some 100 k observations, inside a map of 200
                keyframes whose other 150 hold 15 000 points of their own
Three forms, each through the C entry points with its arguments READY, so none pays for a binding:
    (i)    prepare_window + window_from_map + optimize + store_to_map
    (ii)   svs_ba_window_update in its steady state (the store holds everything but ONE keyframe's observations, which the call brings) + optimize + get_state +
           invert_depth on the host + svs_map_set_poses / svs_map_set_points
    (iii)  svs_ba_set_problem with every edge record + the same tail
Forms (ii) and (iii) are given the model-built arrays: the host's walk over its graph (computeActivePointsAndExtendOuterWindow, copyDataToG2o's loops over hash
tables), which form (i) replaces, is NOT in their time.  Before every timed call the map's poses and points are put back to the start state (outside the timing),
so that every round optimises the same problem; form (ii) is preceded by svs_ba_window_forget_keyframes of the one keyframe (outside the timing).
Per form: wall clock of the blocking calls, and the span between two events on the context's stream around them.  The forms alternate; medians over ROUNDS rounds
behind a warm-up; the whole alternation runs REPS times.  Before it times, the script checks that forms (i) and (ii) hand the optimizer the same bytes.
usage: python tools/time_ba_from_map.py [out.md]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import ba_map_model as BM

ROUNDS, WARMUP, REPS = 30, 5, 3


def large_scene(P=50, L=20000, n_other=150, per_other=100, seed=2012):
    from scavislam_amd import synth
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE
    rng = np.random.default_rng(seed)
    prob = synth.ba_window(P=P, L=L, seed=seed, n_outer=3)
    kf_ids = (n_other + np.arange(P)).astype(np.int32)
    point_ids = np.arange(L, dtype=np.int32)
    e = prob["edges"]
    anchor_idx = np.zeros(L, np.int64)
    anchor_idx[e["point"]] = e["anchor"]
    level = np.round(np.log(1.0 / e["info"][:, 0]) / np.log(4.0)).astype(np.int32)
    # the rest of the map: keyframes 0 .. n_other - 1, each with points of its own seen by itself and the next keyframe
    o_pts = L + np.arange(n_other * per_other, dtype=np.int32)
    o_anchor = (np.arange(len(o_pts)) // per_other).astype(np.int32)
    o_next = np.minimum(o_anchor + 1, n_other - 1)
    two = o_next != o_anchor
    I12 = np.eye(3, 4).reshape(12)
    m = dict(kf_ids=np.concatenate([np.arange(n_other, dtype=np.int32), kf_ids]), kf_poses=np.concatenate([np.tile(I12, (n_other, 1)), prob["poses"]]),
             point_ids=np.concatenate([point_ids, o_pts]), anchor_ids=np.concatenate([kf_ids[anchor_idx], o_anchor]),
             xyz=np.concatenate([BM.invert_depth(prob["psi"]), rng.normal(size=(len(o_pts), 3)) + [0, 0, 8]]),
             obs_point=np.concatenate([point_ids[e["point"]], o_pts, o_pts[two]]).astype(np.int32), obs_kf=np.concatenate([kf_ids[e["pose"]], o_anchor, o_next[two]]).astype(np.int32),
             obs_center=np.concatenate([e["obs"], rng.uniform(0, 400, (len(o_pts) + int(two.sum()), 3))]),
             obs_level=np.concatenate([level, np.zeros(len(o_pts) + int(two.sum()), np.int32)]).astype(np.int32))
    inner = P - 3
    w0_ids = kf_ids[2:].copy()
    w0_types = (np.arange(2, P) >= inner).astype(np.int32)
    pairs = [(kf_ids[i], kf_ids[i - d]) for i in range(3, inner) for d in (1, 2)] + [(kf_ids[2], kf_ids[0]), (kf_ids[3], kf_ids[1]), (kf_ids[2], kf_ids[1])]
    cons = np.zeros(len(prob["cons"]), BA_CONSTRAINT_DTYPE)
    cons[:] = prob["cons"]
    cons["pose1"], cons["pose2"] = kf_ids[prob["cons"]["pose1"]], kf_ids[prob["cons"]["pose2"]]
    return dict(map=m, w0_ids=w0_ids, w0_types=w0_types, pairs=np.array(pairs, np.int32), cons=cons, cam=prob["cam"])


def main():
    import torch
    from scavislam_amd import capi
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BA_EDGE_DTYPE, CANDIDATE_DTYPE, BaParams, BaStats, Cam, MapWindowResult
    from scavislam_amd.register import ResidentMap, keyframe_table

    ctx, stream = capi.torch_context(0)
    lib = ctx.lib
    with torch.cuda.stream(stream):
        any_u8 = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")      # the walks read no image
        any_f32 = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    med = lambda a: float(np.median(a))
    lines = ["| map | window | active points | edges | form | wall per call (ms) | per repetition | stream span (ms) |", "|---|---:|---:|---:|---|---:|---|---:|"]
    notes = []
    for name, sc in (("scene", BM.scene()), ("large", large_scene())):
        m = sc["map"]
        prep = BM.prepare(m, sc["w0_ids"], sc["w0_types"], sc["pairs"])
        prob = BM.problem(m, prep["window_ids"], prep["active_ids"])
        c = sc["cam"]
        cam, prm = Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"]), BaParams.reference_defaults()
        rmap = ResidentMap(ctx, max_keyframes=1024, max_points=1 << 16, max_observations=1 << 19)
        kfs = keyframe_table([([any_u8.data_ptr()] * 3, [64] * 3, T) for T in m["kf_poses"]])
        rmap.add_keyframes(m["kf_ids"], kfs, [(any_f32.data_ptr(), 64)] * len(kfs), [[[25], [25], [25]]] * len(kfs))
        pts = np.zeros(len(m["point_ids"]), CANDIDATE_DTYPE)
        pts["xyz_anchor"], pts["kf_index"] = m["xyz"], m["anchor_ids"]
        rmap.add_points(m["point_ids"], pts)
        rmap.add_measured_observations(m["obs_point"], m["obs_kf"], m["obs_center"], m["obs_level"])
        # ---- the arguments of the three forms, ready
        w0, t0, pairs, cons = (np.ascontiguousarray(sc[k]) for k in ("w0_ids", "w0_types", "pairs", "cons"))
        P, L = len(prob["pose_ids"]), len(prob["point_ids"])
        res, wid, wty = MapWindowResult(), np.zeros(256, np.int32), np.zeros(256, np.int32)
        st = BaStats()
        pose_ids, point_ids, anchor_ids = (np.ascontiguousarray(prob[k], np.int32) for k in ("pose_ids", "point_ids", "anchor_ids"))
        poses0, psi0 = np.ascontiguousarray(prob["poses"]), np.ascontiguousarray(prob["psi"])
        xyz0 = np.ascontiguousarray(BM.invert_depth(psi0))
        widx = {int(k): i for i, k in enumerate(pose_ids)}
        lidx = {int(p): i for i, p in enumerate(point_ids)}
        by_id = prob["edges"]
        by_idx = by_id.copy()
        by_idx["point"] = [lidx[int(p)] for p in by_id["point"]]; by_idx["pose"] = [widx[int(k)] for k in by_id["pose"]]; by_idx["anchor"] = [widx[int(k)] for k in by_id["anchor"]]
        cons_idx = cons.copy()
        cons_idx["pose1"] = [widx[int(k)] for k in cons["pose1"]]; cons_idx["pose2"] = [widx[int(k)] for k in cons["pose2"]]
        inner_seen = [int(k) for k, t in zip(sc["w0_ids"], sc["w0_types"]) if t == 0 and (by_id["pose"] == k).any()]
        newest = np.array([inner_seen[-1]], np.int32)                                      # the newest INNER keyframe that observes anything
        obs_new = np.ascontiguousarray(by_id[by_id["pose"] == newest[0]])
        obs_old = np.ascontiguousarray(by_id[by_id["pose"] != newest[0]])
        out_poses, out_psi = np.zeros((P, 12)), np.zeros((L, 3))
        a, b, d = SlamGraphOptimizer(ctx, stream), SlamGraphOptimizer(ctx, stream), SlamGraphOptimizer(ctx, stream)

        def reset_map():
            ctx.check(lib.svs_map_set_poses(rmap.h, P, pose_ids.ctypes.data, poses0.ctypes.data))
            ctx.check(lib.svs_map_set_points(rmap.h, L, point_ids.ctypes.data, xyz0.ctypes.data))

        def tail(h):
            ctx.check(lib.svs_ba_optimize(h, None, None, C.byref(st)))
            ctx.check(lib.svs_ba_get_state(h, out_poses.ctypes.data, out_psi.ctypes.data))
            xyz = BM.invert_depth(out_psi)
            ctx.check(lib.svs_map_set_poses(rmap.h, P, pose_ids.ctypes.data, out_poses.ctypes.data))
            ctx.check(lib.svs_map_set_points(rmap.h, L, point_ids.ctypes.data, xyz.ctypes.data))
            ctx.sync()

        def form_i():
            ctx.check(lib.svs_map_prepare_window(rmap.h, len(w0), w0.ctypes.data, t0.ctypes.data, len(pairs), pairs.ctypes.data, 1, 256, C.byref(res), wid.ctypes.data, wty.ctypes.data))
            ctx.check(lib.svs_ba_window_from_map(a.h, rmap.h, len(cons), cons.ctypes.data, C.byref(cam), C.byref(prm)))
            ctx.check(lib.svs_ba_optimize(a.h, None, None, C.byref(st)))
            ctx.check(lib.svs_ba_store_to_map(a.h, rmap.h))
            ctx.sync()

        def form_ii():
            ctx.check(lib.svs_ba_window_update(b.h, P, pose_ids.ctypes.data, poses0.ctypes.data, L, point_ids.ctypes.data, psi0.ctypes.data, anchor_ids.ctypes.data,
                                               len(obs_new), obs_new.ctypes.data, len(cons), cons.ctypes.data, C.byref(cam), C.byref(prm)))
            tail(b.h)

        def form_iii():
            ctx.check(lib.svs_ba_set_problem(d.h, P, poses0.ctypes.data, L, psi0.ctypes.data, len(by_idx), by_idx.ctypes.data, len(cons_idx), cons_idx.ctypes.data,
                                             C.byref(cam), C.byref(prm), 1))
            tail(d.h)

        # ---- the same bytes first: forms (i) and (ii) before the optimisation
        ctx.check(lib.svs_ba_window_update(b.h, P, pose_ids.ctypes.data, poses0.ctypes.data, L, point_ids.ctypes.data, psi0.ctypes.data, anchor_ids.ctypes.data,
                                           len(obs_old), obs_old.ctypes.data, len(cons), cons.ctypes.data, C.byref(cam), C.byref(prm)))
        ctx.check(lib.svs_ba_window_update(b.h, P, pose_ids.ctypes.data, poses0.ctypes.data, L, point_ids.ctypes.data, psi0.ctypes.data, anchor_ids.ctypes.data,
                                           len(obs_new), obs_new.ctypes.data, len(cons), cons.ctypes.data, C.byref(cam), C.byref(prm)))
        b.P, b.L = P, L
        rmap.prepare_window(w0, t0, pairs)
        a.windowFromMap(rmap, cons, cam, prm)
        sa, sb = a.restoreDataFromG2o(), b.restoreDataFromG2o()
        assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes() and a.window_edges().tobytes() == b.window_edges().tobytes()
        n_edges = len(a.window_edges())
        per_rep, trials = [], set()
        for _ in range(REPS):
            t = {k + s: [] for k in ("i", "ii", "iii") for s in ("_wall", "_dev")}
            for r in range(WARMUP + ROUNDS):
                for key, call in (("i", form_i), ("ii", form_ii), ("iii", form_iii)):
                    reset_map()
                    if key == "ii":
                        ctx.check(lib.svs_ba_window_forget_keyframes(b.h, newest.ctypes.data, 1))
                    ctx.sync()
                    ctx.timer_start()
                    t0_ = time.perf_counter()
                    call()
                    t1_ = time.perf_counter()
                    ms = ctx.timer_stop_ms()
                    trials.add((key, st.trials, st.accepted))
                    if r >= WARMUP:
                        t[key + "_wall"].append((t1_ - t0_) * 1e3); t[key + "_dev"].append(ms)
            per_rep.append({k: med(x) for k, x in t.items()})
        for key, form in (("i", "(i) prepare + from map + optimize + store to map"), ("ii", "(ii) window_update (one keyframe's observations) + optimize + get_state + set_poses / set_points"),
                          ("iii", "(iii) set_problem + optimize + get_state + set_poses / set_points")):
            w = [r[key + "_wall"] for r in per_rep]
            dv = [r[key + "_dev"] for r in per_rep]
            lines.append(f"| {name} | {P} | {L} | {n_edges} | {form} | {med(w):.3f} | {' / '.join(f'{x:.3f}' for x in w)} | {med(dv):.3f} |")
        notes.append(f"{name}: map of {rmap.info()} keyframes / points / observations; W0 of {len(w0)} ({int((t0 == 0).sum())} INNER), {len(pairs)} pairs, {len(cons)} constraints; form (ii) "
                     f"brings {len(obs_new)} observations; LM records (form, trials, accepted) seen: {sorted(trials)}")
        for o in (a, b, d):
            o.close()
        rmap.close()
    text = "\n".join(lines + [""] + notes + [f"medians over {ROUNDS} rounds behind {WARMUP}, {REPS} repetitions of the whole alternation (median of the repetitions, then each)"])
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
