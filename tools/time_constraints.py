"""computeConstraint on the device (svs_map_compute_constraints) and the window's constraints from the map's edge table (svs_ba_window_from_map_edges), timed on
the "large" map of tools/time_ba_from_map.py (50-keyframe window, feature_tables of about 2 000 points, 200 keyframes in all):
    1. svs_map_compute_constraints in batches of 1, 8 and 32 requests (pairs of keyframes one and two apart, every anchor in the window), wall clock and the span
       between two events on the context's stream; then the same with a stale CSR (one new observation before every timed call, outside the timing)
    2. form (i) of profiles/ba_from_map.md -- prepare_window + window from map + optimize + store_to_map -- with svs_ba_window_from_map_edges, beside the same
       form with the same constraints uploaded through svs_ba_window_from_map.  The constraints are the ones the OUTER keyframes' edges really produce: the edge
       table holds the scene's pairs and the chain, and every edge with an OUTER end in the final window is marginalised by a storing compute_constraints.
Medians over ROUNDS rounds behind a warm-up, the forms alternating; the whole alternation runs REPS times.
usage: python tools/time_constraints.py [out.md] [--cons-out list.npy]
       python tools/time_constraints.py --upload-only list.npy      form (i) with that list uploaded, nothing else: uses no call younger than svs_ba_window_from_map,
                                                                    so the same file times an older tree (copy it into that tree's tools/)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import ba_map_model as BM
from time_ba_from_map import large_scene

ROUNDS, WARMUP, REPS = 30, 5, 3
med = lambda a: float(np.median(a))


def fill(ctx, stream, m, measured):
    import torch
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    with torch.cuda.stream(stream):
        any_u8 = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")      # the walks read no image
        any_f32 = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    rmap = ResidentMap(ctx, max_keyframes=1024, max_points=1 << 16, max_observations=1 << 19)
    rmap.keep = (any_u8, any_f32)
    kfs = keyframe_table([([any_u8.data_ptr()] * 3, [64] * 3, T) for T in m["kf_poses"]])
    rmap.add_keyframes(m["kf_ids"], kfs, [(any_f32.data_ptr(), 64)] * len(kfs), [[[25], [25], [25]]] * len(kfs))
    pts = np.zeros(len(m["point_ids"]), CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = m["xyz"], m["anchor_ids"]
    rmap.add_points(m["point_ids"], pts)
    if measured:
        rmap.add_measured_observations(m["obs_point"], m["obs_kf"], m["obs_center"], m["obs_level"])
    else:
        rmap.add_observations(m["obs_point"], m["obs_kf"])
    return rmap


def timed(ctx, call, before=None):
    """-> (wall ms, stream span ms) medians per repetition"""
    reps = []
    for _ in range(REPS):
        w, d = [], []
        for r in range(WARMUP + ROUNDS):
            if before:
                before()
            ctx.sync()
            ctx.timer_start()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            ms = ctx.timer_stop_ms()
            if r >= WARMUP:
                w.append((t1 - t0) * 1e3); d.append(ms)
        reps.append((med(w), med(d)))
    return reps


def row(label, reps):
    w, d = [r[0] for r in reps], [r[1] for r in reps]
    return f"| {label} | {med(w):.3f} | {' / '.join(f'{x:.3f}' for x in w)} | {max(w) - min(w):.3f} | {med(d):.3f} |"


def form_i_upload(ctx, stream, sc, cons):
    """form (i) with `cons` uploaded: only calls the parent of this tool's commit has as well"""
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams, BaStats, Cam, MapWindowResult
    lib = ctx.lib
    m = sc["map"]
    rmap = fill(ctx, stream, m, True)
    prep = BM.prepare(m, sc["w0_ids"], sc["w0_types"], sc["pairs"])
    prob = BM.problem(m, prep["window_ids"], prep["active_ids"])
    c = sc["cam"]
    cam, prm = Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"]), BaParams.reference_defaults()
    w0, t0, pairs = (np.ascontiguousarray(sc[k]) for k in ("w0_ids", "w0_types", "pairs"))
    cons = np.ascontiguousarray(cons)
    P, L = len(prob["pose_ids"]), len(prob["point_ids"])
    pose_ids, point_ids = np.ascontiguousarray(prob["pose_ids"], np.int32), np.ascontiguousarray(prob["point_ids"], np.int32)
    poses0, xyz0 = np.ascontiguousarray(prob["poses"]), np.ascontiguousarray(BM.invert_depth(prob["psi"]))
    res, wid, wty, st = MapWindowResult(), np.zeros(256, np.int32), np.zeros(256, np.int32), BaStats()
    a = SlamGraphOptimizer(ctx, stream)

    def reset_map():
        ctx.check(lib.svs_map_set_poses(rmap.h, P, pose_ids.ctypes.data, poses0.ctypes.data))
        ctx.check(lib.svs_map_set_points(rmap.h, L, point_ids.ctypes.data, xyz0.ctypes.data))

    def call():
        ctx.check(lib.svs_map_prepare_window(rmap.h, len(w0), w0.ctypes.data, t0.ctypes.data, len(pairs), pairs.ctypes.data, 1, 256, C.byref(res), wid.ctypes.data, wty.ctypes.data))
        ctx.check(lib.svs_ba_window_from_map(a.h, rmap.h, len(cons), cons.ctypes.data if len(cons) else None, C.byref(cam), C.byref(prm)))
        ctx.check(lib.svs_ba_optimize(a.h, None, None, C.byref(st)))
        ctx.check(lib.svs_ba_store_to_map(a.h, rmap.h))
        ctx.sync()
    reps = timed(ctx, call, reset_map)
    a.close(); rmap.close()
    return reps, (P, L, len(cons), st.trials, st.accepted)


def main():
    from scavislam_amd import capi
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams, BaStats, Cam, MapWindowResult
    ctx, stream = capi.torch_context(0)
    lib = ctx.lib
    sc = large_scene()
    m = sc["map"]
    args = sys.argv[1:]
    head = ["| what | wall per call (ms) | per repetition | spread of the repetitions | stream span (ms) |", "|---|---:|---|---:|---:|"]
    if args and args[0] == "--upload-only":
        reps, shape = form_i_upload(ctx, stream, sc, np.load(args[1]))
        print("\n".join(head + [row(f"form (i), {shape[2]} constraints uploaded (window {shape[0]}, {shape[1]} points; LM trials / accepted {shape[3]} / {shape[4]})", reps)]))
        ctx.close()
        return
    lines = list(head)
    notes = []
    kf = [int(k) for k in m["kf_ids"]]
    win = kf[150:]
    # ---- 1. svs_map_compute_constraints
    rmap = fill(ctx, stream, m, False)
    rmap.set_window(win)
    seen = [k for k in win if (m["obs_kf"] == k).any()]                   # (the scene's last three keyframes are held by constraints alone)
    reqs_all = [dict(kf1=seen[i], kf2=seen[i + d]) for i in range(0, len(seen) - 2, 2) for d in (1, 2)]
    spare = iter([(int(p), win[0]) for p in m["point_ids"][20000:]])       # pairs the map does not hold yet: points of the other keyframes, seen by the window's first
    for n in (1, 8, 32):
        reqs = reqs_all[:n]
        out = rmap.compute_constraints(reqs)
        assert all(o["status"] == 0 for o in out)
        call = lambda: rmap.compute_constraints(reqs, missing_cap=0)
        lines.append(row(f"compute_constraints, {n} request(s), common points {min(o['strength'] for o in out)} .. {max(o['strength'] for o in out)}", timed(ctx, call)))

        def stale():
            p, k = next(spare)
            rmap.add_observations([p], [k])
        lines.append(row(f"the same behind a new observation (CSR rebuild of {rmap.info()[2]} pairs inside)", timed(ctx, call, stale)))
    notes.append(f"1: map of {rmap.info()} keyframes / points / observations, feature_tables of the window's keyframes {min(len(np.nonzero(m['obs_kf'] == k)[0]) for k in win)} .. "
                 f"{max(len(np.nonzero(m['obs_kf'] == k)[0]) for k in win)} points; through the Python binding (request structures built per call)")
    rmap.close()
    # ---- 2. form (i): the constraints from the edge table against the same list uploaded
    rmap = fill(ctx, stream, m, True)
    _, wid, wty = rmap.prepare_window(sc["w0_ids"], sc["w0_types"], sc["pairs"])
    types = dict(zip(wid.tolist(), wty.tolist()))
    # the scene's own constraints hold its last three keyframes, which observe nothing: those edges take the caller's values (svs_map_set_constraints); every
    # other edge with an OUTER end is marginalised by computeConstraint on the device
    given = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in zip(sc["cons"]["pose1"], sc["cons"]["pose2"])}
    seen = {k for k in kf if (m["obs_kf"] == k).any()}
    keys = sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in sc["pairs"]} | {(kf[i], kf[i + 1]) for i in range(150, len(kf) - 1) if kf[i + 1] in seen} | given)
    rmap.reserve_edges(len(keys))
    rmap.add_edges(keys, 30, 0)
    rmap.set_constraints(sc["cons"])
    outer = [(a, b) for a, b in keys if a in types and b in types and (types[a] == 1 or types[b] == 1) and (a, b) not in given]
    out = rmap.compute_constraints([dict(kf1=a, kf2=b, store=True) for a, b in outer])
    assert all(o["status"] == 0 for o in out), [o["status"] for o in out]
    c = sc["cam"]
    cam, prm = Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"]), BaParams.reference_defaults()
    a = SlamGraphOptimizer(ctx, stream)
    a.windowFromMap(rmap, None, cam, prm)
    cons = a.window_constraints()
    cons["pose1"], cons["pose2"] = wid[cons["pose1"]], wid[cons["pose2"]]                      # frame ids, as svs_ba_window_from_map takes them
    for i, arg in enumerate(args):
        if arg == "--cons-out":
            np.save(args[i + 1], cons)
    prep = BM.prepare(m, sc["w0_ids"], sc["w0_types"], sc["pairs"])
    prob = BM.problem(m, prep["window_ids"], prep["active_ids"])
    w0, t0, pairs = (np.ascontiguousarray(sc[k]) for k in ("w0_ids", "w0_types", "pairs"))
    P, L = len(prob["pose_ids"]), len(prob["point_ids"])
    pose_ids, point_ids = np.ascontiguousarray(prob["pose_ids"], np.int32), np.ascontiguousarray(prob["point_ids"], np.int32)
    poses0, xyz0 = np.ascontiguousarray(prob["poses"]), np.ascontiguousarray(BM.invert_depth(prob["psi"]))
    res, wid2, wty2, st = MapWindowResult(), np.zeros(256, np.int32), np.zeros(256, np.int32), BaStats()

    def reset_map():
        ctx.check(lib.svs_map_set_poses(rmap.h, P, pose_ids.ctypes.data, poses0.ctypes.data))
        ctx.check(lib.svs_map_set_points(rmap.h, L, point_ids.ctypes.data, xyz0.ctypes.data))

    def form(edges):
        ctx.check(lib.svs_map_prepare_window(rmap.h, len(w0), w0.ctypes.data, t0.ctypes.data, len(pairs), pairs.ctypes.data, 1, 256, C.byref(res), wid2.ctypes.data, wty2.ctypes.data))
        if edges:
            ctx.check(lib.svs_ba_window_from_map_edges(a.h, rmap.h, C.byref(cam), C.byref(prm)))
        else:
            ctx.check(lib.svs_ba_window_from_map(a.h, rmap.h, len(cons), cons.ctypes.data, C.byref(cam), C.byref(prm)))
        ctx.check(lib.svs_ba_optimize(a.h, None, None, C.byref(st)))
        ctx.check(lib.svs_ba_store_to_map(a.h, rmap.h))
        ctx.sync()
    # the two forms alternate inside every round
    per = {True: [], False: []}
    for _ in range(REPS):
        t = {True: ([], []), False: ([], [])}
        for r in range(WARMUP + ROUNDS):
            for edges in (True, False):
                reset_map()
                ctx.sync()
                ctx.timer_start()
                t0_ = time.perf_counter()
                form(edges)
                t1_ = time.perf_counter()
                ms = ctx.timer_stop_ms()
                if r >= WARMUP:
                    t[edges][0].append((t1_ - t0_) * 1e3); t[edges][1].append(ms)
        for e in (True, False):
            per[e].append((med(t[e][0]), med(t[e][1])))
    lines.append(row(f"form (i) with svs_ba_window_from_map_edges ({len(cons)} constraints gathered on the device; window {P}, {L} points)", per[True]))
    lines.append(row(f"form (i) with the same {len(cons)} constraints uploaded (svs_ba_window_from_map), this tree", per[False]))
    notes.append(f"2: {len(keys)} edges, {len(outer)} with an OUTER end in the final window marginalised by compute_constraints and {len(given)} by set_constraints; LM trials / accepted of the last call {st.trials} / {st.accepted}")
    a.close(); rmap.close()
    text = "\n".join(lines + [""] + notes + [f"medians over {ROUNDS} rounds behind {WARMUP}, {REPS} repetitions of the whole alternation (median of the repetitions, then each, then max - min)"])
    print(text)
    if args and not args[0].startswith("--"):
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        open(args[0], "w").write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
