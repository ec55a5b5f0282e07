"""The pose graph's walks on the device-resident map (svs_map_initial_windows, svs_map_frames_in_neighborhood, svs_map_absolute_poses, svs_map_reinitialize_poses,
svs_map_prepare_window_from_root), timed at the reference's scale: inner window 25 / double window 200 (backend.cpp:141-144), neighbourhood 40 (:552), 10 and 100
absolute poses per call.  The graph is a trajectory of N_KF keyframes: each joins the COVIS keyframes before it with strengths that fall with the distance (runs
of equal values), and every 97th keyframe closes a loop to one far behind it.  Per entry point: wall clock and the span between two events on the context's
stream (medians over ROUNDS rounds behind a warm-up, REPS repetitions), the same call behind an svs_map_add_edges (the adjacency rebuild inside), and -- for
orientation only, a CPU figure about a Python model -- the time of the same walk in tests/walk_model.py.
usage: python tools/time_walk.py [out.md]      (--model-only: the scene and the model's times, no device)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import constraint_model as CM
import walk_model as WM

ROUNDS, WARMUP, REPS = 30, 5, 3
N_KF, COVIS, SPARE = 2000, 8, 400
INNER, DOUBLE, NBH = 25, 200, 40
med = lambda a: float(np.median(a))


def trajectory(seed=7):
    from scavislam_amd import synth
    rng = np.random.default_rng(seed)
    ids = [CM.kf_id(i) for i in range(N_KF)]
    poses = {k: [float(v) for v in synth.pose(synth.so3_exp(rng.normal(0, 0.2, 3)), rng.normal(0, 2.0, 3)).reshape(12)] for k in ids}
    edges = []
    for i in range(1, N_KF):
        for d in range(1, min(COVIS, i) + 1):
            edges.append((ids[i - d], ids[i], 60 - 6 * d + int(rng.integers(0, 3)), 0))
        if i % 97 == 0 and i > 300:
            edges.append((ids[i - 250 - int(rng.integers(0, 40))], ids[i], 25, 2))
    table = CM.EdgeTable()
    for a, b, s, t in edges:
        table.insert(a, b, s, t)
    marg = [(lo, hi) for k, (lo, hi) in enumerate(table.e) if k % 3 == 0]
    for lo, hi in marg:
        table.set_constraint(lo, hi, CM.pose_mul(poses[lo], CM.pose_inv(poses[hi])), np.eye(6).reshape(36))
    return dict(ids=ids, poses=poses, edges=edges, table=table, marg=marg)


def fill(ctx, stream, sc):
    import torch
    from scavislam_amd.ctypes_types import BA_CONSTRAINT_DTYPE, CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    with torch.cuda.stream(stream):
        any_u8 = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")      # the walks read no image
        any_f32 = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    ids = sc["ids"]
    rmap = ResidentMap(ctx, max_keyframes=8192, max_points=1 << 14, max_observations=1 << 16)
    rmap.keep = (any_u8, any_f32)
    kfs = keyframe_table([([any_u8.data_ptr()] * 3, [64] * 3, sc["poses"][k]) for k in ids])
    rmap.add_keyframes(ids, kfs, [(any_f32.data_ptr(), 64)] * len(kfs), [[[25], [25], [25]]] * len(kfs))
    # one point per keyframe, seen there and in the next: enough for svs_map_prepare_window_from_root to have something to mark
    pts = np.zeros(len(ids), CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = [[0.1, -0.2, 4.0]] * len(ids), ids
    rmap.add_points(np.arange(len(ids)), pts)
    p = np.concatenate([np.arange(len(ids)), np.arange(len(ids) - 1)])
    k = np.concatenate([np.array(ids), np.array(ids[1:])])
    rmap.add_measured_observations(p, k, np.full((len(p), 3), 100.0), np.zeros(len(p), np.int32))
    rmap.reserve_edges(len(sc["edges"]) + SPARE)
    rmap.add_edges([(a, b) for a, b, _, _ in sc["edges"]], [s for _, _, s, _ in sc["edges"]], [t for _, _, _, t in sc["edges"]])
    cons = np.zeros(len(sc["marg"]), BA_CONSTRAINT_DTYPE)
    for c, (lo, hi) in zip(cons, sc["marg"]):
        c["T_21"], c["info"], c["pose1"], c["pose2"] = sc["table"].e[(lo, hi)]["T"], np.eye(6).reshape(36), hi, lo
    rmap.set_constraints(cons)
    return rmap


def timed(ctx, call, before=None):
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


def host_ms(call, n=5):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return med(t)


def main():
    args = sys.argv[1:]
    sc = trajectory()
    ids, table, poses = sc["ids"], sc["table"], sc["poses"]
    root = ids[1500]
    adj = WM.adjacency(table)
    w_ids, w_types = WM.initial_window(adj, root, INNER, DOUBLE)
    window = set(w_ids)
    far = [k for k in ids[1100:1400] if k not in window]
    old_ids, _ = WM.initial_window(adj, ids[1490], INNER, DOUBLE)
    pairs = WM.inner_pairs(adj, w_ids, w_types)
    model = {
        "initial window, 1 root": host_ms(lambda: WM.initial_window(adj, root, INNER, DOUBLE)),
        "initial windows, 8 roots": host_ms(lambda: [WM.initial_window(adj, ids[1500 - 20 * j], INNER, DOUBLE) for j in range(8)]),
        "frames in neighbourhood": host_ms(lambda: WM.frames_in_neighborhood(adj, w_ids, root, NBH)),
        "absolute poses, 10": host_ms(lambda: [WM.absolute_pose(adj, window, table, poses, x) for x in far[:10]]),
        "absolute poses, 100": host_ms(lambda: [WM.absolute_pose(adj, window, table, poses, x) for x in far[:100]]),
        "reinitialise": host_ms(lambda: WM.reinitialize_poses(adj, w_ids, table, poses, root, old_ids, -1)),
        "window from root": float("nan"),
        "adjacency": host_ms(lambda: WM.adjacency(table), 3),
    }
    paths = [len(WM.shortest_path_to_window(adj, window, x)) for x in far[:100]]
    notes = [f"graph: {len(ids)} keyframes, {len(table.e)} edges ({len(sc['marg'])} marginalised), longest row {max(len(r) for r in adj.values())}; window from keyframe index 1500: "
             f"{len(w_ids)} keyframes; absolute poses of keyframes {min(paths)} .. {max(paths)} keyframes of path away; reinitialise against the window of index 1490 "
             f"({len(WM.reinitialize_poses(adj, w_ids, table, poses, root, old_ids, -1)[0])} poses rewritten); {len(pairs)} pairs of the INNER rows",
             f"walk_model (Python, this host's CPU, orientation only) ms: " + ", ".join(f"{k} {v:.2f}" for k, v in model.items())]
    if args and args[0] == "--model-only":
        print("\n".join(notes))
        return
    from scavislam_amd import capi
    ctx, stream = capi.torch_context(0)
    rmap = fill(ctx, stream, sc)
    rmap.set_window(w_ids)
    spare = iter([(ids[i], ids[i + 900]) for i in range(SPARE)])

    def stale():
        a, b = next(spare)
        rmap.add_edges([(a, b)], 1, 0)
    head = ["| what | wall per call (ms) | per repetition | spread of the repetitions | stream span (ms) | walk_model on the host (ms) |", "|---|---:|---|---:|---:|---:|"]

    def row(label, reps, key):
        w, d = [r[0] for r in reps], [r[1] for r in reps]
        return f"| {label} | {med(w):.3f} | {' / '.join(f'{x:.3f}' for x in w)} | {max(w) - min(w):.3f} | {med(d):.3f} | {model[key]:.2f} |"
    roots8 = [ids[1500 - 20 * j] for j in range(8)]
    calls = [
        ("svs_map_initial_windows, 1 root, 25 / 200", lambda: rmap.initial_windows([root], INNER, DOUBLE), "initial window, 1 root"),
        ("svs_map_initial_windows, 8 roots", lambda: rmap.initial_windows(roots8, INNER, DOUBLE), "initial windows, 8 roots"),
        ("svs_map_frames_in_neighborhood, 1 root, 40", lambda: rmap.frames_in_neighborhood([root], NBH), "frames in neighbourhood"),
        ("svs_map_absolute_poses, 10 keyframes", lambda: rmap.absolute_poses(far[:10]), "absolute poses, 10"),
        ("svs_map_absolute_poses, 100 keyframes", lambda: rmap.absolute_poses(far[:100]), "absolute poses, 100"),
    ]
    lines = list(head)
    for label, call, key in calls:
        lines.append(row(label, timed(ctx, call), key))
    lines.append(row("svs_map_initial_windows, 1 root, behind an svs_map_add_edges (adjacency rebuild inside)", timed(ctx, calls[0][1], stale), "adjacency"))
    rmap.close()
    # the check rides along, on a fresh map (the spare edges changed the first one's graph): what is timed is what the model gives
    rmap = fill(ctx, stream, sc)
    rmap.set_window(w_ids)
    assert rmap.initial_windows([root], INNER, DOUBLE)[0][0].tolist() == w_ids
    assert rmap.frames_in_neighborhood([root], NBH)[0].tolist() == WM.frames_in_neighborhood(adj, w_ids, root, NBH)
    for o, x in zip(rmap.absolute_poses(far[:100]), far[:100]):
        assert o["T"].tobytes() == np.array(WM.absolute_pose(adj, window, table, poses, x)[2]).tobytes()
    start = np.array([poses[k] for k in ids])
    lines.append(row("svs_map_reinitialize_poses, window of 200 (poses put back before every call, outside the timing)",
                     timed(ctx, lambda: rmap.reinitialize_poses(root, old_ids, -1), lambda: rmap.set_poses(ids, start)), "reinitialise"))
    lines.append(row("svs_map_prepare_window_from_root, 25 / 200", timed(ctx, lambda: rmap.prepare_window_from_root(root, INNER, DOUBLE)), "window from root"))
    lines.append(row("svs_map_prepare_window with W0 and the pairs ready on the host", timed(ctx, lambda: rmap.prepare_window(w_ids, w_types, pairs)), "window from root"))
    rmap.close()
    text = "\n".join(lines + [""] + notes + [f"medians over {ROUNDS} rounds behind {WARMUP}, {REPS} repetitions (median of the repetitions, then each, then max - min); through the Python binding"])
    print(text)
    if args and not args[0].startswith("--"):
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        open(args[0], "w").write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
