"""One svs_map_add_keyframe at the reference's operating point -- about 300 track points, 100 new points, observer rows of about 6, covis_thr 15 -- beside the same
insertion replayed through the five existing calls (svs_map_add_keyframes, _add_points, _add_measured_observations, _add_edges, a storing
_compute_constraints; their code is that of the parent commit) on a twin map, with the host computeStrength that replay needs timed separately: the literal
restatement of slam_graph.cpp:467-552 from tests/test_addkf_cpu.py and the closed form of tests/addkf_model.py (Python on this host's CPU: orientation only).
A trajectory of STEPS keyframes is inserted into both maps, alternating, so both see the same map at every step; every record array is built before the clock
starts; a step's time is the wall clock around calls that end in a device synchronise.  The first WARMUP steps are left out.  The two maps are compared at the end.
usage: python tools/time_add_keyframe.py [out.md]      (--model-only: the scene's figures, no device)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import addkf_model as AM

STEPS, WARMUP = 220, 20
N_NEW, N_TRACK, THR, HW, HH, WINDOW = 100, 300, 15, 320, 240, 12
med = lambda a: float(np.median(a))


def trajectory(seed=3):
    rng = np.random.default_rng(seed)
    g = AM.Graph()
    g.add_first_keyframe(10)
    keys, pid, steps, by_anchor = [10], 0, [], {}
    for i in range(STEPS):
        newkey, oldkey = 10 + 3 * (i + 1), keys[-1]
        new = []
        for _ in range(N_NEW):
            new.append(dict(point_id=pid, anchor_id=oldkey, xyz_anchor=[float(rng.uniform(-2, 2)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(3, 12))],
                            anchor_obs_pyr=rng.uniform(1, 300, 3).tolist(), anchor_level=int(rng.integers(3)), feat_center=rng.uniform(1, 600, 3).tolist(),
                            feat_level=int(rng.integers(3))))
            pid += 1
        # a track lives eight keyframes: of every keyframe's points the same part is followed (by_anchor holds them in a fixed random order)
        pool = [by_anchor[k] for k in keys[-9:-1] if k in by_anchor]
        track = []
        if pool:
            share = -(-N_TRACK // len(pool))
            for gid in rng.permutation([p for row in pool for p in row[:share]])[:N_TRACK]:
                track.append(dict(global_id=int(gid), center=[float(rng.uniform(0, 640)), float(rng.uniform(0, 480)), float(rng.uniform(0, 600))], level=int(rng.integers(3))))
        a = float(rng.uniform(-0.03, 0.03))
        T_rel = [float(np.cos(a)), -float(np.sin(a)), 0.0, float(rng.uniform(-0.1, 0.1)), float(np.sin(a)), float(np.cos(a)), 0.0, float(rng.uniform(-0.1, 0.1)), 0.0, 0.0, 1.0,
                 float(rng.uniform(-0.3, -0.1))]
        vis_before = {p: set(g.vis[p]) for t in track for p in [t["global_id"]]}
        out = g.add_keyframe(newkey, oldkey, T_rel, new, track, THR, HW, HH)
        by_anchor[oldkey] = [int(v) for v in rng.permutation([p["point_id"] for p in out["points"]])]
        steps.append(dict(newkey=newkey, oldkey=oldkey, T_rel=T_rel, new=new, track=track, out=out, vis=vis_before))
        keys.append(newkey)
    return steps, g


def main():
    args = sys.argv[1:]
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_addkf_cpu import literal_compute_strength
    steps, g = trajectory()
    tail = steps[WARMUP:]
    rows = [len(v) for s in tail for v in s["vis"].values()]
    t_lit, t_closed = [], []
    for s in tail[::10]:
        t0 = time.perf_counter()
        literal_compute_strength(s["new"], s["track"], s["vis"], THR, 2 * HW, 2 * HH)
        t1 = time.perf_counter()
        AM.strength_closed_form([p["anchor_id"] for p in s["new"]], [(t["global_id"], t["center"][0], t["center"][1]) for t in s["track"]], s["vis"], THR, HW, HH)
        t_lit.append((t1 - t0) * 1e3); t_closed.append((time.perf_counter() - t1) * 1e3)
    notes = [f"scene: {STEPS} insertions ({WARMUP} of them warm-up), per insertion {N_NEW} new points and {med([len(s['track']) for s in tail]):.0f} track points, observer rows of "
             f"{np.mean(rows):.1f} on average (max {max(rows)}), covis_thr {THR}; keys per insertion {med([len(s['out']['keys']) for s in tail]):.0f}, new edges "
             f"{med([len(s['out']['edges']) for s in tail]):.0f}, kept new points {med([sum(s['out']['kept']) for s in tail]):.0f}; the map ends with {len(g.pose)} keyframes, "
             f"{len(g.point)} points, {len(g.log)} pairs, {len(g.edges)} edges",
             f"host computeStrength (Python, this host's CPU, orientation only) ms per insertion: literal restatement {med(t_lit):.2f}, closed form {med(t_closed):.2f}"]
    if args and args[0] == "--model-only":
        print("\n".join(notes))
        return
    import torch
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    ctx, stream = capi.torch_context(0)
    with torch.cuda.stream(stream):
        any_u8 = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")      # the insertion reads no image
        any_f32 = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    ctx.sync()
    kf = keyframe_table([([any_u8.data_ptr()] * 3, [64] * 3, AM.I12)])
    disp, thr = (any_f32.data_ptr(), 64), [[25], [25], [25]]
    maps = []
    for _ in range(2):
        m = ResidentMap(ctx, max_keyframes=1024, max_points=1 << 15, max_observations=1 << 18)
        m.reserve_edges(1 << 14)
        maps.append(m)
    d, t = maps
    d.add_first_keyframe(10, kf, disp, thr)
    t.add_keyframes([10], kf, [disp], [thr])
    keys = [10]
    wall = dict(one=[], five=[], each=[[] for _ in range(5)])
    for i, s in enumerate(steps):
        out = s["out"]
        window = keys[-WINDOW:]
        d.set_window(window)
        t.set_window(window)
        # every record array before the clock starts
        np_rec, tp_rec = AM.new_point_records(s["new"], MAP_NEW_POINT_DTYPE), AM.track_point_records(s["track"], MAP_TRACK_POINT_DTYPE)
        kfr = kf.copy()
        kfr["T_anchor_from_w"][0] = out["pose"]
        pts = np.zeros(len(out["points"]), CANDIDATE_DTYPE)
        for o, p in zip(pts, out["points"]):
            o["xyz_anchor"], o["anchor_obs_pyr"], o["anchor_level"], o["kf_index"] = p["xyz_anchor"], p["anchor_obs_pyr"], p["anchor_level"], p["anchor_id"]
        pid = np.array([p["point_id"] for p in out["points"]], np.int32)
        pr = out["pairs"]
        pp, pk = np.array([q[0] for q in pr], np.int32), np.array([q[1] for q in pr], np.int32)
        pc, pl = np.array([q[2] for q in pr], np.float64).reshape(-1, 3), np.array([q[3] for q in pr], np.int32)
        ep, es = [(a, b) for a, b, _ in out["edges"]], [c for _, _, c in out["edges"]]
        reqs = [dict(kf1=a, kf2=b, store=True) for a, b in ep]
        ctx.sync()
        t0 = time.perf_counter()
        got = d.add_keyframe(s["newkey"], s["oldkey"], s["T_rel"], kf[0], disp, thr, np_rec, tp_rec, THR, HW, HH)
        t1 = time.perf_counter()
        marks = [time.perf_counter()]
        t.add_keyframes([s["newkey"]], kfr, [disp], [thr]); marks.append(time.perf_counter())
        t.add_points(pid, pts); marks.append(time.perf_counter())
        t.add_measured_observations(pp, pk, pc, pl); marks.append(time.perf_counter())
        t.add_edges(ep, es, 0); marks.append(time.perf_counter())
        res = t.compute_constraints(reqs); marks.append(time.perf_counter())      # blocking: ends in a synchronise
        assert got["edges"] == ep and got["new_kept"].tolist() == out["kept"]
        assert [o["info"].tobytes() for o in got["edge_results"]] == [o["info"].tobytes() for o in res]
        if i >= WARMUP:
            wall["one"].append((t1 - t0) * 1e3); wall["five"].append((marks[-1] - marks[0]) * 1e3)
            for k in range(5):
                wall["each"][k].append((marks[k + 1] - marks[k]) * 1e3)
        keys.append(s["newkey"])
    # the two maps are one map
    assert d.info() == t.info() and d.edge_info() == t.edge_info()
    assert d.get_edges([(a, b) for a, b, _ in g.edges]).tobytes() == t.get_edges([(a, b) for a, b, _ in g.edges]).tobytes()
    assert d.get_poses(sorted(g.pose)).tobytes() == t.get_poses(sorted(g.pose)).tobytes() and d.get_points(sorted(g.point)).tobytes() == t.get_points(sorted(g.point)).tobytes()
    q = lambda a: f"{med(a):.3f} ({np.percentile(a, 10):.3f} .. {np.percentile(a, 90):.3f})"
    names = ["svs_map_add_keyframes", "svs_map_add_points", "svs_map_add_measured_observations", "svs_map_add_edges", "svs_map_compute_constraints (storing; the CSR rebuild inside)"]
    lines = ["| what | wall per insertion, ms: median (10th .. 90th percentile) |", "|---|---:|", f"| svs_map_add_keyframe | {q(wall['one'])} |",
             f"| the five existing calls, the decision already made | {q(wall['five'])} |"] + [f"| - {n} | {q(a)} |" for n, a in zip(names, wall["each"])]
    text = "\n".join(lines + [""] + notes + [f"{STEPS - WARMUP} timed insertions, the two paths alternating on twin maps that are byte for byte equal at the end; through the Python binding"])
    print(text)
    if args and not args[0].startswith("--"):
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        open(args[0], "w").write(text + "\n")
    for m in maps:
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
