"""re-registration against a device-resident map (svs_map_*, svs_reg_register_map_batch) beside the stateless call (svs_reg_register_batch), on the scene of
tools/time_register.py: 640 x 480, about 1 500 source points, 1 and 32 requests (32 separate copies of the root frame, each a keyframe of the map).
Three forms alternate in one process, medians over 30 rounds behind a warm-up of each:
    stateless        the caller's tables staged on every call (the arrays are ready: the graph walk that makes them is NOT in the time)
    map              the request by ids
    update + map     the same behind the per-frame update a back end makes: one new keyframe, its 500 points, 1 500 observations, set_poses of a 50-keyframe
                     window -- so the call also rebuilds the map's CSR views
The whole alternation runs REPS times; the spread of the stateless form's medians over the repetitions is the yardstick for a difference.  Before it times, the
script checks that the map call returns the bytes of the stateless call.
usage: python tools/time_register_map.py [out.md]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import register_model as M
from scavislam_amd import synth

ROUNDS, NB, REPS = 30, 32, 3
CAM = synth.CAM_DEFAULT
N_NEW_PTS, N_NEW_OBS, N_WINDOW = 500, 1500, 50


def main():
    import torch
    from scavislam_amd import capi
    from scavislam_amd.frontend import FramePyramid
    from scavislam_amd.register import KeyframeRegistrar, ResidentMap, keyframe_table

    scene = M.make_scene(cam=CAM, n_per_kf=(300, 150, 50), seed=9)
    src = scene["src"]
    n_src, n_kf = len(src), len(scene["kf_T"])
    ctx, stream = capi.torch_context(0)
    frames = []
    for pyr in scene["kf_pyrs"]:
        fr = FramePyramid(ctx, stream, CAM, batch=1, with_float=False)
        fr.upload(pyr[0][None], scene["root_disp"][None])
        fr.preprocessing(with_float=False)
        frames.append(fr)
    roots = [frames[0]]
    for _ in range(NB - 1):
        fr = FramePyramid(ctx, stream, CAM, batch=1, with_float=False)
        fr.upload(scene["root_pyr"][0][None], scene["root_disp"][None])
        fr.preprocessing(with_float=False)
        roots.append(fr)
    ctx.sync()

    def request(root):
        ent = [([t.data_ptr() for t in (root if k == 0 else frames[k]).pyr], root.stride, scene["kf_T"][k]) for k in range(n_kf)]
        return dict(kfs=keyframe_table(ent), flags=scene["flags"], root_kf=0, root_disp=(root.disp.data_ptr(), root.stride[0]), fast_thr=scene["fast_thr"],
                    T_root_from_world=scene["T_root"], src=src, obs_begin=scene["obs_begin"], obs_kf=scene["obs_kf"])

    reg = KeyframeRegistrar(ctx, CAM, max_requests=NB, max_points=2048, max_keyframes=8, max_observers=8192)
    reqs = [request(r) for r in roots]

    # ---- the map: the scene's keyframes 1 .. under ids 7, 13, ..; the 32 roots under 100 ..; 50 window keyframes under 300 ..; the per-frame keyframes from 400
    ids = [7 + 6 * k for k in range(n_kf - 1)]
    root_ids = [100 + i for i in range(NB)]
    window_ids = [300 + i for i in range(N_WINDOW)]
    rmap = ResidentMap(ctx, max_keyframes=1024, max_points=1 << 17, max_observations=1 << 19)
    kf_of = lambda fr, T: ([t.data_ptr() for t in fr.pyr], fr.stride, T)
    disp_of = lambda fr: (fr.disp.data_ptr(), fr.stride[0])
    all_frames = [frames[k] for k in range(1, n_kf)] + roots + [frames[1]] * N_WINDOW
    all_T = [scene["kf_T"][k] for k in range(1, n_kf)] + [scene["kf_T"][0]] * NB + [scene["kf_T"][1]] * N_WINDOW
    rmap.add_keyframes(ids + root_ids + window_ids, keyframe_table([kf_of(f, T) for f, T in zip(all_frames, all_T)]), [disp_of(f) for f in all_frames],
                       [scene["fast_thr"]] * len(all_frames))
    table_id = [root_ids[0]] + ids
    pts = np.array(src)
    pts["kf_index"] = [table_id[int(e)] for e in src["kf_index"]]
    rmap.add_points(src["point_id"], pts)
    op = np.repeat(src["point_id"], np.diff(scene["obs_begin"]))
    ok = scene["obs_kf"]
    for e in range(1, n_kf):
        rmap.add_observations(op[ok == e], np.full(int((ok == e).sum()), ids[e - 1]))
    for r in root_ids:      # the root observes what entry 0 observes (it is a direct neighbour: the walk skips it, the observer rows hold it)
        rmap.add_observations(op[ok == 0], np.full(int((ok == 0).sum()), r))
    rmap.set_window([table_id[e] for e in range(1, n_kf) if int(scene["flags"][e]) & M.IN_WINDOW] + root_ids)
    mreqs = [dict(mode=M.LOCAL, root_kf=r, T_root_from_world=scene["T_root"], walk_kf=[r] + ids, direct_kf=[r, ids[0]]) for r in root_ids]
    window_T = np.array([scene["kf_T"][1]] * N_WINDOW)
    state = dict(next_kf=400, next_pt=int(src["point_id"].max()) + 1)
    rng = np.random.default_rng(0)

    def frame_update():
        """what addKeyframeToGraph and the optimiser's write-back send per frame"""
        kf, p0 = state["next_kf"], state["next_pt"]
        state["next_kf"], state["next_pt"] = kf + 1, p0 + N_NEW_PTS
        rmap.add_keyframes([kf], keyframe_table([kf_of(frames[1], scene["kf_T"][1])]), [disp_of(frames[1])], [scene["fast_thr"]])
        new = np.array(src[:N_NEW_PTS])
        new["kf_index"] = kf
        new_ids = np.arange(p0, p0 + N_NEW_PTS)
        rmap.add_points(new_ids, new)
        # the other observations: points of the last four keyframes (at the start: of the scene), as a camera that moves on sees them
        recent = np.arange(p0 - 4 * N_NEW_PTS, p0) if p0 - 4 * N_NEW_PTS > int(src["point_id"].max()) else src["point_id"]
        old = rng.choice(recent, N_NEW_OBS - N_NEW_PTS, replace=False)
        rmap.add_observations(np.concatenate([new_ids, old]), np.full(N_NEW_OBS, kf))
        rmap.set_poses(window_ids, window_T)

    def raw(i):
        r = reg.raw
        sz = len(r["results"]) // len(r["cand_src"])
        return (r["results"][i * sz:(i + 1) * sz],) + tuple(r[k][i].tobytes() for k in ("cand_src", "matches", "status_pass1", "accepted", "kf_stats"))

    lines = []
    with torch.cuda.stream(stream):
        # ---- the bytes first
        for n in (1, NB):
            reg.local_register(reqs[:n])
            want = [raw(i) for i in range(n)]
            outs = reg.register_map_batch(rmap, mreqs[:n])
            assert [raw(i) for i in range(n)] == want, "the map call does not return the bytes of the stateless call"
            assert all(o.status == 0 and list(o.kf_ids) == [root_ids[i]] + ids for i, o in enumerate(outs))
            frame_update()
            reg.register_map_batch(rmap, mreqs[:n])
            assert [raw(i) for i in range(n)] == want, "the per-frame update changed a request it does not touch"
        one = outs[0]
        med = lambda a: float(np.median(a)) * 1e3
        table = {}
        for n in (1, NB):
            per_rep = []
            for _ in range(REPS):
                t = dict(stateless=[], map=[], update_map=[], update=[])
                for _ in range(ROUNDS):
                    t0 = time.perf_counter(); reg.local_register(reqs[:n]); t["stateless"].append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); reg.register_map_batch(rmap, mreqs[:n]); t["map"].append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); frame_update(); t1 = time.perf_counter(); reg.register_map_batch(rmap, mreqs[:n]); t2 = time.perf_counter()
                    t["update"].append(t1 - t0); t["update_map"].append(t2 - t0)
                per_rep.append({k: med(v) for k, v in t.items()})
            table[n] = per_rep
    lines += [f"{n_src} source points, {one.n_candidates} candidates, {one.n_accepted} accepted, {one.n_qualified} keyframes qualify; map: {rmap.info()} keyframes / points / "
              f"observations at the end; medians over {ROUNDS} rounds, {REPS} repetitions of the whole alternation (median of the repetitions, then each)", "",
              "| requests | form | host time per call (ms) | per repetition | per request (ms) |", "|---:|---|---:|---|---:|"]
    for n in (1, NB):
        for k, name in (("stateless", "stateless call"), ("map", "map call"), ("update_map", "per-frame update + map call"), ("update", "(of which the four update calls)")):
            v = [rep[k] for rep in table[n]]
            lines.append(f"| {n} | {name} | {np.median(v):.3f} | {' / '.join(f'{x:.3f}' for x in v)} | {np.median(v) / n:.3f} |")
    lines.append("")
    for n in (1, NB):
        s = [rep["stateless"] for rep in table[n]]
        m = [rep["map"] for rep in table[n]]
        spread = max(s) - min(s)
        lines.append(f"{n} request(s): run-to-run spread of the stateless form {spread:.3f} ms; map form {np.median(m) - np.median(s):+.3f} ms against it "
                     f"({'below by more than the spread' if np.median(s) - np.median(m) > spread else 'not below by more than the spread'}; "
                     f"{'not above' if np.median(m) <= np.median(s) else 'ABOVE'} the stateless form)")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    rmap.close(); reg.close(); ctx.close()


if __name__ == "__main__":
    main()
