"""a stream's neighbourhood list built from the device-resident map (svs_frontend_set_candidates_from_map) beside the upload of the same list
(svs_frontend_set_candidates_all + one svs_frontend_keep_keyframes), in one process, for 1 and 64 streams, on two maps:
    scene       the test scene (tests/register_map_model.fill of register_model.make_scene at 320 x 240): vertex list of 2 keyframes, some 400 points
    synthetic   200 keyframes of 250 points each, a point observed by its anchor and by some of the four keyframes behind it; vertex list of 12 keyframes,
                a few thousand points -- near the reference's scale (findNeighborsOfRoot(root, 10))
Both forms are called through the C entry points with their arguments READY (request structs, concatenated records), so neither pays for a binding.  The upload
form is given the model-built list: the host's walk over its graph and the translation of anchor ids into slots, which the device call replaces, are NOT in its
time, and it refreshes ONE keyframe slot where the device call refreshes every slot -- the difference is a lower bound on the gain.
Per form: wall clock of the whole blocking call(s), and the span between two events on the context's stream around them (uploads, launch, download).  The two
forms alternate; medians over ROUNDS rounds behind a warm-up; the whole alternation runs REPS times.  Before it times, the script checks that both forms leave the
same records on the device.
usage: python tools/time_neighborhood.py [out.md]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import neighborhood_model as NM
import register_map_model as MM
import register_model as M

ROUNDS, WARMUP, REPS = 30, 5, 3
CAM = M.SMALL_CAM
K, MAX_POINTS, VCAP = 16, 8192, 64
I12 = np.array(M.I12)


def synthetic_map(rng, n_kf=200, per_kf=250):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    model = MM.MapModel()
    model.add_keyframes(list(range(n_kf)), [I12] * n_kf)
    pts = np.zeros(n_kf * per_kf, CANDIDATE_DTYPE)
    pts["xyz_anchor"] = rng.normal(size=(len(pts), 3)) + [0, 0, 8]
    pts["anchor_obs_pyr"] = rng.uniform(10, 200, size=(len(pts), 3))
    pts["anchor_level"] = rng.integers(0, 3, len(pts))
    pts["kf_index"] = np.arange(len(pts)) // per_kf
    model.add_points(list(range(len(pts))), pts)
    op, ok = [np.arange(len(pts))], [pts["kf_index"].copy()]
    for d in range(1, 5):
        seen = np.nonzero((rng.random(len(pts)) < 0.5) & (pts["kf_index"] + d < n_kf))[0]
        op.append(seen); ok.append(pts["kf_index"][seen] + d)
    model.add_observations(np.concatenate(op).tolist(), np.concatenate(ok).tolist())
    vertex = list(range(100, 112))
    return model, vertex, vertex + [-1] * (K - len(vertex))


def scene_map():
    scene = M.make_scene()
    model = MM.MapModel()
    MM.fill(model, scene, cand_ids_few=scene["src"]["point_id"][:10])
    ids = MM.scene_ids(scene)
    slots = ids[1:] + [MM.ROOT_ID]
    return model, [MM.ROOT_ID, ids[2]], slots + [-1] * (K - len(slots))


def device_map(ctx, model, frame):
    """the model's content in an svs_map; every keyframe's images are the one frame (the walk reads none of them)"""
    from scavislam_amd.register import ResidentMap, keyframe_table
    rmap = ResidentMap(ctx, max_keyframes=1024, max_points=1 << 16, max_observations=1 << 19)
    kf_ids = sorted(model.kf)
    ent = ([t.data_ptr() for t in frame.pyr], frame.stride, None)
    rmap.add_keyframes(kf_ids, keyframe_table([(ent[0], ent[1], model.kf[k]["T"]) for k in kf_ids]), [(frame.disp.data_ptr(), frame.stride[0])] * len(kf_ids),
                       [[np.full(9, 25), np.full(9, 25), np.full(4, 25)]] * len(kf_ids))
    pt_ids = sorted(model.pt)
    rmap.add_points(pt_ids, np.concatenate([model.pt[p].reshape(1) for p in pt_ids]))
    pairs = sorted(model.obs)
    rmap.add_observations([p for p, _ in pairs], [k for _, k in pairs])
    return rmap


def main():
    import torch
    from scavislam_amd import capi, synth
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, NbhRequest, NbhResult
    from scavislam_amd.frontend import FramePyramid, StereoFrontend

    ctx, stream = capi.torch_context(0)
    lib = ctx.lib
    img = synth.noise_image(CAM["w"], CAM["h"], 7)
    disp = np.full((CAM["h"], CAM["w"]), 6.0, np.float32)
    frame = FramePyramid(ctx, stream, CAM, batch=1, with_float=False)
    frame.upload(img[None], disp[None])
    frame.preprocessing(with_float=False)
    ctx.sync()
    rng = np.random.default_rng(0)
    med = lambda a: float(np.median(a))
    lines = ["| map | streams | points per list | vertices | form | wall per call (ms) | per repetition | stream span (ms) | wall per stream (ms) |", "|---|---:|---:|---:|---|---:|---|---:|---:|"]
    notes = []
    for name, (model, vertex, slots) in (("scene", scene_map()), ("synthetic", synthetic_map(rng))):
        rmap = device_map(ctx, model, frame)
        want = NM.build(model, vertex, slots, max_points=MAX_POINTS, vertex_cap=VCAP)
        assert not want["over_capacity"]
        n_kept = sum(1 for s in slots if s >= 0)
        for B in (1, 64):
            fe = StereoFrontend(ctx, CAM, max_points=MAX_POINTS, max_keyframes=K, n_streams=B)
            with torch.cuda.stream(stream):
                left = torch.as_tensor(np.stack([img] * B)).cuda()
                dd = torch.as_tensor(np.stack([disp] * B)).cuda()
            stream.synchronize()
            fe.processFirstFrames(left=left, disp=dd)
            poses = np.ascontiguousarray(np.stack([I12] * B))
            for s in range(n_kept):
                fe.keepKeyframes(s, poses)
            # ---- the arguments of both forms, ready
            v, sl = np.array(vertex, np.int32), np.array(slots, np.int32)
            ge1 = np.array([0], np.int32)
            req = (NbhRequest * B)()
            for b in range(B):
                req[b].stream, req[b].n_vertex, req[b].n_head, req[b].n_head_groups = b, len(v), 0, 1
                req[b].h_vertex_kf, req[b].h_slot_kf, req[b].h_head_group_end, req[b].h_head = v.ctypes.data, sl.ctypes.data, ge1.ctypes.data, None
            res = (NbhResult * B)()
            pid = np.empty((B, MAX_POINTS), np.int32)
            vid = np.empty((B, VCAP), np.int32)
            vT = np.empty((B, VCAP, 12))
            table = np.empty((B, MAX_POINTS), CANDIDATE_DTYPE)
            up_pts = np.ascontiguousarray(np.concatenate([want["records"]] * B))
            up_n = np.full(B, want["n_points"], np.int32)
            up_ge = np.ascontiguousarray(np.array([want["group_end"]] * B, np.int32))

            def from_map(records=None):
                ctx.check(lib.svs_frontend_set_candidates_from_map(fe.h, rmap.h, B, req, 1, VCAP, res, pid.ctypes.data, vid.ctypes.data, vT.ctypes.data, records))

            def from_map_lean():      # the list alone: no ids, no vertex set come back (the download is the counts and the slot poses)
                ctx.check(lib.svs_frontend_set_candidates_from_map(fe.h, rmap.h, B, req, 1, VCAP, res, None, None, None, None))

            def upload():
                ctx.check(lib.svs_frontend_set_candidates_all(fe.h, up_pts.ctypes.data, up_n.ctypes.data, up_ge.ctypes.data, 2))
                ctx.check(lib.svs_frontend_keep_keyframes(fe.h, 0, poses.ctypes.data))

            # ---- the same records first
            upload()
            from_map(table.ctypes.data)
            for b in range(B):
                assert table[b, :want["n_points"]].tobytes() == want["records"].tobytes() and res[b].n_points == want["n_points"] and not res[b].over_capacity
            fe.n_points = [want["n_points"]] * B
            per_rep = []
            for _ in range(REPS):
                t = dict(map_wall=[], map_dev=[], lean_wall=[], lean_dev=[], up_wall=[], up_dev=[])
                for i in range(WARMUP + ROUNDS):
                    for key, call in (("map", from_map), ("lean", from_map_lean), ("up", upload)):
                        ctx.timer_start()
                        t0 = time.perf_counter()
                        call()
                        t1 = time.perf_counter()
                        ms = ctx.timer_stop_ms()
                        if i >= WARMUP:
                            t[key + "_wall"].append((t1 - t0) * 1e3); t[key + "_dev"].append(ms)
                per_rep.append({k: med(x) for k, x in t.items()})
            for key, form in (("map", "from the map"), ("lean", "from the map, no id / vertex rows asked for"), ("up", "upload of the ready list + one keep_keyframes")):
                w = [r[key + "_wall"] for r in per_rep]
                d = [r[key + "_dev"] for r in per_rep]
                lines.append(f"| {name} | {B} | {want['n_points']} | {want['n_vertex']} | {form} | {med(w):.3f} | {' / '.join(f'{x:.3f}' for x in w)} | {med(d):.3f} | {med(w) / B:.4f} |")
            fe.close()
        notes.append(f"{name}: map of {rmap.info()} keyframes / points / observations, vertex list of {len(vertex)}, {want['n_no_slot']} records without a slot")
        rmap.close()
    text = "\n".join(lines + [""] + notes + [f"medians over {ROUNDS} rounds behind {WARMUP}, {REPS} repetitions of the whole alternation (median of the repetitions, then each)"])
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
