"""a stream's whole neighbourhood from a root id (svs_frontend_set_neighborhood_from_root) beside the four-call composition it replaces, in one process, for 1 and
64 requests at the reference's scale: a root with 11 in-window neighbours, some 3 800 points per list, two anchors outside the window that need a search.
    joined        StereoFrontend.setNeighborhoodFromMap: one call for the batch
    composition   per stream ResidentMap.neighbors_of_root (the host sort of the binding's edge log and one window query per candidate), then for the batch
                  absolute_poses of the vertices outside the window, set_poses with the result (which changes the map), setCandidatesFromMap with the vertex lists
                  and setVertexTable, whose strength_to_neighbors is looked up edge by edge in a host mirror of the edge table
Both go through the Python binding, so both pay for it.  The composition is GIVEN the ids of the anchors outside the window (a caller would have to learn them
from a first setCandidatesFromMap); that favours it.  The forms alternate; wall-clock medians over ROUNDS rounds behind a warm-up, the alternation REPS times;
the table shows the median of the repetitions, each repetition, and the fastest and slowest single call.  Before it times, the script checks that both forms leave
the same candidate records on the device.
usage: python tools/time_neighborhood_root.py [out.md]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import nbh_root_model as RM
import register_model as M
from time_neighborhood import CAM, I12, K, MAX_POINTS, VCAP, device_map, synthetic_map

ROUNDS, WARMUP, REPS = 30, 5, 3
ROOT_KF = 100


def edge_list(n_kf):
    """a chain over all keyframes (strength 30) and the root's eleven weaker edges to the keyframes behind it"""
    edges = [(k, k + 1, 30, 0) for k in range(n_kf - 1) if k != ROOT_KF]
    edges += [(ROOT_KF, ROOT_KF + j, 10 + j // 2, 0) for j in range(1, 12)]
    return edges


def main():
    import torch
    from constraint_model import EdgeTable
    from scavislam_amd import capi, synth
    from scavislam_amd.frontend import FramePyramid, StereoFrontend

    ctx, stream = capi.torch_context(0)
    img = synth.noise_image(CAM["w"], CAM["h"], 7)
    disp = np.full((CAM["h"], CAM["w"]), 6.0, np.float32)
    frame = FramePyramid(ctx, stream, CAM, batch=1, with_float=False)
    frame.upload(img[None], disp[None])
    frame.preprocessing(with_float=False)
    ctx.sync()
    rng = np.random.default_rng(0)
    model, _, _ = synthetic_map(rng)
    n_kf = len(model.kf)
    window = list(range(98, 116))                      # the anchors 96 and 97 of the list's points lie outside it: two searches per request
    model.set_window(window)
    for k in model.kf:
        model.kf[k]["T"] = np.array(synth.pose(synth.so3_exp(rng.normal(0, 0.1, 3)), rng.normal(0, 1.0, 3)).reshape(12))
    edges = edge_list(n_kf)
    table = EdgeTable()
    for a, b, s, ty in edges:
        table.insert(a, b, s, ty)
    rmap = device_map(ctx, model, frame)
    rmap.set_window(window)
    rmap.reserve_edges(len(edges))
    rmap.add_edges([(a, b) for a, b, _, _ in edges], [s for _, _, s, _ in edges], [t for _, _, _, t in edges])
    strength_of = {(min(a, b), max(a, b)): s for a, b, s, _ in edges}      # the caller's mirror of the edge table
    slots = list(range(ROOT_KF, ROOT_KF + 12)) + [-1] * (K - 12)
    want = RM.build(model, table, dict(root_id=ROOT_KF, act_id=ROOT_KF, slot_kf=slots), max_points=MAX_POINTS, vertex_cap=VCAP)
    assert not want["over_capacity"] and want["n_root_neighbors"] == 11
    vertex = [int(k) for k in want["vertex_ids"]]
    outside = [k for k in vertex if k not in window]
    stored = rmap.get_poses(outside)
    med = lambda a: float(np.median(a))
    lines = ["| requests | points per list | vertices | searches | form | wall per call (ms) | per repetition | fastest .. slowest call | wall per request (ms) |",
             "|---:|---:|---:|---:|---|---:|---|---|---:|"]
    for B in (1, 64):
        fe = StereoFrontend(ctx, CAM, max_points=MAX_POINTS, max_keyframes=K, n_streams=B)
        with torch.cuda.stream(stream):
            left = torch.as_tensor(np.stack([img] * B)).cuda()
            dd = torch.as_tensor(np.stack([disp] * B)).cuda()
        stream.synchronize()
        fe.processFirstFrames(left=left, disp=dd)
        for s in range(12):
            fe.keepKeyframes(s, np.ascontiguousarray(np.stack([I12] * B)))
        reqs = [dict(stream=b, root_id=ROOT_KF, act_id=ROOT_KF, slot_kf=slots) for b in range(B)]

        def joined(records=False):
            return fe.setNeighborhoodFromMap(rmap, reqs, refresh_poses=True, vertex_cap=VCAP, want_records=records)

        def composition(records=False):
            lists = [[ROOT_KF] + rmap.neighbors_of_root(ROOT_KF, 10).tolist() for _ in range(B)]
            T = rmap.absolute_poses(outside * B)[:len(outside)]
            rmap.set_poses(outside, [t["T"] for t in T])
            outs = fe.setCandidatesFromMap(rmap, [dict(stream=b, vertex_kf=lists[b], slot_kf=slots) for b in range(B)], refresh_poses=True, vertex_cap=VCAP,
                                           want_records=records)
            tabs = []
            for b, o in enumerate(outs):
                ids = o["vertex_ids"].tolist()
                nbrs = sorted((strength_of[(min(ROOT_KF, k), max(ROOT_KF, k))], k) for k in ids if k != ROOT_KF and (min(ROOT_KF, k), max(ROOT_KF, k)) in strength_of)
                tabs.append(dict(stream=b, vertex_kf=ids, vertex_T=o["vertex_T"], sets=["map"] * len(ids), act=ids.index(ROOT_KF),
                                 neighbors=[ids.index(k) for _, k in nbrs], slot_kf=slots))
            fe.setVertexTable(tabs)
            return outs

        a = joined(True)
        rec_joined = a[0]["table"].copy()
        assert a[0]["n_points"] == want["n_points"] and rec_joined[0, :want["n_points"]].tobytes() == want["records"].tobytes()
        c = composition(True)
        assert c[0]["table"].tobytes() == rec_joined.tobytes() and c[0]["vertex_T"].tobytes() == a[0]["vertex_T"].tobytes()
        rmap.set_poses(outside, stored)                  # (the composition leaves the searches' poses in the map)
        per_rep, every = [], dict(joined=[], composition=[])
        for _ in range(REPS):
            t = dict(joined=[], composition=[])
            for i in range(WARMUP + ROUNDS):
                for key, call in (("joined", joined), ("composition", composition)):
                    ctx.sync()
                    t0 = time.perf_counter()
                    call()
                    t1 = time.perf_counter()
                    if i >= WARMUP:
                        t[key].append((t1 - t0) * 1e3)
                rmap.set_poses(outside, stored)
            per_rep.append({k: med(x) for k, x in t.items()})
            for k in every:
                every[k] += t[k]
        for key, form in (("joined", "svs_frontend_set_neighborhood_from_root"), ("composition", "the four-call composition")):
            w = [r[key] for r in per_rep]
            lines.append(f"| {B} | {want['n_points']} | {want['n_vertex']} | {len(outside)} | {form} | {med(w):.3f} | {' / '.join(f'{x:.3f}' for x in w)} | "
                         f"{min(every[key]):.3f} .. {max(every[key]):.3f} | {med(w) / B:.4f} |")
        fe.close()
    notes = [f"map of {rmap.info()} keyframes / points / observations, {len(edges)} edges; root {ROOT_KF} with {want['n_root_neighbors']} in-window neighbours, "
             f"{want['n_no_slot']} records without a slot",
             f"wall-clock medians over {ROUNDS} rounds behind {WARMUP}, {REPS} repetitions of the alternation (median of the repetitions, then each); both forms through the Python binding"]
    text = "\n".join(lines + [""] + notes)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    rmap.close()
    ctx.close()


if __name__ == "__main__":
    main()
