"""Times one drop cycle of the resident newpoint_map (newpoints.hip) for B = 1, 64, 512 streams and writes profiles/newpoints.md (or --out).

The state.  Every stream sees frame 0 of the synthetic 640 x 480 sequence, seeds its first keyframe (id 10, slot 0) into the store, takes its list from the store and
tracks frame 1.  Both paths then do the same work on the records of ONE step (untimed) per cycle -- two steps never leave the same records: the detector's thresholds
adapt from frame to frame -- in the same run: the host path's reading parts, the store's whole cycle, then the host path's upload (setting a list ends the validity of
the step's records, so it comes last).  Removed, seeded and listed counts of the two paths must agree in every cycle, and in the first the two lists byte for byte.
The store is put back to its state of before (untimed) behind every cycle.

  store    pruneNewpoints (all streams) + seedNewpoints (SVS_SEED_MORE into keyframe 11, one request per stream) + setCandidatesFromNewpoints (keys 11, 10; no tail):
           nothing but the counts and the per-stream results comes back, nothing but the requests goes up.
  host     the composition it replaces, from calls the parent commit has: seedKeyframes (the same requests, records downloaded), decideKeyframes(want_lists = 2) for the
           record indices of the matched new points (a one-vertex table per stream, set once), a NumPy prune of the host lists with them, and setCandidateListsAll with
           the pruned lists.  The parent's root-id hand-over (setNeighborhoodFromMap with a host head) uploads the same head records; it also walks a map, which no
           path here does, so the plain setter stands in for it on both sides' terms: bytes of the head only.
Host clock around blocking calls; WARMUP cycles first, median (min .. max) of CALLS.  Bytes moved are counted from the shapes.  Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, WARMUP = 10, 2
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def spread(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def run(ctx, stream, B):
    import torch
    import seed_common as S
    import seq_common
    from scavislam_amd import synth
    from scavislam_amd.ctypes_types import KEYFRAME_DECISION_DTYPE, MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE, SEED_FIRST, SEED_MORE, SeedParams
    from scavislam_amd.frontend import StereoFrontend
    cam = seq_common.cam_of("default")
    traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)
    T0 = np.stack([traj[0].reshape(12)] * B)
    fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2, n_streams=B)
    fe.reserveNewpoints(2048, 8)
    imgs = [S.frame("default", k) for k in (0, 1)]
    with torch.cuda.stream(stream):
        dev = [(torch.as_tensor(np.stack([i] * B)).cuda(), torch.as_tensor(np.stack([d] * B).astype(np.float32)).cuda()) for i, d in imgs]
    fe.processFirstFrames(left=dev[0][0], disp=dev[0][1])
    first = [dict(stream=b, mode=SEED_FIRST, kf_index=0, first_point_id=1, seed=5 + b, kf_id=10) for b in range(B)]
    lists0 = [r.copy() for r, _ in fe.seedKeyframes(first)]       # the host's newpoint_map[10] of every stream
    fe.seedNewpoints(first)
    fe.keepKeyframes(0, T0)
    slot = [10, -1]
    fe.setVertexTable([dict(stream=b, vertex_kf=[10], vertex_T=traj[0].reshape(1, 12), sets=[[]], act=0, neighbors=[], slot_kf=slot) for b in range(B)])
    more = [dict(stream=b, mode=SEED_MORE, kf_index=1, first_point_id=4000, seed=900 + b, kf_id=11) for b in range(B)]
    hand = [dict(stream=b, keys=[11, 10], slot_kf=slot) for b in range(B)]
    restore = [dict(stream=b, kf_id=10, records=lists0[b], mode=1) for b in range(B)]

    def step():
        fe.processFrames(np.stack([I34.reshape(12)] * B), T0, left=dev[1][0], disp=dev[1][1])
        ctx.sync()

    fe.setCandidatesFromNewpoints([dict(stream=b, keys=[10], slot_kf=slot) for b in range(B)])
    t_store, t_host, parts_store, parts_host = [], [], [], []
    n_removed = n_seeded = n_list = 0
    for it in range(WARMUP + CALLS):
        # ---- one step; both paths work on ITS records (the detector's thresholds adapt from frame to frame, so two steps never leave the same ones).  The host
        # path's first three parts only read; its upload comes last, behind the store's cycle, because setting a list ends the step's validity
        step()
        h0 = time.perf_counter()
        seeded = fe.seedKeyframes(more)
        h1 = time.perf_counter()
        dec = fe.decideKeyframes(want_lists=2)
        h2 = time.perf_counter()
        new_lists = []
        for b in range(B):
            gone = lists0[b]["point_id"][dec[b]["new_rec"]] if dec[b]["new_rec"] is not None else np.zeros(0, np.int32)
            kept = lists0[b][~np.isin(lists0[b]["point_id"], gone)]
            rec11 = seeded[b][0].copy()
            rec11["kf_index"], kept["kf_index"] = -1, 0
            new_lists.append((np.concatenate([rec11, kept]), [len(rec11), len(rec11) + len(kept), len(rec11) + len(kept)]))
        h3 = time.perf_counter()
        # ---- through the store
        t0 = time.perf_counter()
        pruned = fe.pruneNewpoints()
        t1 = time.perf_counter()
        cnt = fe.seedNewpoints(more)
        t2 = time.perf_counter()
        res = fe.setCandidatesFromNewpoints(hand, want_records=it == 0)
        t3 = time.perf_counter()
        n_removed, n_seeded, n_list = sum(p[0] for p in pruned), int(cnt.sum()), sum(r["n_points"] for r in res)
        h_removed, h_seeded = sum(len(lists0[b]) + len(seeded[b][0]) - len(new_lists[b][0]) for b in range(B)), sum(len(sd[0]) for sd in seeded)
        assert (h_removed, h_seeded, sum(len(l) for l, _ in new_lists)) == (n_removed, n_seeded, n_list), \
            f"the two paths differ: host removed / seeded / listed {h_removed} / {h_seeded} / {sum(len(l) for l, _ in new_lists)}, store {n_removed} / {n_seeded} / {n_list}"
        if it == 0:      # the two lists, byte for byte
            for b in range(B):
                assert res[0]["table"][b, :len(new_lists[b][0])].tobytes() == new_lists[b][0].tobytes(), f"stream {b}: the store's list is not the host's"
        h4 = time.perf_counter()
        fe.setCandidateListsAll([l for l, _ in new_lists], [g for _, g in new_lists])
        h5 = time.perf_counter()
        fe.dropNewpointGroups([dict(stream=b, keys=[11]) for b in range(B)])
        fe.putNewpoints(restore)
        fe.setCandidatesFromNewpoints([dict(stream=b, keys=[10], slot_kf=slot) for b in range(B)])
        if it >= WARMUP:
            t_store.append((t3 - t0) * 1e3); parts_store.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            t_host.append((h3 - h0 + h5 - h4) * 1e3); parts_host.append(((h1 - h0) * 1e3, (h2 - h1) * 1e3, (h3 - h2) * 1e3, (h5 - h4) * 1e3))
    n_step = max(fe.n_points)
    cap = SeedParams.reference().max_records()
    # bytes that cross the bus in one cycle, from the shapes
    store_bytes = B * (4 + 4 + 64 * 4) + B * (184 + 4 + 12) + B * (16 + 16 * 64) + B * 4
    host_bytes = B * (184 + 4 + 12) + (B * cap * 64 if B * cap * 64 <= 1 << 20 else n_seeded // max(B, 1) * 64 * B) \
        + B * KEYFRAME_DECISION_DTYPE.itemsize + B * n_step * (MAP_NEW_POINT_DTYPE.itemsize + MAP_TRACK_POINT_DTYPE.itemsize + 8) + B * 1024 * 64
    fe.close()
    col = lambda parts, k: spread([p[k] for p in parts])
    return dict(B=B, store=spread(t_store), host=spread(t_host), store_parts=[col(parts_store, k) for k in range(3)], host_parts=[col(parts_host, k) for k in range(4)],
                removed=n_removed // B, seeded=n_seeded // B, listed=n_list // B, store_bytes=store_bytes, host_bytes=host_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newpoints.md"))
    ap.add_argument("--streams", default="1,64,512")
    a = ap.parse_args()
    import torch
    from scavislam_amd import capi
    assert torch.cuda.is_available(), "needs a GPU"
    ctx, stream = capi.torch_context(0)
    rows = [run(ctx, stream, int(b)) for b in a.streams.split(",")]
    ctx.close()
    out = ["# One drop cycle of newpoint_map: through the resident store and through the host", "",
           f"`python tools/time_newpoints.py` on one MI355X; frame 0 / 1 of the synthetic 640 x 480 sequence on every stream; host clock around blocking calls; median (min .. max) of "
           f"{CALLS} cycles behind {WARMUP} warm-up cycles, the two paths alternating in one run.  The host path's prune is NumPy: an upper bound of a C++ walk, given on its own.  "
           "The parent's root-id hand-over uploads the same head records as the plain setter timed here and walks a map besides, which neither path does.", "",
           "| streams | store: whole cycle ms | prune | seed | hand-over | host: whole cycle ms | seedKeyframes + download | decideKeyframes + lists | NumPy prune | setCandidateListsAll | "
           "store KB moved | host KB moved | per stream: removed / seeded / listed |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['B']} | {r['store']} | {' | '.join(r['store_parts'])} | {r['host']} | {' | '.join(r['host_parts'])} | {r['store_bytes'] / 1024:.1f} | {r['host_bytes'] / 1024:.1f} | "
                   f"{r['removed']} / {r['seeded']} / {r['listed']} |")
    out += ["", "Bytes are counted from the shapes of the calls: requests, counts and result records for the store; for the host the seeded records (the longest list's width per "
            "request above 1 MiB of rows), the decision records, the list rows of `want_lists = 2` and the staged candidate block.  No bar was set in advance."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
