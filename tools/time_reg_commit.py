"""One svs_reg_commit behind one registration at the reference's operating point -- covis_thr 15, a few hundred candidates, two qualifying keyframes -- beside the
composition a caller of the parent commit had to make: the three existing calls (svs_map_add_measured_observations, svs_map_add_edges, a storing
svs_map_compute_constraints with the pose override) on a twin map, with the lists already built on the host before the clock starts.  The scene is
tests/register_model.make_scene() put into a map by tests/register_map_model.fill(), with 8 twins of the root keyframe: every commit registers another twin, so
every commit finds a fresh root (136 of its pairs already present, as on the root of the tests).  Registrations run in batches of the 8 roots; a batch's 8
commits follow it one by one, and every batch gets a fresh pair of maps (built and touched once outside the clock), so that the observer rows stay as short as
the reference's: a point is seen by a handful of keyframes, not by hundreds of roots.  Times are the wall clock of the host around blocking calls, through the
Python binding.  The registration is also timed with every optional output and with the results alone: the difference is what the host composition needs
downloaded on top.
usage: python tools/time_reg_commit.py [--out FILE] [--resources-md FILE]
       python tools/time_reg_commit.py --resources      (no device: compiles register.hip and map.hip to assembly and prints the kernel resource table)"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

N_ROOTS, WARMUP, BATCH = 224, 24, 8
FIRST_TWIN = 100
KERNELS = [("register.hip", "reg_commit_kernel", "1 workgroup x 256"), ("map.hip", "map_commit_append_kernel", "1 workgroup x 512"),
           ("map.hip", "map_edge_add_kernel", "ceil(n_edges / 4) x 256 (unchanged)"), ("map.hip", "map_cons_kernel", "n_edges x 512 (unchanged)")]


def stat(a):
    a = np.asarray(a) * 1e3
    return "%.3f (%.3f .. %.3f)" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def resources():
    """the kernels' register, LDS and scratch use from the device assembly, compiled with the flags of the library's Makefile"""
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for unit in sorted({u for u, _, _ in KERNELS}):
            out = os.path.join(tmp, unit + ".s")
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-munsafe-fp-atomics", "-ffp-contract=off",
                                   "--offload-device-only", "-S", os.path.join(ROOT, "scavislam_amd", "csrc", unit), "-o", out])
            text = open(out).read()
            for u, name, launch in KERNELS:
                if u != unit:
                    continue
                m = [b for b in re.split(r"\n  - \.agpr_count:", text) if re.search(r"\.name:\s+\S*%s\S*\n" % name, b)]
                get = lambda key, blk: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                b = m[0]
                rows.append("| `%s` | %s | %d | %d | %d | %d |" % (name, launch, get("vgpr_count", b), get("sgpr_count", b), get("group_segment_fixed_size", b),
                                                                 get("private_segment_fixed_size", b)))
    return "\n".join(["| kernel | launch | VGPRs | SGPRs | LDS (bytes) | scratch |", "|---|---|---:|---:|---:|---:|"] + rows)


def main():
    if "--resources" in sys.argv:
        print(resources())
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res_md = open(sys.argv[sys.argv.index("--resources-md") + 1]).read() if "--resources-md" in sys.argv else None
    import torch
    import regcommit_model as RC
    import register_map_model as MM
    import register_model as M
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import RegMapRequest, RegResult
    from scavislam_amd.register import KeyframeRegistrar, ResidentMap, keyframe_table

    CAM = M.SMALL_CAM
    scene = M.make_scene()
    ctx, stream = capi.torch_context(0)
    with torch.cuda.stream(stream):
        pyrs = [[torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in pyr] for pyr in scene["kf_pyrs"]]
        disp = torch.as_tensor(np.ascontiguousarray(scene["root_disp"], np.float32)).cuda()
    ctx.sync()
    twins = list(range(FIRST_TWIN, FIRST_TWIN + BATCH))
    model = RC.CommitModel()
    MM.fill(RC.measured(model), scene, attach=lambda e: dict(entry=e))
    root_pairs = sorted(p for p, k in model.obs if k == MM.ROOT_ID)

    class Dev:
        def __init__(self):
            self.map = ResidentMap(ctx, max_keyframes=128, max_points=2048, max_observations=1 << 14)
            self.map.reserve_edges(64)

        def add_keyframes(self, ids, Ts, entry):
            kfs = keyframe_table([([t.data_ptr() for t in pyrs[e]], [t.shape[1] for t in pyrs[e]], T) for e, T in zip(entry, Ts)])
            self.map.add_keyframes(ids, kfs, [(disp.data_ptr(), disp.shape[1])] * len(ids), [scene["fast_thr"]] * len(ids))

        def __getattr__(self, name):
            return getattr(self.map, name)

    def build():
        d = Dev()
        MM.fill(RC.measured(d), scene, attach=lambda e: dict(entry=e))
        d.add_keyframes(twins, [scene["kf_T"][0]] * BATCH, entry=[0] * BATCH)
        for r in twins:
            d.add_measured_observations(root_pairs, [r] * len(root_pairs), [[float(v % 97), float(v % 89), 1.0] for v in root_pairs], [v % 3 for v in root_pairs])
        d.set_window([k for k in model.kf if model.kf[k]["window"]] + twins)
        # first use outside the clock: the download block, the scratch rows and two bitmap rows are allocated by the first constraint call of a map
        d.compute_constraints([dict(kf1=13, kf2=19, cached=cached), dict(kf1=19, kf2=13, cached=cached)])
        return d

    cached = {k: model.kf[k]["T"] for k in model.kf if not model.kf[k]["window"]}
    reg = KeyframeRegistrar(ctx, CAM, max_requests=BATCH, max_points=512, max_keyframes=8, max_observers=4096)
    level = {int(p["point_id"]): int(p["anchor_level"]) for p in scene["src"]}
    t_commit, t_three, t_obs, t_edges, t_cons, t_reg_all, t_reg_res = [], [], [], [], [], [], []
    n_track, n_added, n_edges, n_cand = [], [], [], []

    def results_only(dmap, qs):
        """svs_reg_register_map_batch with h_res alone"""
        arr, keep = (RegMapRequest * len(qs))(), []
        for i, q in enumerate(qs):
            walk, direct = np.array(q["walk_kf"], np.int32), np.array(q["direct_kf"], np.int32)
            keep += [walk, direct]
            arr[i].mode, arr[i].root_kf, arr[i].n_walk, arr[i].n_direct = q["mode"], q["root_kf"], len(walk), len(direct)
            arr[i].T_root_from_world[:] = np.asarray(q["T_root_from_world"], np.float64).reshape(12).tolist()
            arr[i].h_walk_kf, arr[i].h_direct_kf = walk.ctypes.data, direct.ctypes.data
        res = (RegResult * len(qs))()
        t0 = time.perf_counter()
        ctx.check(ctx.lib.svs_reg_register_map_batch(reg.h, dmap.map.h, len(qs), arr, C.byref(reg.params), res, None, None, None, None, None, None, None, None, None))
        return time.perf_counter() - t0

    one = twin = None
    for at in range(0, N_ROOTS, BATCH):
        for m in (one, twin):
            if m is not None:
                m.close()
        one, twin = build(), build()
        roots = twins
        qs = [MM.scene_request(scene, M.LOCAL, r) for r in roots]
        timed = at >= WARMUP
        dt = results_only(one, qs)
        t0 = time.perf_counter()
        outs = reg.register_map_batch(one.map, qs)
        dt_all = time.perf_counter() - t0
        if timed:
            t_reg_res.append(dt); t_reg_all.append(dt_all)
        lists = []
        for i, (r, o) in enumerate(zip(roots, outs)):
            t0 = time.perf_counter()
            got = reg.commit(one.map, i, cached=cached, resolve_missing=False)
            dt = time.perf_counter() - t0
            assert got["committed"] and all(x["status"] == 0 for x in got["edge_results"])
            if timed:
                t_commit.append(dt)
                n_track.append(got["n_track"]); n_added.append(got["n_pairs_added"]); n_edges.append(len(got["edges"])); n_cand.append(o.n_candidates)
            # the host composition's lists, from the registration's downloaded outputs: built before its clock starts
            at_id = {int(p): k for k, p in enumerate(o.point_ids)}
            idx = [at_id[int(g)] for g in got["track_point_ids"]]
            lists.append((r, got["T_new"], [int(g) for g in got["track_point_ids"]], o.matches["obs"][idx].copy(), [level[int(g)] for g in got["track_point_ids"]],
                          [(a, b) for a, b in got["edges"]], got["edge_strength"], reg.commit_raw["results"][:len(got["edges"])].tobytes()))
        for r, T_new, ids, centers, levels, edges, strength, want in lists:
            reqs = [dict(kf1=a, kf2=b, store=True, overrides=[(r, T_new)], cached=cached) for a, b in edges]
            t0 = time.perf_counter()
            twin.add_measured_observations(ids, [r] * len(ids), centers, levels)
            t1 = time.perf_counter()
            twin.add_edges(edges, strength, 1)
            t2 = time.perf_counter()
            twin.compute_constraints(reqs)
            t3 = time.perf_counter()
            assert twin.raw["results"].tobytes() == want
            if at >= WARMUP:
                t_three.append(t3 - t0); t_obs.append(t1 - t0); t_edges.append(t2 - t1); t_cons.append(t3 - t2)
        # what is timed is what the tests check: the two maps byte for byte
        all_edges = sorted(one.edge_keys)
        assert one.info() == twin.info() and one.edge_info() == twin.edge_info() and one.get_edges(all_edges).tobytes() == twin.get_edges(all_edges).tobytes()
        for r in twins[::3]:
            a, b = one.get_feature_table(r), twin.get_feature_table(r)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    lines = ["| what | wall, ms: median (10th .. 90th percentile) |", "|---|---:|",
             "| svs_reg_commit, per commit | %s |" % stat(t_commit),
             "| the three existing calls, the lists already built, per commit | %s |" % stat(t_three),
             "| - svs_map_add_measured_observations | %s |" % stat(t_obs),
             "| - svs_map_add_edges | %s |" % stat(t_edges),
             "| - svs_map_compute_constraints (storing, with the override; the CSR rebuild inside) | %s |" % stat(t_cons),
             "| svs_reg_register_map_batch of %d requests, every optional output | %s |" % (BATCH, stat(t_reg_all)),
             "| svs_reg_register_map_batch of %d requests, h_res alone | %s |" % (BATCH, stat(t_reg_res)),
             "",
             "scene: %d commits timed (%d more as warm-up), per commit %d candidates, %d track points of which %d bring a new pair, %d new edges (medians); covis_thr 15; "
             "every pair of maps ends with %d keyframes, %d points, %d pairs, %d edges and is byte for byte equal"
             % (len(t_commit), WARMUP, np.median(n_cand), np.median(n_track), np.median(n_added), np.median(n_edges), *one.info(), one.edge_info()[0])]
    text = "\n".join(lines)
    if res_md:
        text += "\n\n" + res_md.strip()
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")
    reg.close(); one.close(); twin.close()


if __name__ == "__main__":
    main()
