"""re-registration of a keyframe against the map (svs_reg_register_batch; Backend::localRegisterFrame, backend.cpp:549-611): host time of the ONE call for 1 and for
32 requests at 640 x 480 with about 1 500 source points each, its per-stage device times from the library's own events (svs_reg_set_timing), and beside them what a
caller does for one request WITHOUT the call, from the entry points that were there before it (the tools/two_threads.py pattern): cull on the host (vectorised
NumPy), the stored thresholds into the FastGrid, svs_fast_detect(trials = 0), svs_match at radius 10, download, svs_motion_only(25), download, svs_match at radius 4,
download, svs_motion_only(15), svs_process_matched_points, download, the observer walk on the host (vectorised NumPy).
usage: python tools/time_register.py [out.md]
Prints a markdown table (and writes it when a path is given).  Both forms end in a device synchronise, so the host clock around them is the time a back-end thread
waits; rounds alternate between the forms in one process.  The script checks that both forms reach the same decision, the same strengths and the same pose."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import register_model as M
from scavislam_amd import synth

ROUNDS, NB = 30, 32
CAM = synth.CAM_DEFAULT


def host_cull(req, cams):
    """pointsVisibleInRoot (backend.cpp:472-546) the way a caller writes it in NumPy: one relative pose per keyframe, the points as arrays"""
    src, flags = req["src"], req["flags"]
    kf, lvl = src["kf_index"], src["anchor_level"]
    T = np.array([M.pose_mul(req["T_root"], M.pose_inv(t)) for t in req["kf_T"]]).reshape(-1, 3, 4)[kf]
    p = np.einsum("nij,nj->ni", T[:, :, :3], src["xyz_anchor"]) + T[:, :, 3]
    f, cx, cy = cams["f"][lvl], cams["cx"][lvl], cams["cy"][lvl]
    with np.errstate(all="ignore"):
        u, v = f * (p[:, 0] / p[:, 2]) + cx, f * (p[:, 1] / p[:, 2]) + cy
    ok = (np.abs(u) < 2 ** 31) & (np.abs(v) < 2 ** 31)
    ui, vi = np.where(ok, u, -1).astype(np.int64), np.where(ok, v, -1).astype(np.int64)      # astype truncates toward zero
    keep = ok & ((flags[kf] & M.IN_WINDOW) != 0) & (ui >= 0) & (vi >= 0) & (ui < cams["w"][lvl]) & (vi < cams["h"][lvl])
    idx = np.nonzero(keep)[0]
    in_vt = np.zeros(len(flags), bool)
    in_vt[req["root_kf"]] = True
    in_vt[np.unique(kf[idx])] = True
    return idx, in_vt


def host_count(req, idx, accepted, uvu, in_vt, covis):
    """keyframesToRegister's counters (backend.cpp:628-721) in NumPy: one row of (observer, half) pairs per accepted observation"""
    n_kf = len(req["flags"])
    a = idx[np.nonzero(accepted)[0]]
    ob, ok = req["obs_begin"], req["obs_kf"]
    cnt = (ob[a + 1] - ob[a]).astype(np.int64)
    rows = np.repeat(np.arange(len(a)), cnt)
    ent = np.repeat(ob[a].astype(np.int64), cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    kfs = ok[ent]
    use = in_vt[kfs] & ((req["flags"][kfs] & M.DIRECT_NEIGHBOR) == 0)
    kfs, rows = kfs[use], rows[use]
    obs = uvu[np.nonzero(accepted)[0]][rows]
    st = np.zeros((n_kf, 5), np.int64)
    st[:, 0] = np.bincount(kfs, minlength=n_kf)
    st[:, 1] = np.bincount(kfs[obs[:, 0] > CAM["w"] * 0.5], minlength=n_kf)
    st[:, 3] = np.bincount(kfs[obs[:, 1] > CAM["h"] * 0.5], minlength=n_kf)
    st[:, 2], st[:, 4] = st[:, 0] - st[:, 1], st[:, 0] - st[:, 3]
    q = (st[:, 0] >= covis) & (st[:, 1:] >= covis // 2).all(1)
    return st, q


def main():
    import torch
    from scavislam_amd import capi
    from scavislam_amd.frontend import FastGrid, FramePyramid, GuidedMatcher, PoseOptimizer
    from scavislam_amd.register import KeyframeRegistrar, keyframe_table

    scene = M.make_scene(cam=CAM, n_per_kf=(300, 150, 50), seed=9)
    n_src, n_kf = len(scene["src"]), len(scene["kf_T"])
    ctx, stream = capi.torch_context(0)
    # every keyframe's pyramid in FramePyramid buffers (the strides the front end uses); 32 separate copies of the root frame for the batch
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
                    T_root_from_world=scene["T_root"], src=scene["src"], obs_begin=scene["obs_begin"], obs_kf=scene["obs_kf"])

    reg = KeyframeRegistrar(ctx, CAM, max_requests=NB, max_points=2048, max_keyframes=8, max_observers=8192)
    reqs = [request(r) for r in roots]

    # ---- the composition from the entry points that were there before the call
    root = frames[0]
    fast = FastGrid(ctx, root)
    matcher = GuidedMatcher(ctx, root, fast)
    po = PoseOptimizer(ctx, root)
    from scavislam_amd.ctypes_types import PoseOptParams
    lc = M.level_cams(CAM)
    cams = {k: np.array([c[k] for c in lc]) for k in ("f", "cx", "cy", "w", "h")}
    kf_entries = [(frames[k].pyr, 0, scene["kf_T"][k]) for k in range(n_kf)]

    def composition():
        idx, in_vt = host_cull(scene, cams)
        if len(idx) < 15:
            return None
        cand = np.ascontiguousarray(scene["src"][idx])
        for l in range(3):
            fast.set_thresholds(0, l, scene["fast_thr"][l])
        fast.detect()
        T = np.eye(3, 4)
        for radius, it in ((10, 25), (4, 15)):
            res = matcher.match(kf_entries, T.reshape(12), scene["T_root"], cand, radius, 22, 10)[0]      # blocking download
            if (res["status"] == 0).sum() < 15:
                return None
            Tb, _ = po.calcFastMotionOnly(matcher, T.reshape(12), PoseOptParams(1, it, 2.0, -1.0, 1e-5, 15, 0))      # blocking download
            T = Tb[0]
        gated, _ = po.processMatchedPoints(matcher, 0)                                                    # blocking download
        acc = gated[0]["accepted"] * (res["status"] == 0)
        st, q = host_count(scene, idx, acc, res["obs"], in_vt, 15)
        return T, st, q

    with torch.cuda.stream(stream):
        one = reg.local_register(reqs[:1])[0]
        many = reg.local_register(reqs)
        base = composition()
        assert one.status == 0 and all(o.status == 0 for o in many) and base is not None
        assert np.array_equal(one.kf_stats["strength"], base[1][:, 0]) and np.array_equal(one.kf_stats["qualifies"] != 0, base[2]), "the two forms disagree"
        assert np.abs(one.T_newroot_from_oldroot - base[0]).max() < 1e-9
        assert all(o.T_newroot_from_oldroot.tobytes() == one.T_newroot_from_oldroot.tobytes() for o in many)
        t_one, t_many, t_base = [], [], []
        for _ in range(ROUNDS):
            t0 = time.perf_counter(); reg.local_register(reqs[:1]); t_one.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); composition(); t_base.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); reg.local_register(reqs); t_many.append(time.perf_counter() - t0)
        reg.set_timing(True)
        s_one, s_many = [], []
        for _ in range(ROUNDS):
            reg.local_register(reqs[:1]); s_one.append(reg.stage_times_ms())
            reg.local_register(reqs); s_many.append(reg.stage_times_ms())
    med = lambda a: float(np.median(a)) * 1e3
    s_one, s_many = np.median(np.array(s_one), 0), np.median(np.array(s_many), 0)
    out = [f"{n_src} source points, {one.n_candidates} candidates, {one.n_obs_pass1} / {one.n_obs_pass2} observations, {one.n_accepted} accepted, "
           f"{one.n_qualified} of {n_kf} keyframes qualify; medians over {ROUNDS} rounds", "",
           "| form | host time per call (ms) | per request (ms) |", "|---|---:|---:|",
           f"| composition of the earlier entry points, 1 request | {med(t_base):.3f} | {med(t_base):.3f} |",
           f"| one call, 1 request | {med(t_one):.3f} | {med(t_one):.3f} |",
           f"| one call, {NB} requests | {med(t_many):.3f} | {med(t_many) / NB:.3f} |", "",
           "| device time per stage (ms) | cull | FAST | match 1 | refinement 1 | match 2 | refinement 2 | gate | sum |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|",
           "| 1 request | " + " | ".join(f"{v:.4f}" for v in s_one) + f" | {s_one.sum():.4f} |",
           f"| {NB} requests | " + " | ".join(f"{v:.4f}" for v in s_many) + f" | {s_many.sum():.4f} |"]
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    print("one call not slower than the composition for one request:", med(t_one) <= med(t_base))
    reg.close(); fast.close(); ctx.close()


if __name__ == "__main__":
    main()
