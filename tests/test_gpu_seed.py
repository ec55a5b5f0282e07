"""New-point seeding on the device (svs_seed_points, svs_frontend_seed_keyframes: StereoFrontend::addNewPoints / addMorePoints, stereo_frontend.cpp:682-823)
against the NumPy restatement tests/seed_model.py, which tests/test_seed_cpu.py holds against the reference.

Bounds.  Every decision of the procedure is an integer predicate or `d > 0` on one exact product of a float with a power of two, so counts, order, integer
fields and anchor_obs_pyr = (x, y, x - d) (one f64 subtraction) must be IDENTICAL.  xyz_anchor is fewer than ten f64 roundings of 1.1e-16 each on terms bounded
by |xyz|: 1e-12 max(1, |xyz|).  The library is compiled without contraction and evaluates the model's expression tree, so it is expected to be equal; the test
prints whether it is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seed_common as S
import seed_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def assert_records(got, n_new, rec, n_ref, what):
    from_model = np.hstack([rec["xyz_anchor"], rec["anchor_obs_pyr"]])
    assert np.array_equal(n_new, n_ref), f"{what}: counts {n_new} vs the model's {n_ref}"
    assert len(got) == len(rec["point_id"])
    for k in ("anchor_level", "kf_index", "point_id"):
        assert np.array_equal(got[k], rec[k]), f"{what}: {k}"
    assert (got["pad_"] == 0).all()
    assert np.array_equal(got["anchor_obs_pyr"].view(np.uint64), rec["anchor_obs_pyr"].view(np.uint64)), f"{what}: anchor_obs_pyr"
    if len(got):
        err = np.abs(got["xyz_anchor"] - rec["xyz_anchor"]).max(1)
        bound = 1e-12 * np.maximum(1.0, np.linalg.norm(rec["xyz_anchor"], axis=1))
        print(f"{what}: {len(got)} records, xyz_anchor", "EQUAL to the model's" if np.array_equal(got["xyz_anchor"], rec["xyz_anchor"]) else f"max err {err.max():.3e}")
        assert (err <= bound).all(), f"{what}: xyz_anchor off by {err.max()}"
    return from_model


def run_seed_points(gpu_ctx, probs, R, nmp, use_order, cap=None, prefill=None, expect_error=False):
    """one svs_seed_points call over a batch of hand-made problems (same level-0 size); returns [(records, counts)] and the raw output block.
    expect_error: the call must raise SvsError; returns (the error, the output block and the counts as the device holds them behind the refused call)"""
    from scavislam_amd.capi import SvsError
    import torch
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, SEED_PROBLEM_DTYPE, Cam, SeedArgs, SeedParams
    ctx, stream = gpu_ctx
    B = len(probs)
    cam = probs[0]["cam"]
    W, H = cam["w"], cam["h"]
    prm = SeedParams.reference(clearance=R, num_max_points=nmp)
    cap = prm.max_records() if cap is None else cap
    dstride = W + 3      # a padded row stride
    disp = np.full((B, H, dstride), np.nan, np.float32)
    prob = np.zeros(B, SEED_PROBLEM_DTYPE)
    tmax = max(1, max(len(p["tree_level"]) for p in probs))
    tree_xy, tree_level = np.zeros((B, tmax, 2)), np.full((B, tmax), -1, np.int32)
    host = dict(xy=[], n=[], cells=[], order=[])
    for l in range(3):
        capl = max(1, max(len(p["corners"][l]) for p in probs))
        xy = np.full((B, capl, 2), -7, np.int16)
        order = np.full((B, capl), -1, np.int32)
        for b, p in enumerate(probs):
            xy[b, :len(p["corners"][l])] = p["corners"][l]
            order[b, :len(p["orders"][l])] = p["orders"][l]
        host["xy"].append(xy); host["order"].append(order)
        host["n"].append(np.array([len(p["corners"][l]) for p in probs], np.int32))
        host["cells"].append(np.stack([p["cells"][l] for p in probs]).astype(np.int32))
    for b, p in enumerate(probs):
        disp[b, :, :W] = p["disp"]
        q = prob[b]
        q["T_newkey_from_cur"] = np.asarray(p["T"]).reshape(12); q["seed"] = p["seed"] & 0xFFFFFFFFFFFFFFFF; q["add_flags"] = p["flags"]; q["n0"] = p["n0"]
        q["n_tree"] = len(p["tree_level"]); q["kf_index"] = p["kf_index"]; q["first_point_id"] = p["first_point_id"]; q["use_order"] = int(use_order)
        q["n_order"] = [len(o) for o in p["orders"]]
        tree_xy[b, :len(p["tree_level"])] = p["tree_xy"]; tree_level[b, :len(p["tree_level"])] = p["tree_level"]
    with torch.cuda.stream(stream):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        d = dict(disp=dev(disp), prob=dev(prob), tree_xy=dev(tree_xy), tree_level=dev(tree_level), xy=[dev(a) for a in host["xy"]], n=[dev(a) for a in host["n"]],
                 cells=[dev(a) for a in host["cells"]], order=[dev(a) for a in host["order"]])
        out_h = np.zeros((B, max(cap, 1)), CANDIDATE_DTYPE)
        if prefill is not None:
            out_h.view(np.uint8)[...] = prefill
        out = dev(out_h)
        cnt = dev(np.full((B, 3), -5, np.int32))
    a = SeedArgs()
    for l in range(3):
        a.d_xy[l] = d["xy"][l].data_ptr(); a.xy_bstride[l] = host["xy"][l].shape[1] * 2; a.xy_cap[l] = host["xy"][l].shape[1]
        a.d_n[l] = d["n"][l].data_ptr(); a.n_bstride[l] = 1
        a.d_cell_count[l] = d["cells"][l].data_ptr(); a.cell_bstride[l] = 4; a.n_cells[l] = 4
        a.d_order[l] = d["order"][l].data_ptr(); a.order_bstride[l] = host["order"][l].shape[1]
    a.d_disp, a.disp_stride, a.disp_bstride = d["disp"].data_ptr(), dstride, H * dstride
    a.cam = Cam(cam["f"], cam["cx"], cam["cy"], cam["b"], W, H)
    a.d_prob, a.d_tree_xy, a.d_tree_level, a.tree_bstride, a.batch = d["prob"].data_ptr(), d["tree_xy"].data_ptr(), d["tree_level"].data_ptr(), tmax, B
    err = None
    try:
        ctx.call("svs_seed_points", C.byref(a), C.byref(prm), out.data_ptr(), cap, cnt.data_ptr())
    except SvsError as e:
        err = e
    assert (err is not None) == expect_error, err
    ctx.sync()
    out_h = out.cpu().numpy().view(CANDIDATE_DTYPE).reshape(B, max(cap, 1))
    cnt_h = cnt.cpu().numpy().view(np.int32).reshape(B, 3)
    if expect_error:
        return err, out_h, cnt_h
    return [(out_h[b, :int(cnt_h[b].sum())].copy(), cnt_h[b].copy()) for b in range(B)], out_h


def model_of(p, R, nmp, use_order):
    orders = p["orders"] if use_order else [M.generated_order(p["seed"], l, p["cells"][l]) for l in range(3)]
    return M.seed_points(p["corners"], orders, p["disp"], p["cam"], p["tree_xy"], p["tree_level"], p["flags"], p["n0"], T=p["T"], kf_index=p["kf_index"],
                         first_point_id=p["first_point_id"], clearance=R, num_max_points=nmp)


@pytest.mark.parametrize("use_order", [True, False], ids=["callers_order", "generated_order"])
@pytest.mark.parametrize("W,H,R,nmp", [(80, 48, 2, 12), (80, 48, 0, 12), (96, 64, 2, 12), (96, 64, 0, 12), (80, 48, 2, 300)])
def test_seed_points_against_model(gpu_ctx, W, H, R, nmp, use_order):
    probs = [S.handmade_problem(W, H, 7, R, v) for v in range(3)]
    batch, _ = run_seed_points(gpu_ctx, probs, R, nmp, use_order)
    reasons, visited0 = set(), []
    for b, p in enumerate(probs):
        rec, n_ref, trace = model_of(p, R, nmp, use_order)
        assert_records(batch[b][0], batch[b][1], rec, n_ref, f"{W}x{H} R={R} problem {b}")
        reasons |= {why for t in trace for _, why in t}
        visited0.append((len(trace[0]), len(p["corners"][0])))
        alone, _ = run_seed_points(gpu_ctx, [p], R, nmp, use_order)      # batch invariance: the same bytes alone
        assert alone[0][0].tobytes() == batch[b][0].tobytes() and np.array_equal(alone[0][1], batch[b][1])
    # the cases the problems were made for did occur
    assert reasons == {"disp", "border", "flag", "window", "taken"}, reasons
    assert len(probs[0]["corners"][0]) == 150 and len(probs[0]["corners"][2]) == 0
    assert any(v == n and n > 128 for v, n in visited0), visited0                                   # a level walked through three chunks, the last one ragged
    if nmp == 12:
        assert any(v < n and v % 64 != 0 for v, n in visited0), visited0                            # the cap fell inside a chunk


def test_capacity_one_too_small_writes_nothing(gpu_ctx):
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import SeedParams
    probs = [S.handmade_problem(80, 48, 7, 2, 0)]
    need = SeedParams.reference(num_max_points=12).max_records()
    assert need == 13 + 7 + 4
    err, raw, cnt = run_seed_points(gpu_ctx, probs, 2, 12, True, cap=need - 1, prefill=0xAB, expect_error=True)
    assert isinstance(err, SvsError) and "status 4" in str(err), err
    assert (raw.view(np.uint8) == 0xAB).all() and (cnt == -5).all(), "the refused call wrote to its outputs"
    res, raw = run_seed_points(gpu_ctx, probs, 2, 12, True, cap=need, prefill=0xAB)      # the context is usable, and only the records are written
    m = int(res[0][1].sum())
    assert m > 0 and (raw.view(np.uint8).reshape(-1)[m * 64:] == 0xAB).all()


# ---- the front end's own state --------------------------------------------------------------------------------------------------------------------------------
def frontend_after_first_frames(gpu_ctx, camname, B=2):
    """a B-stream front end behind processFirstFrames on frame 0 of the sequence (rendered here: nothing of the fixture is needed, so nothing can skip)"""
    import torch
    import seq_common
    from scavislam_amd.frontend import StereoFrontend
    ctx, stream = gpu_ctx
    cam = seq_common.cam_of(camname)
    img, disp0 = S.frame(camname, 0)
    fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2, n_streams=B)
    with torch.cuda.stream(stream):
        left = torch.as_tensor(np.stack([img] * B)).cuda()
        disp = torch.as_tensor(np.stack([disp0] * B).astype(np.float32)).cuda()
    fe.processFirstFrames(left=left, disp=disp)
    return fe, cam, (left, disp)


@pytest.mark.parametrize("camname", ["default", "newcollege"])
def test_frontend_first_keyframe_equals_the_fixture(gpu_ctx, camname):
    """processFirstFrames on frame 0 of the sequence, SVS_SEED_FIRST in the order that retraces the reference: its first keyframe's points (528: 301 / 151 / 76)"""
    from scavislam_amd.ctypes_types import SEED_FIRST
    case = S.keyframe_case(camname, 0)
    if case["why"] == "crc":
        pytest.skip("the rendered frame is not the fixture's (crc)")
    assert case["ok"], f"the oracle's FAST detection does not reproduce the fixture's thresholds on frame 0 ({case['why']})"
    fe, cam, keep = frontend_after_first_frames(gpu_ctx, camname)
    for l in range(3):
        assert np.array_equal(fe.corners(1, l)[0], case["corners"][l])
    fid = case["first_point_id"]
    out = fe.seedKeyframes([dict(stream=0, mode=SEED_FIRST, kf_index=0, first_point_id=fid, order=case["orders"]),
                            dict(stream=1, mode=SEED_FIRST, kf_index=1, first_point_id=fid, seed=77),
                            dict(stream=1, mode=SEED_FIRST, kf_index=0, first_point_id=fid, order=case["orders"])])
    for r in (0, 2):
        rec, cnt = out[r]
        assert cnt.tolist() == [301, 151, 76]
        S.assert_equals_reference(rec, case, f"{camname} request {r}")
    assert out[0][0].tobytes() == out[2][0].tobytes()
    # the generated order beside it in the same call, against the model
    orders = [M.generated_order(77, l, case["cells"][l]) for l in range(3)]
    ref, n_ref, _ = M.seed_points(case["corners"], orders, case["disp"], case["cam"], np.zeros((0, 2)), np.zeros(0, np.int32), np.ones(9, np.int32), np.zeros(3, np.int32),
                                  kf_index=1, first_point_id=fid)
    assert_records(out[1][0], out[1][1], ref, n_ref, f"{camname} generated")
    fe.close()


@pytest.mark.parametrize("camname", ["default", "newcollege"])
def test_frontend_seed_more_after_a_step(gpu_ctx, camname):
    """one processFrames step on every third point seeded from frame 0, then SVS_SEED_MORE (generated order) = the model on the downloaded corners, disparity,
    gate records and statistics.  Every third point: 176 candidates leave at least one 3 x 3 cell with <= 25 matched points (176 / 9 < 25), so at least one cell
    asks for points and the clearance test runs; with all 528 tracked every cell is full and SVS_SEED_MORE rightly adds nothing"""
    import torch
    from scavislam_amd import synth
    from scavislam_amd.ctypes_types import MATCH_OK, SEED_FIRST, SEED_MORE
    import seq_common
    ctx, stream = gpu_ctx
    fe, cam, keep = frontend_after_first_frames(gpu_ctx, camname)
    B = 2
    traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)
    first = fe.seedKeyframes([dict(stream=b, mode=SEED_FIRST, kf_index=0, first_point_id=1, seed=5 + b) for b in range(B)])
    fe.keepKeyframes(0, np.stack([traj[0].reshape(12)] * B))
    cand = [first[b][0][::3].copy() for b in range(B)]
    fe.setCandidateListsAll(cand, [[len(c), len(c)] for c in cand])
    img, disp = S.frame(camname, 1)
    with torch.cuda.stream(stream):
        left = torch.as_tensor(np.stack([img] * B)).cuda()
        dd = torch.as_tensor(np.stack([disp] * B).astype(np.float32)).cuda()
    fe.processFrames(np.stack([I34.reshape(12)] * B), np.stack([traj[0].reshape(12)] * B), left=left, disp=dd)
    T = np.hstack([np.array([[0.999, -0.04, 0.0], [0.04, 0.999, 0.01], [0.0, -0.01, 1.0]]), [[0.1], [-0.2], [0.05]]])
    out = fe.seedKeyframes([dict(stream=b, mode=SEED_MORE, kf_index=1, first_point_id=4000 + b, seed=900 + b, T_newkey_from_cur=T) for b in range(B)])
    for b in range(B):
        res, m, g = fe.results(b)
        pts = cand[b]
        ok =(m["status"] == MATCH_OK) & (g["accepted"] != 0)
        assert ok.sum() > 100, "the step tracked too little for this test to mean anything"
        st = res.point_stats
        n0 = np.array(list(st.num_matched_points), np.int32)
        flags = M.flags_from_grid3x3(np.array(list(st.num_points_grid3x3)))
        assert n0.sum() == ok.sum()
        corners, cells = [], []
        for l in range(3):
            xy, cc, _, _ = fe.corners(b, l)
            corners.append(xy); cells.append(cc[:(9, 9, 4)[l]])
        orders = [M.generated_order(900 + b, l, cells[l]) for l in range(3)]
        ref, n_ref, trace = M.seed_points(corners, orders, disp, cam, g["uv_pyr"][ok], pts["anchor_level"][ok], flags, n0, T=T, kf_index=1,
                                          first_point_id=4000 + b)
        assert {why for t in trace for _, why in t} >= {"window", "taken"}
        assert_records(out[b][0], out[b][1], ref, n_ref, f"{camname} stream {b}")
    fe.close()


def test_seed_more_needs_the_records_of_a_step(gpu_ctx):
    """SVS_SEED_MORE reads the last step's gate records and point statistics: refused behind a first frame, and behind a step once the candidate list was replaced"""
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import SEED_FIRST, SEED_MORE
    fe, cam, keep = frontend_after_first_frames(gpu_ctx, "default", B=1)
    more = [dict(stream=0, mode=SEED_MORE, kf_index=1, first_point_id=1, seed=3)]
    with pytest.raises(SvsError, match="status 1"):
        fe.seedKeyframes(more)
    first = fe.seedKeyframes([dict(stream=0, mode=SEED_FIRST, kf_index=0, first_point_id=1, seed=3)])[0][0]      # the front end is still usable
    assert len(first) == 528
    T0 = I34.reshape(1, 12)
    fe.keepKeyframes(0, T0)
    fe.setCandidateListsAll([first[::3].copy()], [[176, 176]])
    fe.processFrames(T0, T0, left=keep[0], disp=keep[1])
    assert fe.seedKeyframes(more)[0][1].sum() >= 0
    fe.setCandidateListsAll([first[::4].copy()], [[132, 132]])
    with pytest.raises(SvsError, match="status 1"):
        fe.seedKeyframes(more)
    fe.close()


def test_frontend_many_requests_equal_one_at_a_time(gpu_ctx):
    """40 requests on 2 streams: more than 1 MiB of output rows (40 x 531 x 64 B), so the records come home as the counts plus one strided copy of the longest
    list's width.  Every request's counts and records are those of the same request issued alone (the one-copy path); lists of different lengths are in the call"""
    from scavislam_amd.ctypes_types import SEED_FIRST, SeedParams
    fe, cam, keep = frontend_after_first_frames(gpu_ctx, "default")
    few = [np.arange(5 + r, dtype=np.int32) * 7 for r in range(3)]      # a caller's order over a few corners: a short list among the long ones
    T = np.hstack([np.array([[0.999, -0.04, 0.0], [0.04, 0.999, 0.01], [0.0, -0.01, 1.0]]), [[0.1], [-0.2], [0.05]]])
    reqs = [dict(stream=r % 2, mode=SEED_FIRST, kf_index=r % 2, first_point_id=100 * r, seed=31 + r, T_newkey_from_cur=T if r % 3 else None) for r in range(40)]
    reqs = [{k: v for k, v in q.items() if v is not None} for q in reqs]
    reqs[7]["order"] = few
    reqs[39]["order"] = few[::-1]
    assert 40 * SeedParams.reference().max_records() * 64 > 1 << 20
    together = fe.seedKeyframes(reqs)
    lengths = set()
    for r, q in enumerate(reqs):
        alone = fe.seedKeyframes([q])[0]
        assert np.array_equal(together[r][1], alone[1]), f"request {r}: counts"
        assert together[r][0].tobytes() == alone[0].tobytes(), f"request {r}: records"
        lengths.add(len(alone[0]))
    assert max(lengths) == 528 and min(lengths) < 30, lengths
    fe.close()


def test_cpp_adaptor_produces_the_c_calls_records(gpu_ctx, tmp_path):
    """tests/cpp/seed_smoke.cpp: StereoFrontend::addNewPoints / addMorePoints of include/scavislam_hip.hpp against svs_frontend_seed_keyframes called directly"""
    exe = tmp_path / "seed_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "seed_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("SEED ")]
    assert tok and tok[0].split()[1] == "ok", out
    first, more = int(tok[0].split()[2]), int(tok[0].split()[3])
    assert first > 100 and more > 0
