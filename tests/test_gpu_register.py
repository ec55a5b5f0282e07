"""GPU parity of the back end's re-registration in one call (svs_reg_register_batch: Backend::localRegisterFrame / globalLoopClosure, backend.cpp:549-611,
830-1001) against tests/register_model.py -- stage by stage, each stage of the model fed the device's own previous output so that a last-bit pose difference
cannot cascade, then end to end on a scene whose strengths are far from covis_thr."""
import os
import subprocess

import numpy as np
import pytest

import register_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = M.SMALL_CAM


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model_run(scene):
    return M.register(scene, CAM)


@pytest.fixture(scope="module")
def device_scene(gpu_ctx, scene):
    """the scene's pyramids and the root's disparity in device memory (one tensor each: the frames of two requests lie at no common stride)"""
    import torch
    ctx, stream = gpu_ctx
    with torch.cuda.stream(stream):
        pyrs = [[torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in pyr] for pyr in scene["kf_pyrs"]]
        disp = torch.as_tensor(np.ascontiguousarray(scene["root_disp"], np.float32)).cuda()
        disp_copy = disp.clone()
        root_copy = [t.clone() for t in pyrs[0]]
    ctx.sync()
    return dict(pyrs=pyrs, disp=disp, disp_copy=disp_copy, root_copy=root_copy)


@pytest.fixture(scope="module")
def registrar(gpu_ctx):
    from scavislam_amd.register import KeyframeRegistrar
    reg = KeyframeRegistrar(gpu_ctx[0], CAM, max_requests=8, max_points=512, max_keyframes=8, max_observers=4096)
    yield reg
    reg.close()


def _dev_request(dev, req, copy=False):
    """the model's request as KeyframeRegistrar takes it; copy: the root frame in a second set of buffers (another address, the same bytes)"""
    from scavislam_amd.register import keyframe_table
    entries = []
    for k, pyr in enumerate(dev["pyrs"]):
        p = dev["root_copy"] if (copy and k == req["root_kf"]) else pyr
        entries.append(([t.data_ptr() for t in p], [t.shape[1] for t in p], req["kf_T"][k]))
    disp = dev["disp_copy"] if copy else dev["disp"]
    return dict(kfs=keyframe_table(entries), flags=req["flags"], root_kf=req["root_kf"], root_disp=(disp.data_ptr(), disp.shape[1]), fast_thr=req["fast_thr"],
                T_root_from_world=req["T_root"], src=req["src"], obs_begin=req["obs_begin"], obs_kf=req["obs_kf"])


def _run(registrar, dev, reqs, **kw):
    return registrar.register_batch([_dev_request(dev, r, copy=bool(i & 1)) for i, r in enumerate(reqs)], [r["mode"] for r in reqs], **kw)


def _same_records(a, b, what):
    """two MATCH_RESULT_DTYPE arrays, byte for byte"""
    assert len(a) == len(b), what
    bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
    assert not bad, (what, bad[:5], a[bad[:5]], b[bad[:5]])


# ---- the cull ------------------------------------------------------------------------------------------------------------------------------------------------
def _cull_request(scene, n_src, seed, all_out=False):
    """n_src points: entry 1 (identity pose, like the root) anchors points whose projections sit 1e-4 px either side of the frame's borders and at -0.5 / w - 0.5,
    entry 3 (a real pose) random points around the frame, entry 2 is outside the double window, one point lies behind the camera"""
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    rng = np.random.default_rng(seed)
    cams = M.level_cams(CAM)
    kf_T = np.array([M.I12, M.I12, M.I12, scene["kf_T"][2], M.I12])
    flags = np.array([3, 1, 0, 1, 1], np.uint8)
    src = np.zeros(n_src, CANDIDATE_DTYPE)
    e = 1e-4
    for i in range(n_src):
        lvl = int(rng.integers(0, 3))
        c = cams[lvl]
        kind = i % 8 if n_src > 1 else 8
        z = float(rng.uniform(2.0, 9.0))
        if all_out:
            u, v, kf = c["w"] + float(rng.uniform(1.5, 50.0)), float(rng.uniform(-40.0, -1.5)), 1
        elif kind == 0:      # a border of u
            u, v, kf = float(rng.choice([-1.0 - e, -1.0 + e, -0.5, -e, e, c["w"] - 1 - e, c["w"] - 1 + e, c["w"] - 0.5, c["w"] - e, c["w"] + e])), 0.5 * c["h"] + 0.37, 1
        elif kind == 1:      # a border of v
            u, v, kf = 0.5 * c["w"] + 0.37, float(rng.choice([-1.0 - e, -1.0 + e, -0.5, -e, e, c["h"] - 1 - e, c["h"] - 1 + e, c["h"] - 0.5, c["h"] - e, c["h"] + e])), 1
        elif kind == 8:      # a lone point on both truncating borders: kept
            u, v, kf = -0.5, c["h"] - 0.5, 1
        elif kind == 2:      # anchor outside the double window, projection inside
            u, v, kf = 0.3 * c["w"] + 0.37, 0.3 * c["h"] + 0.37, 2
        elif kind == 3:      # behind the camera, projecting into the frame: kept
            u, v, kf, z = 0.4 * c["w"] + 0.37, 0.6 * c["h"] + 0.37, 4, -z
        else:
            u, v, kf = float(rng.uniform(-0.3, 1.3)) * c["w"], float(rng.uniform(-0.3, 1.3)) * c["h"], int(rng.choice([1, 3, 4]))
        src[i]["xyz_anchor"] = [(u - c["cx"]) / c["f"] * z, (v - c["cy"]) / c["f"] * z, z]
        src[i]["anchor_obs_pyr"] = [0.5 * c["w"], 0.5 * c["h"], 0.5 * c["w"] - 2.0]
        src[i]["anchor_level"], src[i]["kf_index"], src[i]["point_id"] = lvl, kf, 5000 + i
    req = dict(scene, mode=M.LOCAL, T_root=np.array(M.I12), kf_T=kf_T, flags=flags, src=src, obs_begin=np.zeros(n_src + 1, np.int32), obs_kf=np.zeros(0, np.int32))
    # no projection closer than 1e-6 px to an integer: the contraction of a multiply-add cannot decide a point
    for p in src:
        kf = int(p["kf_index"])
        u, v = M.project(req["T_root"], kf_T[kf], p["xyz_anchor"], cams[int(p["anchor_level"])])
        assert abs(u - round(u)) >= 1e-6 and abs(v - round(v)) >= 1e-6, (u, v)
    return req


def test_candidate_lists_equal_the_model_in_content_and_order(registrar, device_scene, scene):
    sizes = [1, 63, 64, 65, 257]
    reqs = [_cull_request(scene, n, 100 + n) for n in sizes] + [_cull_request(scene, 40, 7, all_out=True)]
    outs = _run(registrar, device_scene, reqs)
    kept_total = 0
    for req, out in zip(reqs, outs):
        keep, in_vt = M.cull(req, CAM)
        assert out.n_candidates == len(keep) and np.array_equal(out.cand_src, keep), (len(req["src"]), out.cand_src, keep)
        assert np.array_equal(out.kf_stats["in_vertex_table"], in_vt)
        kept_total += len(keep)
        if len(keep) < 15:
            assert out.status == M.FEW_CANDIDATES and out.n_obs_pass1 == 0 and out.n_obs_pass2 == 0 and out.n_accepted == 0
            assert np.array_equal(out.T_newroot_from_oldroot, np.eye(3, 4))
    assert outs[-1].n_candidates == 0 and outs[0].n_candidates == 1
    keep257 = M.cull(reqs[4], CAM)[0]
    assert 40 < len(keep257) < 257 and kept_total > 100
    behind = np.nonzero(reqs[4]["src"]["xyz_anchor"][:, 2] < 0)[0]
    assert len(behind) > 5 and set(behind) <= set(keep257)                  # no depth test in the cull
    assert not set(np.nonzero(reqs[4]["src"]["kf_index"] == 2)[0]) & set(keep257)


# ---- stage by stage ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def both_modes(registrar, device_scene, scene):
    reqs = [dict(scene, mode=M.LOCAL), dict(scene, mode=M.LOOP)]
    return reqs, _run(registrar, device_scene, reqs, want_pass1=True)


def test_match_records_of_both_passes_equal_the_oracle(both_modes, scene):
    """svs_match at radius 10 (one wave per point: the window is wider than 17) from the identity and at radius 4 from the device's own pose"""
    reqs, outs = both_modes
    trees = M.root_trees(scene)
    for req, out in zip(reqs, outs):
        keep, _ = M.cull(req, CAM)
        assert np.array_equal(out.cand_src, keep) and len(keep) > 200
        cand = np.ascontiguousarray(req["src"][out.cand_src])
        m1 = M.match(req, CAM, cand, M.I12, 10, trees)
        _same_records(out.matches_pass1, m1, "pass 1")
        assert np.array_equal(out.status_pass1, m1["status"]) and out.n_obs_pass1 == int((m1["status"] == 0).sum()) > 100
        m2 = M.match(req, CAM, cand, out.T_pass1, 4, trees)
        _same_records(out.matches, m2, "pass 2")
        assert out.n_obs_pass2 == int((m2["status"] == 0).sum()) > 100


def test_poses_and_statistics_equal_the_oracle(both_modes, scene):
    """the bars tests/test_gpu_motion.py holds svs_motion_only to: pose atol 1e-9, chi2 rtol 1e-9"""
    import oracle as O
    from scavislam_amd import synth
    reqs, outs = both_modes
    for out in outs:
        for res, T0, it, T, st in ((out.matches_pass1, np.eye(3, 4), 25, out.T_pass1, out.stats_pass1), (out.matches, out.T_pass1, 15, out.T_newroot_from_oldroot, out.stats_pass2)):
            Tr, sr = O.motion_only(res, M.cam_c(CAM), T0, M.pose_params(it))
            print("pose diff", np.abs(T - Tr).max(), "chi2", st.chi2, sr.chi2)
            assert st.status == 0 and st.num_obs == sr.num_obs
            np.testing.assert_allclose(T, Tr, rtol=0, atol=1e-9)
            np.testing.assert_allclose([st.initial_chi2, st.chi2, st.max_err], [sr.initial_chi2, sr.chi2, sr.max_err], rtol=1e-9)
        dT = scene["T_true_from_stored"]      # the root image was rendered this far off the stored pose
        assert np.abs(out.T_newroot_from_oldroot - synth.pose(synth.so3_exp(dT[0]), dT[1])).max() < 0.02


def test_gate_counters_and_status_equal_the_model(both_modes):
    reqs, outs = both_modes
    for req, out in zip(reqs, outs):
        cand = np.ascontiguousarray(req["src"][out.cand_src])
        acc = M.gate(out.matches, cand, CAM, out.T_newroot_from_oldroot)
        assert np.array_equal(out.accepted, acc) and out.n_accepted == int(acc.sum()) > 100
        in_vt = M.cull(req, CAM)[1]
        st = M.count(req, CAM, out.cand_src, acc, out.matches["obs"], in_vt, 15)
        got = np.stack([out.kf_stats[k] for k in ("strength", "n_u_hi", "n_u_lo", "n_v_hi", "n_v_lo", "qualifies", "in_vertex_table")], 1)
        assert np.array_equal(got, st), (got, st)
        assert out.n_qualified == int(st[:, 5].sum())
        assert out.status == M.decide(req["mode"], out.n_candidates, out.n_obs_pass1, out.n_obs_pass2, out.n_qualified, 15) == M.OK
    assert outs[0].neighborid_to_strength().keys() == {2, 3} and outs[1].neighborid_to_strength().keys() == {0}
    ids, uvu, lvl = outs[0].track_points(reqs[0]["src"])
    assert len(ids) == outs[0].n_accepted and set(ids) <= set(reqs[0]["src"]["point_id"])


def test_end_to_end_equals_the_model_run_on_its_own(both_modes, model_run, scene):
    """strengths at least 5 away from covis_thr (checked on the CPU): the decision, the qualifying set and the pose of the model's own chain"""
    reqs, outs = both_modes
    for req, out in zip(reqs, outs):
        mo = model_run if req["mode"] == M.LOCAL else M.register(req, CAM)
        st = mo["kf_stats"]
        assert np.all(np.abs(st[:, 0] - 15) >= 5) and np.all(np.abs(st[st[:, 0] > 0][:, 1:5] - 7) >= 5)
        assert out.status == mo["status"] == M.OK
        assert np.array_equal(out.kf_stats["qualifies"], st[:, 5])
        np.testing.assert_allclose(out.T_newroot_from_oldroot, mo["T"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(out.T_pass1, mo["T1"], rtol=0, atol=1e-9)


# ---- batches -------------------------------------------------------------------------------------------------------------------------------------------------
def _exit3_request(scene, model_run):
    """16 candidates of the scene of which the first match finds at least 15 and the second fewer (chosen with the model: points the radius-4 match loses)"""
    ok1, ok2 = model_run["m1"]["status"] == 0, model_run["m2"]["status"] == 0
    both, only1 = np.nonzero(ok1 & ok2)[0], np.nonzero(ok1 & ~ok2)[0]
    rng = np.random.default_rng(0)
    for _ in range(200):
        n1 = int(rng.integers(3, min(8, len(only1)) + 1))
        sel = np.sort(np.concatenate([rng.choice(both, 16 - n1, replace=False), rng.choice(only1, n1, replace=False)]))
        idx = model_run["cand_src"][sel]
        req = dict(scene, mode=M.LOOP, src=scene["src"][idx], obs_begin=np.zeros(len(idx) + 1, np.int32), obs_kf=np.zeros(0, np.int32))
        mo = M.register(req, CAM)
        if mo["status"] == M.FEW_MATCHES_PASS2 and mo["n_obs_pass2"] <= 13:
            return req
    raise AssertionError("no subset of the scene leaves at the third exit")


def _mixed(scene, model_run):
    few = scene["src"][model_run["cand_src"][:10]]
    empty_rows = dict(obs_begin=np.zeros(11, np.int32), obs_kf=np.zeros(0, np.int32))
    return [dict(scene, mode=M.LOCAL, src=few, **empty_rows),                                                       # exit 1: 10 candidates
            dict(scene, mode=M.LOOP, src=few, **empty_rows),                                                        # exit 2: at most 10 observations
            _exit3_request(scene, model_run),                                                                      # exit 3
            dict(scene, mode=M.LOCAL, obs_begin=np.zeros(len(scene["src"]) + 1, np.int32), obs_kf=np.zeros(0, np.int32)),      # exit 4: nobody observes the points
            dict(scene, mode=M.LOCAL)]                                                                              # a registration


def _raw_of(registrar, i):
    raw = registrar.raw
    sz = len(raw["results"]) // max(len(raw["cand_src"]), 1)
    return (raw["results"][i * sz:(i + 1) * sz], raw["cand_src"][i].tobytes(), raw["matches"][i].tobytes(), raw["status_pass1"][i].tobytes(),
            raw["accepted"][i].tobytes(), raw["kf_stats"][i].tobytes(), raw["matches_pass1"][i].tobytes())


def test_mixed_batch_equals_the_single_runs_byte_for_byte(registrar, device_scene, scene, model_run):
    reqs = _mixed(scene, model_run)
    outs = _run(registrar, device_scene, reqs, want_pass1=True)
    together = [_raw_of(registrar, i) for i in range(len(reqs))]
    assert [o.status for o in outs] == [1, 2, 3, 4, 0]
    assert outs[1].n_obs_pass1 <= 10 and outs[2].n_obs_pass1 >= 15 > outs[2].n_obs_pass2 and outs[3].n_accepted > 100 and outs[3].n_qualified == 0
    for o in outs[:3]:
        assert o.n_accepted == 0 and not o.accepted.any() and not o.kf_stats["strength"].any()
    assert np.array_equal(outs[2].T_newroot_from_oldroot, outs[2].T_pass1)      # the pose stays where the reference returned
    for i, q in enumerate(reqs):
        for copy in (False, True):      # alone, from either set of root buffers; in another slot next to another neighbour
            registrar.register_batch([_dev_request(device_scene, q, copy=copy)], [q["mode"]], want_pass1=True)
            assert _raw_of(registrar, 0) == together[i], (i, copy)
    _run(registrar, device_scene, [reqs[4], reqs[i % 5], reqs[2]], want_pass1=True)
    assert _raw_of(registrar, 0) == together[4] and _raw_of(registrar, 2) == together[2]


def test_the_same_batch_twice_is_bit_identical(registrar, device_scene, scene, model_run):
    reqs = _mixed(scene, model_run)
    runs = []
    for _ in range(2):
        _run(registrar, device_scene, reqs, want_pass1=True)
        runs.append([_raw_of(registrar, i) for i in range(len(reqs))])
    assert runs[0] == runs[1]
    # four requests on one root frame (one stride between them: read in place)
    same = [_dev_request(device_scene, dict(scene, mode=m)) for m in (M.LOCAL, M.LOOP, M.LOCAL, M.LOOP)]
    registrar.register_batch(same, [M.LOCAL, M.LOOP, M.LOCAL, M.LOOP], want_pass1=True)
    assert _raw_of(registrar, 0) == _raw_of(registrar, 2) == runs[0][4] and _raw_of(registrar, 1) == _raw_of(registrar, 3)


def test_error_handling(gpu_ctx, registrar, device_scene, scene):
    from scavislam_amd.capi import SvsError
    from scavislam_amd.register import KeyframeRegistrar
    assert registrar.register_batch([], []) == []                          # n_requests = 0: SVS_OK
    q = _dev_request(device_scene, dict(scene, mode=M.LOCAL))
    small = KeyframeRegistrar(gpu_ctx[0], CAM, max_requests=1, max_points=64, max_keyframes=4, max_observers=16)
    try:
        for bad in ([q, q], [q]):                                          # too many requests; too many points, keyframes and observers
            with pytest.raises(SvsError, match="status 4"):
                small.register_batch(bad, [M.LOCAL] * len(bad))
    finally:
        small.close()
    with pytest.raises(SvsError, match="status 1"):
        registrar.register_batch([dict(q, root_kf=9)], [M.LOCAL])
    with pytest.raises(SvsError, match="status 1"):
        registrar.register_batch([dict(q, fast_thr=[np.full(9, 3), np.full(9, 25), np.full(4, 25)])], [M.LOCAL])
    assert registrar.register_batch([q], [M.LOCAL])[0].status == M.OK      # the handle is as good as before


def test_stage_times_are_reported(registrar, device_scene, scene):
    registrar.set_timing(True)
    try:
        _run(registrar, device_scene, [dict(scene, mode=M.LOCAL)])
        ms = registrar.stage_times_ms()
    finally:
        registrar.set_timing(False)
    assert len(ms) == 7 and all(0.0 < v < 100.0 for v in ms), ms


def test_cpp_adaptor_agrees_with_the_c_call(gpu_ctx, tmp_path):
    """tests/cpp/register_smoke.cpp: BackendRegistration::localRegisterFrame / globalLoopClosure of include/scavislam_hip.hpp against svs_reg_register_batch called directly"""
    exe = tmp_path / "register_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "register_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("REGISTER ")]
    assert tok and tok[0].split()[1] == "ok", out
    assert int(tok[0].split()[2]) >= 15 and int(tok[0].split()[3]) >= 15      # strength of the local neighbour, track points of the loop
