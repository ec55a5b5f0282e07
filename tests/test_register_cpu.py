"""CPU tests of the back end's re-registration (svs_reg_*): the composition tests/register_model.py restates is pinned where reference-compiled code exists
(matcher at radius 10 and 4, refinement with 25 iterations, the gate), the parts that are not (cull, vertex table, observer walk, thresholds: backend.cpp is not
among the reference-compiled libraries) are held to hand-made inputs whose answer can be read off backend.cpp:472-546, 615-722, 853-961, and the header and the
binding agree."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import register_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG_SYMBOLS = ["svs_reg_create", "svs_reg_destroy", "svs_reg_register_batch", "svs_reg_set_timing", "svs_reg_stage_times", "svs_reg_params_default"]
CAM = M.SMALL_CAM


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model_run(scene):
    return M.register(scene, CAM)


# ---- the composition, where oracle/_ref allows --------------------------------------------------------------------------------------------------------------
def test_matcher_at_both_radii_equals_the_reference_compiled_matcher(scene, model_run):
    """GuidedMatcher::match as matchAndAlign calls it (backend.cpp:738-749 at radius 10 from the identity, :763-774 at radius 4 from the refined pose), on the
    registration scene's candidate list: the reference-compiled matcher appends exactly the restatement's OK records, in order, with bit-equal observations."""
    import oracle as O
    cand = np.ascontiguousarray(scene["src"][model_run["cand_src"]])
    trees = M.root_trees(scene)
    corners = []
    for l in range(3):
        g = O.fastgrid_for_level(scene["root_pyr"][l].shape[1], scene["root_pyr"][l].shape[0], l)
        for c, t in enumerate(scene["fast_thr"][l]):
            g.thr[c] = int(t)
        corners.append(O.fastgrid_detect(g, scene["root_pyr"][l])[0])
    # the root is the active keyframe: its vertex-table pose is T_root_from_world
    for radius, T in ((10, np.eye(3, 4)), (4, model_run["T1"])):
        res = M.match(scene, CAM, cand, T, radius, trees)
        idx, obs, xyz = O.ref_match(scene["kf_pyrs"], scene["kf_T"], np.asarray(T).reshape(12), scene["root_kf"], scene["root_pyr"], scene["root_disp"], corners,
                                    M.cams_c(CAM), cand, radius, 22, 10)
        ok = np.nonzero(res["status"] == 0)[0]
        assert len(ok) > 100
        assert np.array_equal(ok, idx), (radius, len(ok), len(idx))
        assert np.array_equal(res["obs"][ok], obs) and np.array_equal(res["xyz_actkey"][ok], xyz), radius


def test_refinement_with_25_iterations_equals_the_reference_compiled_optimizer(model_run):
    import oracle as O
    for res, T0, it in ((model_run["m1"], np.eye(3, 4), 25), (model_run["m2"], model_run["T1"], 15)):
        prm = M.pose_params(it)
        Ta, sa = O.ref_motion_only(res, M.cam_c(CAM), T0, prm)
        Tb, sb = O.motion_only(res, M.cam_c(CAM), T0, prm)
        assert sa.status == sb.status == 0 and np.array_equal(Ta, Tb)
        assert (sa.initial_chi2, sa.chi2, sa.max_err, sa.num_obs) == (sb.initial_chi2, sb.chi2, sb.max_err, sb.num_obs)
    assert np.array_equal(model_run["T1"], O.motion_only(model_run["m1"], M.cam_c(CAM), np.eye(3, 4), M.pose_params(25))[0])


def test_gate_equals_the_reference_compiled_gate(scene, model_run):
    """the inequality of backend.cpp:644-646 / :928-930 is the one of processMatchedPoints at max_reproj_error = 2 (stereo_frontend.cpp:869-871)"""
    import oracle as O
    cand = np.ascontiguousarray(scene["src"][model_run["cand_src"]])
    res = model_run["m2"].copy()
    inside = (res["obs"][:, 0] >= 1) & (res["obs"][:, 0] < CAM["w"] - 1) & (res["obs"][:, 1] >= 1) & (res["obs"][:, 1] < CAM["h"] - 1)
    res["status"][~inside] = 5      # the reference-compiled function asserts that an accepted observation lies inside its level image
    ga = O.ref_process_matched_points(res, cand, 0, M.cam_c(CAM), model_run["T"], 2.0)[0]
    mine = M.gate(res, cand, CAM, model_run["T"])
    assert np.array_equal(ga["accepted"] * (res["status"] == 0), mine)
    assert 0 < mine.sum() < (res["status"] == 0).sum()
    # and restated by hand
    T, c = model_run["T"], CAM
    for k in np.nonzero(res["status"] == 0)[0]:
        p = T[:, :3] @ res["xyz_actkey"][k] + T[:, 3]
        pred = np.array([p[0] / p[2] * c["f"] + c["cx"], p[1] / p[2] * c["f"] + c["cy"], (p[0] - c["b"]) / p[2] * c["f"] + c["cx"]])
        d = np.abs(res["obs"][k] - pred)
        f = 2.0 * (1 << int(cand["anchor_level"][k]))
        margin = min(abs(d[0] - f), abs(d[1] - f), abs(d[2] - 6.0))
        if margin > 1e-9:
            assert bool(mine[k]) == bool(d[0] < f and d[1] < f and d[2] < 6.0), k


def test_model_on_the_scene_is_a_clear_registration(model_run):
    """the end-to-end GPU test needs every strength at least 5 away from covis_thr"""
    st = model_run["kf_stats"]
    assert model_run["status"] == M.OK and model_run["n_qualified"] == 2
    assert np.all(np.abs(st[:, 0] - 15) >= 5) and np.all(np.abs(st[st[:, 0] > 0][:, 1:5] - 7) >= 5)
    assert st[0, 0] == st[1, 0] == st[4, 0] == 0 and list(st[:, 6]) == [1, 0, 1, 1, 0]


# ---- model properties on hand-made inputs --------------------------------------------------------------------------------------------------------------------
def _point(xyz, kf=0, level=0):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    p = np.zeros(1, CANDIDATE_DTYPE)
    p["xyz_anchor"], p["kf_index"], p["anchor_level"] = xyz, kf, level
    return p


def _req(src, flags=(M.IN_WINDOW | M.DIRECT_NEIGHBOR, M.IN_WINDOW), mode=M.LOCAL, obs=None):
    n_kf = len(flags)
    ob, ok = [0], []
    for row in (obs or [[] for _ in src]):
        ok += list(row)
        ob.append(len(ok))
    return dict(mode=mode, T_root=M.I12, root_kf=0, kf_T=np.array([M.I12] * n_kf), flags=np.array(flags, np.uint8), src=np.concatenate(src) if len(src) else src,
                obs_begin=np.array(ob, np.int32), obs_kf=np.array(ok, np.int32))


UNIT_CAM = dict(f=1.0, cx=0.0, cy=0.0, b=0.1, w=8, h=6)      # u = x / z exactly for z = 1: projections at chosen, exactly representable coordinates


def test_cull_truncates_toward_zero_at_the_frame_border():
    """projections at -0.5, 0, w - 1, w - 0.5 and w: (int)(-0.5) = 0 is inside, (int)(w - 0.5) = w - 1 is inside, w is not; the same for v"""
    w, h = UNIT_CAM["w"], UNIT_CAM["h"]
    us = [-1.0, -0.5, 0.0, w - 1.0, w - 0.5, float(w)]
    src = [_point((u, 1.0, 1.0), kf=1) for u in us] + [_point((1.0, v, 1.0), kf=1) for v in (-1.0, -0.5, h - 0.5, float(h))]
    keep, in_vt = M.cull(_req(src), UNIT_CAM)
    assert list(keep) == [1, 2, 3, 4, 7, 8]
    assert list(in_vt) == [1, 1]
    # level 1: the camera of the anchor level decides (w / 2 = 4 columns, f / 2)
    keep, _ = M.cull(_req([_point((7.0, 1.0, 1.0), kf=1, level=1), _point((8.0, 1.0, 1.0), kf=1, level=1)]), UNIT_CAM)
    assert list(keep) == [0]


def test_cull_has_no_depth_test_and_drops_what_no_int_holds():
    """a point behind the camera that projects into the frame is kept (the matcher answers SVS_MATCH_DEPTH later); z = 0 gives infinity or NaN: dropped"""
    src = [_point((-2.0, -2.0, -1.0), kf=1), _point((1.0, 1.0, 0.0), kf=1), _point((0.0, 0.0, 0.0), kf=1), _point((3e10, 1.0, 1.0), kf=1)]
    keep, _ = M.cull(_req(src), UNIT_CAM)
    assert list(keep) == [0]


def test_cull_skips_anchors_outside_the_double_window_and_keeps_them_out_of_the_vertex_table():
    src = [_point((1.0, 1.0, 1.0), kf=1), _point((1.0, 1.0, 1.0), kf=2), _point((100.0, 1.0, 1.0), kf=3), _point((1.0, 1.0, 1.0), kf=7)]
    keep, in_vt = M.cull(_req(src, flags=(3, 1, 0, 1)), UNIT_CAM)
    assert list(keep) == [0]
    assert list(in_vt) == [1, 1, 0, 0]      # entry 2 is outside the window, entry 3 anchors only a culled point


def test_counts_skip_direct_neighbours_and_keyframes_outside_the_vertex_table():
    """entry 1: a direct neighbour; entry 2: observes every accepted point but anchors only culled ones (not in the vertex table); entry 3 counts"""
    n = 20
    src = [_point((1.0 + 0.1 * i, 1.0, 1.0), kf=3) for i in range(n)] + [_point((100.0, 1.0, 1.0), kf=2)]
    req = _req(src, flags=(3, 3, 1, 1), obs=[[1, 2, 3]] * n + [[2]])
    keep, in_vt = M.cull(req, UNIT_CAM)
    assert list(keep) == list(range(n)) and list(in_vt) == [1, 0, 0, 1]
    in_vt[1] = 1      # even inside the vertex table a direct neighbour gets nothing
    uvu = np.array([[i % 8, i % 6, 0.0] for i in range(n)], np.float64)
    st = M.count(req, UNIT_CAM, keep, np.ones(n, np.int32), uvu, in_vt, 15)
    assert st[3, 0] == n and st[1, 0] == st[2, 0] == st[0, 0] == 0
    assert st[3, 1] + st[3, 2] == n and st[3, 3] + st[3, 4] == n


@pytest.mark.parametrize("covis", [15, 16])
@pytest.mark.parametrize("mode", [M.LOCAL, M.LOOP])
def test_thresholds_are_strength_and_integer_halves(covis, mode):
    """strength == covis_thr with one half at covis_thr / 2 - 1 fails, with the half at covis_thr / 2 passes (integer division: 7 for 15, 8 for 16)"""
    half = covis // 2
    cam = dict(UNIT_CAM, w=100, h=100)
    src = [_point((1.0, 1.0, 1.0), kf=1) for _ in range(covis)]
    req = _req(src, mode=mode, obs=[[1]] * covis)
    row = 1 if mode == M.LOCAL else 0
    for n_hi, want in ((half - 1, 0), (half, 1)):
        uvu = np.array([[60.0 if i < n_hi else 40.0, 60.0 if i % 2 else 40.0, 0.0] for i in range(covis)])
        st = M.count(req, cam, np.arange(covis), np.ones(covis, np.int32), uvu, np.array([1, 1]), covis)
        assert st[row, 0] == covis and st[row, 1] == n_hi and st[row, 5] == want
        assert M.decide(mode, covis, covis, covis, int(st[:, 5].sum()), covis) == (M.OK if want else M.NOT_COVISIBLE)
    # u == w / 2 is not "> w / 2"
    uvu = np.array([[50.0, 50.0, 0.0]] * covis)
    st = M.count(req, cam, np.arange(covis), np.ones(covis, np.int32), uvu, np.array([1, 1]), covis)
    assert st[row, 1] == 0 and st[row, 2] == covis and st[row, 3] == 0 and st[row, 4] == covis
    # one observation short of covis_thr
    acc = np.ones(covis, np.int32); acc[0] = 0
    uvu = np.array([[60.0 if i % 2 else 40.0, 60.0 if (i // 2) % 2 else 40.0, 0.0] for i in range(covis)])
    assert M.count(req, cam, np.arange(covis), acc, uvu, np.array([1, 1]), covis)[row, 5] == 0
    assert M.count(req, cam, np.arange(covis), np.ones(covis, np.int32), uvu, np.array([1, 1]), covis)[row, 5] == 1


def test_exits_are_taken_in_the_reference_order():
    assert M.decide(M.LOCAL, 14, 0, 0, 0, 15) == M.FEW_CANDIDATES
    assert M.decide(M.LOOP, 14, 14, 0, 0, 15) == M.FEW_MATCHES_PASS1      # globalLoopClosure has no candidate-count exit
    assert M.decide(M.LOCAL, 15, 15, 14, 3, 15) == M.FEW_MATCHES_PASS2
    assert M.decide(M.LOCAL, 15, 15, 15, 0, 15) == M.NOT_COVISIBLE
    assert M.decide(M.LOCAL, 15, 15, 15, 1, 15) == M.OK


# ---- header and binding ----------------------------------------------------------------------------------------------------------------------------------------
def test_binding_names_the_registration_entry_points():
    from scavislam_amd import capi
    for n in REG_SYMBOLS:
        assert n in capi.EXPORTS, n
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    for n in REG_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    lib = capi.load()
    for n in REG_SYMBOLS:
        assert hasattr(lib, n)
    from scavislam_amd.ctypes_types import RegParams
    p = RegParams()
    lib.svs_reg_params_default(C.byref(p))
    q = RegParams.reference()
    assert bytes(p) == bytes(q) and (p.covis_thr, list(p.search_radius), p.thr_mean, p.thr_std, list(p.num_iter), p.reproj_thr, p.kernel_param) == (
        15, [10, 4], 22, 10, [25, 15], 2.0, 2.0)


def test_pod_layouts_of_the_registration_structs(tmp_path):
    from scavislam_amd.ctypes_types import REG_KF_STATS_DTYPE, RegParams, RegRequest, RegResult
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n",'
                   "sizeof(svs_reg_params),sizeof(svs_reg_request),sizeof(svs_reg_result),sizeof(svs_reg_kf_stats),offsetof(svs_reg_params,reproj_thr),"
                   "offsetof(svs_reg_request,fast_thr),offsetof(svs_reg_request,T_root_from_world),offsetof(svs_reg_request,h_obs_kf),"
                   "offsetof(svs_reg_result,T_pass1),offsetof(svs_reg_result,stats_pass2),SVS_REG_STAGES);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    from scavislam_amd.ctypes_types import REG_STAGES
    assert got == [C.sizeof(RegParams), C.sizeof(RegRequest), C.sizeof(RegResult), REG_KF_STATS_DTYPE.itemsize, RegParams.reproj_thr.offset,
                   RegRequest.fast_thr.offset, RegRequest.T_root_from_world.offset, RegRequest.h_obs_kf.offset, RegResult.T_pass1.offset,
                   RegResult.stats_pass2.offset, REG_STAGES]
