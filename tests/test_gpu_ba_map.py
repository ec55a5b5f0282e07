"""GPU tests of the double window's BA problem built from the device-resident map: svs_map_add_measured_observations, svs_map_prepare_window,
svs_ba_window_from_map, svs_ba_store_to_map and svs_ba_window_edges against the NumPy model (tests/ba_map_model.py), the upload path (svs_ba_window_update on
the model's arrays) and the oracle.  The scene is ba_map_model.scene(): 14 keyframes (8 INNER, 3 OUTER, 3 outside W0), 1 340 active of 1 700 points."""
import numpy as np
import pytest

import ba_map_model as BM

MAP_CAPS = dict(max_keyframes=256, max_points=20000, max_observations=16384)


def _rel_update_err(new, ref, start):      # the bar of tests/test_gpu_ba.py
    upd = np.abs(ref - start).max()
    return np.abs(new - ref).max() / max(upd, 1e-300)


@pytest.fixture(scope="module")
def scene():
    return BM.scene()


@pytest.fixture(scope="module")
def model(scene):
    prep = BM.prepare(scene["map"], scene["w0_ids"], scene["w0_types"], scene["pairs"])
    return prep, BM.problem(scene["map"], prep["window_ids"], prep["active_ids"])


@pytest.fixture(scope="module")
def frames(gpu_ctx, scene):
    """one blank pyramid and disparity for every keyframe: the walks never read them, the flag probe's registrar finds no corner in them"""
    import torch
    ctx, stream = gpu_ctx
    w, h = int(scene["cam"]["w"]), int(scene["cam"]["h"])
    with torch.cuda.stream(stream):
        pyr = [torch.zeros((h >> l, w >> l), dtype=torch.uint8, device="cuda") for l in range(3)]
        disp = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    ctx.sync()
    return pyr, disp


def _fill(ctx, frames, scene, rng=None, caps=None):
    """the scene as a ResidentMap; rng: the same content in a shuffled order, in several calls of each kind, one of them repeated"""
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    from scavislam_amd.register import ResidentMap, keyframe_table
    m = scene["map"]
    pyr, disp = frames
    dmap = ResidentMap(ctx, **(caps or MAP_CAPS))
    pts = np.zeros(len(m["point_ids"]), CANDIDATE_DTYPE)
    pts["xyz_anchor"], pts["kf_index"] = m["xyz"], m["anchor_ids"]
    kf_order = np.arange(len(m["kf_ids"])) if rng is None else rng.permutation(len(m["kf_ids"]))
    pt_order = np.arange(len(pts)) if rng is None else rng.permutation(len(pts))
    ob_order = np.arange(len(m["obs_point"])) if rng is None else rng.permutation(len(m["obs_point"]))
    for part in np.array_split(kf_order, 1 if rng is None else 3):
        kfs = keyframe_table([([t.data_ptr() for t in pyr], [t.shape[1] for t in pyr], m["kf_poses"][i]) for i in part])
        dmap.add_keyframes(m["kf_ids"][part], kfs, [(disp.data_ptr(), disp.shape[1])] * len(part), [[[25], [25], [25]]] * len(part))
    for part in np.array_split(pt_order, 1 if rng is None else 4):
        dmap.add_points(m["point_ids"][part], pts[part])
    parts = np.array_split(ob_order, 1 if rng is None else 5)
    for part in parts + ([] if rng is None else [parts[1]]):                                   # pairs already present are ignored
        dmap.add_measured_observations(m["obs_point"][part], m["obs_kf"][part], m["obs_center"][part], m["obs_level"][part])
    return dmap


def _prepare(dmap, scene, **kw):
    return dmap.prepare_window(scene["w0_ids"], scene["w0_types"], scene["pairs"], **kw)


@pytest.fixture(scope="module")
def dmap(gpu_ctx, frames, scene):
    d = _fill(gpu_ctx[0], frames, scene)
    yield d
    d.close()


def _cam(scene):
    from scavislam_amd.ctypes_types import Cam
    c = scene["cam"]
    return Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"])


def _all_observations(m):
    from scavislam_amd.ctypes_types import BA_EDGE_DTYPE
    e = np.zeros(len(m["obs_point"]), BA_EDGE_DTYPE)
    e["obs"], e["info"], e["point"], e["pose"] = m["obs_center"], BM.info_from_level(m["obs_level"]), m["obs_point"], m["obs_kf"]
    return e


def _upload(opt, scene, prob, new_obs):
    """the upload path: svs_ba_window_update given the model's arrays"""
    opt.windowUpdate(prob["pose_ids"], prob["poses"], prob["point_ids"], prob["psi"], prob["anchor_ids"], new_obs, scene["cons"], _cam(scene))


def _state(opt):
    poses, psi = opt.restoreDataFromG2o()
    return poses.tobytes(), psi.tobytes(), opt.window_edges().tobytes()


def _info(opt):
    i = opt.info()
    return i["solve_kernel"], i["envelope_rows"], i["wave_chunks"], i["wide_landmarks"]


@pytest.fixture(scope="module")
def registrar(gpu_ctx, scene):
    from scavislam_amd.register import KeyframeRegistrar
    reg = KeyframeRegistrar(gpu_ctx[0], scene["cam"], max_requests=8, max_points=2048, max_keyframes=16, max_observers=16384)
    yield reg
    reg.close()


def _flag_probe(reg, dmap, scene):
    """SVS_REG_KF_IN_WINDOW as the registration chain sees it: a loop-closure request per keyframe q culls the points of q's feature_table whose anchor is not in
    the window (backend.cpp:861).  -> {q: the candidates' point ids}"""
    from scavislam_amd.ctypes_types import REG_LOOP
    m = scene["map"]
    out = {}
    ids = m["kf_ids"].tolist()
    for part in (ids[:8], ids[8:]):
        qs = [dict(mode=REG_LOOP, root_kf=q, T_root_from_world=m["kf_poses"][ids.index(q)], walk_kf=[q], direct_kf=[]) for q in part]
        for q, o in zip(part, reg.register_map_batch(dmap, qs)):
            out[q] = tuple(int(p) for p in o.point_ids)
    return out


def _flagged_by_own_points(probe, scene):
    """keyframe q is flagged iff the points it anchors AND observes (they project to their own pixel in q) survive the cull of the request rooted at q"""
    m = scene["map"]
    anchor_of = dict(zip(m["point_ids"].tolist(), m["anchor_ids"].tolist()))
    own = {}
    for p, f in zip(m["obs_point"].tolist(), m["obs_kf"].tolist()):
        if anchor_of[p] == f:
            own.setdefault(f, set()).add(p)
    flagged = set()
    for q, cand in probe.items():
        mine = {p for p in cand if anchor_of[p] == q}
        assert mine in (set(), own.get(q, set())), q
        if mine:
            flagged.add(q)
    return flagged, set(own)


@pytest.mark.gpu
def test_prepare_window_equals_the_model(gpu_ctx, dmap, registrar, scene, model):
    prep, prob = model
    m = scene["map"]
    assert dmap.measured_info() == (len(m["obs_point"]), 0) and dmap.info() == (len(m["kf_ids"]), len(m["point_ids"]), len(m["obs_point"]))
    dmap.set_window([])
    res, wid, wtype = _prepare(dmap, scene, set_window_flags=True)
    assert (res.n_window, res.n_initial, res.n_active, res.n_edges_bound) == (len(prep["window_ids"]), len(scene["w0_ids"]), len(prep["active_ids"]), prep["n_edges_bound"])
    assert np.array_equal(wid, prep["window_ids"]) and np.array_equal(wtype, prep["window_types"])
    # the flags: exactly the final window, as svs_map_set_window on it leaves them
    by_prepare = _flag_probe(registrar, dmap, scene)
    flagged, anchors = _flagged_by_own_points(by_prepare, scene)
    assert flagged == set(prep["window_ids"].tolist()) & anchors and anchors - flagged == {int(m["kf_ids"][0])}
    dmap.set_window(prep["window_ids"])
    assert _flag_probe(registrar, dmap, scene) == by_prepare
    # set_window_flags = 0 leaves them as they are
    dmap.set_window(scene["w0_ids"])
    res2, wid2, _ = _prepare(dmap, scene, set_window_flags=False)
    assert res2.n_active == res.n_active and np.array_equal(wid2, wid)
    flagged0, _ = _flagged_by_own_points(_flag_probe(registrar, dmap, scene), scene)
    assert flagged0 == set(scene["w0_ids"].tolist()) & anchors
    # window_cap exactly the final window still fits
    res3, wid3, _ = _prepare(dmap, scene, set_window_flags=False, window_cap=len(wid))
    assert res3.n_active == res.n_active and np.array_equal(wid3, wid)


@pytest.mark.gpu
def test_from_map_equals_the_upload_path_and_both_follow_the_oracle(gpu_ctx, dmap, scene, model):
    import oracle as O
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams
    ctx, stream = gpu_ctx
    prep, prob = model
    _prepare(dmap, scene)
    a, b = SlamGraphOptimizer(ctx, stream), SlamGraphOptimizer(ctx, stream)
    a.windowFromMap(dmap, scene["cons"], _cam(scene))
    _upload(b, scene, prob, _all_observations(scene["map"]))
    assert (a.P, a.L) == (b.P, b.L) == (len(prob["pose_ids"]), len(prob["point_ids"]))
    sa, sb = _state(a), _state(b)
    assert sa[0] == sb[0] == prob["poses"].tobytes(), "poses differ"
    assert sa[1] == sb[1] == prob["psi"].tobytes(), "psi differs from invert_depth(xyz_anchor) bit for bit"
    assert sa[2] == sb[2], "assembled edge lists differ"
    assert _info(a) == _info(b)
    # the edge list is the model's: (point, pose) pairs with measurement and information, anchors by window index
    edges = a.window_edges()
    widx = {int(k): i for i, k in enumerate(prob["pose_ids"])}
    got = {(int(e["point"]), int(e["pose"]), int(e["anchor"]), e["obs"].tobytes(), e["info"].tobytes()) for e in edges}
    lidx = {int(p): i for i, p in enumerate(prob["point_ids"])}
    want = {(lidx[int(e["point"])], widx[int(e["pose"])], widx[int(e["anchor"])], e["obs"].tobytes(), e["info"].tobytes()) for e in prob["edges"]}
    assert len(edges) == len(prob["edges"]) and got == want
    # optimize on both and on the oracle
    cons = scene["cons"].copy()
    cons["pose1"] = [widx[int(k)] for k in scene["cons"]["pose1"]]; cons["pose2"] = [widx[int(k)] for k in scene["cons"]["pose2"]]
    prm = BaParams.reference_defaults()
    # the export after the third way to set a problem (svs_ba_set_problem, marshalled on the host at this size): the same edges, whatever its slot order
    by_idx = prob["edges"].copy()
    by_idx["point"] = [lidx[int(p)] for p in prob["edges"]["point"]]; by_idx["pose"] = [widx[int(k)] for k in prob["edges"]["pose"]]
    by_idx["anchor"] = [widx[int(k)] for k in prob["edges"]["anchor"]]
    s = SlamGraphOptimizer(ctx, stream)
    s.copyDataToG2o(prob["poses"], prob["psi"], by_idx, cons, _cam(scene), prm)
    es = s.window_edges()
    assert len(es) == len(edges) and {(int(e["point"]), int(e["pose"]), int(e["anchor"]), e["obs"].tobytes(), e["info"].tobytes()) for e in es} == want
    s.close()
    poses_ref, psi_ref, st_ref = O.ba_optimize(prob["poses"], prob["psi"], edges, cons, _cam(scene), prm)
    assert st_ref.accepted >= 1 and st_ref.chi2_final < st_ref.chi2_init
    for name, opt in (("from map", a), ("upload", b)):
        st = opt.optimize()
        poses, psi = opt.restoreDataFromG2o()
        assert (st.iterations, st.trials, st.accepted, st.terminated) == (st_ref.iterations, st_ref.trials, st_ref.accepted, st_ref.terminated), name
        ep, el = _rel_update_err(poses, poses_ref, prob["poses"]), _rel_update_err(psi, psi_ref, prob["psi"])
        print(f"{name}: pose update rel err {ep:.2e}, psi {el:.2e}")
        assert ep < 1e-6 and el < 1e-6, name
    # a later svs_ba_window_update on the handle that took the map's window still equals a fresh handle's
    c = SlamGraphOptimizer(ctx, stream)
    half = _all_observations(scene["map"])[::2]
    _upload(a, scene, prob, half); _upload(c, scene, prob, half)
    assert _state(a) == _state(c) and _info(a) == _info(c)
    with pytest.raises(Exception):
        a.storeToMap(dmap)                                                                      # the handle's problem is no longer the map's window
    for o in (a, b, c):
        o.close()


@pytest.mark.gpu
def test_result_does_not_depend_on_order_grouping_or_repetition(gpu_ctx, frames, dmap, scene, model):
    from scavislam_amd.backend import SlamGraphOptimizer
    ctx, stream = gpu_ctx
    prep, _ = model
    second = _fill(ctx, frames, scene, rng=np.random.default_rng(3))
    assert second.measured_info() == dmap.measured_info() and second.info() == dmap.info()
    states = []
    for d in (dmap, second, second):                                                            # (and repetition)
        res, wid, wtype = _prepare(d, scene)
        assert res.n_active == len(prep["active_ids"]) and res.n_edges_bound == prep["n_edges_bound"] and np.array_equal(wid, prep["window_ids"])
        opt = SlamGraphOptimizer(ctx, stream)
        opt.windowFromMap(d, scene["cons"], _cam(scene))
        states.append(_state(opt) + (_info(opt),))
        opt.close()
    assert states[0] == states[1] == states[2]
    second.close()


@pytest.mark.gpu
def test_store_to_map_and_pose_updates_between_prepare_and_from_map(gpu_ctx, frames, scene, model):
    from scavislam_amd.backend import SlamGraphOptimizer
    ctx, stream = gpu_ctx
    prep, prob = model
    d = _fill(ctx, frames, scene)
    opt = SlamGraphOptimizer(ctx, stream)
    _prepare(d, scene)
    # reinitializePoses runs between the two steps: svs_map_set_poses / svs_map_set_points do not invalidate the window and are honoured
    k = [1, len(prob["pose_ids"]) - 1]                                                          # a keyframe of W0 and one of the extension
    T = prob["poses"].copy(); T[k, 3] += 0.125; T[k, 7] -= 0.0625
    d.set_poses(prob["pose_ids"][k], T[k])
    pid = prob["point_ids"][[0, 1025]]
    xyz = np.array([[0.5, -0.25, 3.0], [1.5, 0.75, 7.0]])
    d.set_points(pid, xyz)
    opt.windowFromMap(d, scene["cons"], _cam(scene))
    poses0, psi0 = opt.restoreDataFromG2o()
    psi_exp = prob["psi"].copy(); psi_exp[[0, 1025]] = BM.invert_depth(xyz)
    assert poses0.tobytes() == T.tobytes() and psi0.tobytes() == psi_exp.tobytes()
    # optimize, store, and start again from the map: exactly the optimised state
    st = opt.optimize()
    assert st.accepted >= 1
    poses1, psi1 = opt.restoreDataFromG2o()
    opt.storeToMap(d)
    res, wid, _ = _prepare(d, scene)
    assert res.n_active == len(prob["point_ids"]) and np.array_equal(wid, prob["pose_ids"])
    with pytest.raises(Exception):
        opt.storeToMap(d)                                                                       # a new prepare: the handle's problem is the previous window
    opt.windowFromMap(d, scene["cons"], _cam(scene))
    poses2, psi2 = opt.restoreDataFromG2o()
    assert poses2.tobytes() == poses1.tobytes()
    assert psi2.tobytes() == BM.invert_depth(BM.invert_depth(psi1)).tobytes()                   # psi goes through invert_depth twice
    assert not np.array_equal(poses1, poses0)
    opt.close(); d.close()


@pytest.mark.gpu
def test_refusals_leave_the_map_and_the_handle_as_they_were(gpu_ctx, frames, scene, model):
    from scavislam_amd import capi
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    ctx, stream = gpu_ctx
    prep, prob = model
    m = scene["map"]
    d = _fill(ctx, frames, scene)
    opt = SlamGraphOptimizer(ctx, stream)
    with pytest.raises(capi.SvsError):
        opt.windowFromMap(d, scene["cons"], _cam(scene))                                        # nothing prepared yet
    _prepare(d, scene)
    opt.windowFromMap(d, scene["cons"], _cam(scene))
    before = _state(opt)
    w0, t0, pairs = scene["w0_ids"], scene["w0_types"], scene["pairs"]
    # section 2, before anything is uploaded: the prepared window stays
    for bad in (dict(kf_ids=np.append(w0[:-1], 9999)), dict(kf_ids=np.append(w0[:-1], w0[0])), dict(kf_type=np.append(t0[:-1], 2)), dict(kf_type=np.ones_like(t0)),
                dict(edge_pairs=np.vstack([pairs, [[w0[0], 9998]]])), dict(window_cap=len(w0) - 1), dict(window_cap=257)):
        args = dict(kf_ids=w0, kf_type=t0, edge_pairs=pairs)
        args.update(bad)
        with pytest.raises(capi.SvsError):
            d.prepare_window(**args)
    with pytest.raises(capi.SvsError):
        d.add_measured_observations(m["obs_point"][:1] + 1, m["obs_kf"][:1], m["obs_center"][:1], [0])      # an unknown point
    with pytest.raises(capi.SvsError):
        d.add_measured_observations(m["obs_point"][:1], m["obs_kf"][:1], m["obs_center"][:1], [3])          # a level outside the pyramid
    opt.windowFromMap(d, scene["cons"], _cam(scene))
    assert _state(opt) == before
    # section 3: a constraint outside the final window, handles of two contexts
    bad_cons = scene["cons"].copy(); bad_cons["pose2"][0] = m["kf_ids"][0]
    with pytest.raises(capi.SvsError):
        opt.windowFromMap(d, bad_cons, _cam(scene))
    assert _state(opt) == before
    ctx2 = capi.Context(0)
    other = SlamGraphOptimizer(ctx2)
    with pytest.raises(capi.SvsError):
        other.windowFromMap(d, scene["cons"], _cam(scene))
    other.close(); ctx2.close()
    # over capacity is only known on the device: the count found, nothing prepared, the handle untouched
    res, wid, wtype = _prepare(d, scene, window_cap=len(prep["window_ids"]) - 1)
    assert (res.n_window, res.n_initial, res.n_active) == (len(prep["window_ids"]), len(w0), -1) and len(wid) == 0
    with pytest.raises(capi.SvsError):
        opt.windowFromMap(d, scene["cons"], _cam(scene))
    with pytest.raises(capi.SvsError):
        opt.storeToMap(d)
    assert _state(opt) == before
    res, wid, _ = _prepare(d, scene)
    assert res.n_active == len(prep["active_ids"]) and np.array_equal(wid, prep["window_ids"])
    # an update of the map's points or observations invalidates the prepared window
    pt = np.zeros(1, CANDIDATE_DTYPE); pt["xyz_anchor"], pt["kf_index"] = [0.0, 0.0, 5.0], m["kf_ids"][7]
    d.add_points([19999], pt)
    with pytest.raises(capi.SvsError):
        opt.windowFromMap(d, scene["cons"], _cam(scene))
    assert _state(opt) == before
    _prepare(d, scene)
    opt.windowFromMap(d, scene["cons"], _cam(scene))
    assert _state(opt) == before                                                                # the new point is observed by nobody
    # a pair without a measurement: no window can be formed from this map any more
    d.add_observations([19999], [m["kf_ids"][7]])
    assert d.measured_info() == (len(m["obs_point"]), 1)
    with pytest.raises(capi.SvsError):
        _prepare(d, scene)
    with pytest.raises(capi.SvsError):
        opt.windowFromMap(d, scene["cons"], _cam(scene))
    assert _state(opt) == before
    opt.close(); d.close()


@pytest.mark.gpu
def test_cpp_adaptor_agrees_with_its_host_marshalled_call(gpu_ctx, tmp_path):
    """tests/cpp/ba_map_smoke.cpp: BackendMap::addObservations (centres, levels) / prepareForOptimization and SlamGraphBA::copyDataFromMap / restoreDataToMap of
    include/scavislam_hip.hpp against SlamGraphBA::optimizeWindow on the same tables"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "ba_map_smoke"
    libdir = os.path.join(root, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "ba_map_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("BA_MAP ")]
    assert tok and tok[0].split()[1:4] == ["ok", "4", "60"], out
    assert int(tok[0].split()[4]) >= 1
