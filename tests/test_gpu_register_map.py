"""GPU tests of the device-resident map (svs_map_*) and of re-registration by ids (svs_reg_register_map_batch): every output is held, byte for byte, against
svs_reg_register_batch on the request that tests/register_map_model.py builds from a host mirror of the same map -- the stateless call is the yardstick, and
tests/test_gpu_register.py holds it to the reference.  Scene: register_model.make_scene() at SMALL_CAM, put into a map by register_map_model.fill()."""
import os
import subprocess

import numpy as np
import pytest

import register_map_model as MM
import register_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = M.SMALL_CAM
EXIT3_ID = 51
MAP_CAPS = dict(max_keyframes=64, max_points=2048, max_observations=8192)


@pytest.fixture(scope="module")
def scene():
    return M.make_scene()


@pytest.fixture(scope="module")
def model_run(scene):
    return M.register(scene, CAM)


@pytest.fixture(scope="module")
def device_scene(gpu_ctx, scene):
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


@pytest.fixture(scope="module")
def exit3_ids(scene, model_run):
    """16 points of which the first match finds at least 15 and the second fewer: the third exit, as tests/test_gpu_register.py builds it"""
    from test_gpu_register import _exit3_request
    return [int(p) for p in _exit3_request(scene, model_run)["src"]["point_id"]]


@pytest.fixture(scope="module")
def few_ids(scene, model_run):
    return [int(p) for p in scene["src"]["point_id"][model_run["cand_src"][:10]]]


def _frames(dev, kf_id, entry):
    """(pyramid tensors, disparity tensor) of a keyframe of the map: the second root lives in buffers of its own"""
    if kf_id == MM.ROOT2_ID:
        return dev["root_copy"], dev["disp_copy"]
    return dev["pyrs"][entry], dev["disp"]


class DeviceMap:
    """ResidentMap behind the update methods of MapModel, so that register_map_model.fill() and a replay of its calls drive both"""

    def __init__(self, ctx, dev, scene, **caps):
        from scavislam_amd.register import ResidentMap
        self.map, self.dev, self.scene = ResidentMap(ctx, **(caps or MAP_CAPS)), dev, scene

    def add_keyframes(self, ids, Ts, entry, fast_thr=None):
        from scavislam_amd.register import keyframe_table
        frames = [_frames(self.dev, int(k), e) for k, e in zip(ids, entry)]
        kfs = keyframe_table([([t.data_ptr() for t in p], [t.shape[1] for t in p], T) for (p, _), T in zip(frames, Ts)])
        self.map.add_keyframes(ids, kfs, [(d.data_ptr(), d.shape[1]) for _, d in frames], fast_thr or [self.scene["fast_thr"]] * len(ids))

    def __getattr__(self, name):
        return getattr(self.map, name)


def _extra(m, exit3_ids):
    """the keyframe of the third exit: observes exactly its 16 points"""
    m.add_keyframes([EXIT3_ID], [M.I12], entry=[1])
    m.add_observations(exit3_ids, [EXIT3_ID] * len(exit3_ids))


def _fill_both(ctx, dev, scene, few_ids, exit3_ids):
    model, dmap = MM.MapModel(), DeviceMap(ctx, dev, scene)
    for m in (model, dmap):
        MM.fill(m, scene, cand_ids_few=few_ids, attach=lambda e: dict(entry=e))
        _extra(m, exit3_ids)
    return model, dmap


@pytest.fixture(scope="module")
def both(gpu_ctx, device_scene, scene, few_ids, exit3_ids):
    """the host mirror and the device map, each built by one call of each kind"""
    model, dmap = _fill_both(gpu_ctx[0], device_scene, scene, few_ids, exit3_ids)
    yield model, dmap
    dmap.close()


def _stateless(registrar, dev, model, scene, qs):
    """svs_reg_register_batch on the requests the model builds for the id requests qs -> (model requests, outputs)"""
    from scavislam_amd.register import keyframe_table
    reqs, dreqs = [], []
    for q in qs:
        req = model.request(q["mode"], q["root_kf"], q["T_root_from_world"], q["walk_kf"], q["direct_kf"])
        frames = [_frames(dev, int(k), model.kf[int(k)]["entry"]) for k in req["kf_ids"]]
        kfs = keyframe_table([([t.data_ptr() for t in p], [t.shape[1] for t in p], T) for (p, _), T in zip(frames, req["kf_T"])])
        disp = frames[0][1]
        dreqs.append(dict(kfs=kfs, flags=req["flags"], root_kf=0, root_disp=(disp.data_ptr(), disp.shape[1]), fast_thr=scene["fast_thr"], T_root_from_world=req["T_root"],
                          src=req["src"], obs_begin=req["obs_begin"], obs_kf=req["obs_kf"]))
        reqs.append(req)
    return reqs, registrar.register_batch(dreqs, [q["mode"] for q in qs], want_pass1=True)


def _raw_of(registrar, i):
    raw = registrar.raw
    sz = len(raw["results"]) // max(len(raw["cand_src"]), 1)
    return (raw["results"][i * sz:(i + 1) * sz], raw["cand_src"][i].tobytes(), raw["matches"][i].tobytes(), raw["status_pass1"][i].tobytes(),
            raw["accepted"][i].tobytes(), raw["kf_stats"][i].tobytes(), raw["matches_pass1"][i].tobytes())


def _lists_of(registrar, i):
    raw = registrar.raw
    return raw["point_ids"][i].tobytes(), raw["kf_ids"][i].tobytes(), int(raw["n_kf"][i])


def _same(a, b, what):
    names = ("results", "cand_src", "matches", "status_pass1", "accepted", "kf_stats", "matches_pass1")
    for n, x, y in zip(names, a, b):
        assert np.array_equal(np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)), (what, n)


def _by_map(registrar, dmap, qs):
    outs = registrar.register_map_batch(dmap.map, qs, want_pass1=True)
    return outs, [_raw_of(registrar, i) for i in range(len(qs))], [_lists_of(registrar, i) for i in range(len(qs))]


def _check_against_stateless(registrar, dev, model, dmap, scene, qs):
    outs, raws, _ = _by_map(registrar, dmap, qs)
    reqs, souts = _stateless(registrar, dev, model, scene, qs)
    for i, (req, out, sout) in enumerate(zip(reqs, outs, souts)):
        _same(raws[i], _raw_of(registrar, i), ("request", i))
        assert np.array_equal(out.kf_ids, req["kf_ids"]), (out.kf_ids, req["kf_ids"])
        assert np.array_equal(out.point_ids, req["point_ids"][sout.cand_src])
        assert np.array_equal(sout.cand_src, M.cull(req, CAM)[0])
    return outs, raws


# ---- 1. the map call against the stateless call ------------------------------------------------------------------------------------------------------------------
def test_map_call_equals_the_stateless_call_on_the_models_request(registrar, device_scene, scene, both):
    model, dmap = both
    qs = [MM.scene_request(scene, M.LOCAL), MM.scene_request(scene, M.LOOP)]
    for q in qs:      # one request per call
        outs, _ = _check_against_stateless(registrar, device_scene, model, dmap, scene, [q])
        assert outs[0].status == M.OK and outs[0].n_candidates >= 200 and outs[0].n_accepted > 100
    assert dmap.info() == model.info()


# ---- 2. how the map was built does not matter ----------------------------------------------------------------------------------------------------------------------
def test_increments_in_a_shuffled_order_give_the_bytes_of_one_call_of_each_kind(gpu_ctx, registrar, device_scene, scene, both, few_ids, exit3_ids):
    model, dmap = both
    qs = [MM.scene_request(scene, M.LOCAL), MM.scene_request(scene, M.LOOP), MM.scene_request(scene, M.LOCAL, MM.ROOT2_ID)]
    _, want, want_lists = _by_map(registrar, dmap, qs)
    rng = np.random.default_rng(11)
    part = MM.MapModel()                                   # the host mirror of the second build, increment by increment
    second = DeviceMap(gpu_ctx[0], device_scene, scene)
    try:
        both_maps = lambda name, *a, **kw: [getattr(m, name)(*a, **kw) for m in (part, second)]
        kf_ids = sorted(model.kf)
        kf_ids = [kf_ids[i] for i in rng.permutation(len(kf_ids))]
        for chunk in (kf_ids[:3], kf_ids[3:]):                                                                   # increments 1-2
            both_maps("add_keyframes", chunk, [model.kf[k]["T"] for k in chunk], entry=[model.kf[k]["entry"] for k in chunk])
        pt_ids = sorted(model.pt)
        pt_ids = [pt_ids[i] for i in rng.permutation(len(pt_ids))]
        for chunk in (pt_ids[:200], pt_ids[200:]):                                                               # 3-4
            both_maps("add_points", chunk, np.concatenate([model.pt[p].reshape(1) for p in chunk]))
        pairs = sorted(model.obs)
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        a, b = len(pairs) // 3, 2 * len(pairs) // 3
        both_maps("add_observations", [p for p, _ in pairs[:a]], [k for _, k in pairs[:a]])                      # 5: before any request
        both_maps("set_window", [k for k in model.kf if model.kf[k]["window"]])
        _check_against_stateless(registrar, device_scene, part, second, scene, qs[:1])                          # a request on a third of the observations
        dup = pairs[:50]
        both_maps("add_observations", [p for p, _ in pairs[a:b] + dup], [k for _, k in pairs[a:b] + dup])        # 6: between requests, with pairs already present
        _check_against_stateless(registrar, device_scene, part, second, scene, qs[:1])
        both_maps("add_observations", [p for p, _ in pairs[b:] + pairs[b:b + 20]], [k for _, k in pairs[b:] + pairs[b:b + 20]])      # 7: pairs twice in one call
        assert second.info() == dmap.info() == model.info()
        _, got, got_lists = _by_map(registrar, second, qs)
        for i in range(len(qs)):
            _same(got[i], want[i], ("request", i))
        assert got_lists == want_lists
        second.add_observations([p for p, _ in pairs[:30]], [k for _, k in pairs[:30]])                          # after the requests: nothing new, nothing changes
        _, again, _ = _by_map(registrar, second, qs)
        assert again == got and second.info() == model.info()
    finally:
        second.close()


# ---- 3. updates are seen -------------------------------------------------------------------------------------------------------------------------------------------
def test_pose_point_and_window_updates_reach_the_result(gpu_ctx, registrar, device_scene, scene, few_ids, exit3_ids):
    model, dmap = _fill_both(gpu_ctx[0], device_scene, scene, few_ids, exit3_ids)
    try:
        q = MM.scene_request(scene, M.LOCAL)
        _, before = _check_against_stateless(registrar, device_scene, model, dmap, scene, [q])
        anchor = MM.scene_ids(scene)[2]
        T = model.kf[anchor]["T"].copy()
        T[3] += 0.004; T[7] -= 0.003
        pts = [int(p) for p in scene["src"]["point_id"][:80]]
        xyz = np.array([model.pt[p]["xyz_anchor"] for p in pts]) * 1.004
        window = [k for k in model.kf if model.kf[k]["window"] and k != anchor]
        for name, args in (("set_poses", ([anchor], [T])), ("set_points", (pts, xyz)), ("set_window", (window,))):
            for m in (model, dmap):
                getattr(m, name)(*args)
            outs, after = _check_against_stateless(registrar, device_scene, model, dmap, scene, [q])
            assert after[0] != before[0], name      # a map that ignored the update would pass the comparison above with a model that ignored it too; not this
            before = after
        assert outs[0].kf_stats["in_vertex_table"][2] == 0      # the anchor that left the window anchors no candidate any more
    finally:
        dmap.close()


# ---- 4. batches ----------------------------------------------------------------------------------------------------------------------------------------------------
def _batch_of_8(scene):
    ids = MM.scene_ids(scene)
    T = scene["T_root"]
    return [MM.scene_request(scene, M.LOCAL), MM.scene_request(scene, M.LOOP),
            dict(mode=M.LOCAL, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[MM.FEW_ID], direct_kf=[]),             # exit 1: 10 candidates
            dict(mode=M.LOOP, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[MM.FEW_ID], direct_kf=[]),              # exit 2: at most 10 observations
            dict(mode=M.LOOP, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[EXIT3_ID], direct_kf=[]),               # exit 3
            dict(mode=M.LOCAL, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[MM.ALL_ID], direct_kf=ids[1:]),        # exit 4: every anchor a direct neighbour
            MM.scene_request(scene, M.LOCAL, MM.ROOT2_ID), MM.scene_request(scene, M.LOOP, MM.ROOT2_ID)]


def test_batch_of_8_equals_the_single_runs_and_itself(registrar, device_scene, scene, both):
    model, dmap = both
    qs = _batch_of_8(scene)
    outs, together, lists = _by_map(registrar, dmap, qs)
    assert [o.status for o in outs] == [0, 0, 1, 2, 3, 4, 0, 0]
    assert outs[2].n_candidates == 10 and outs[4].n_candidates == 16 and outs[5].n_accepted > 100 and outs[5].n_qualified == 0
    for i, q in enumerate(qs):
        _, alone, alone_lists = _by_map(registrar, dmap, [q])
        _same(alone[0], together[i], ("alone", i))
        assert alone_lists[0] == lists[i]
    _, again, again_lists = _by_map(registrar, dmap, qs)
    assert again == together and again_lists == lists
    # and the whole batch is the stateless call's
    _check_against_stateless(registrar, device_scene, model, dmap, scene, qs)


# ---- 5. capacity on the device ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,caps", [(M.LOCAL, dict(max_points=256, max_keyframes=8, max_observers=4096)),      # 450 source points
                                       (M.LOOP, dict(max_points=512, max_keyframes=4, max_observers=4096)),       # 5 table entries behind a walk of one
                                       (M.LOCAL, dict(max_points=512, max_keyframes=8, max_observers=100))])      # some 1500 observer entries
def test_a_request_over_the_registrars_capacity_is_answered_alone(gpu_ctx, scene, both, mode, caps):
    from scavislam_amd.ctypes_types import REG_OVER_CAPACITY
    from scavislam_amd.register import KeyframeRegistrar
    model, dmap = both
    T = scene["T_root"]
    small_q = dict(mode=M.LOOP, root_kf=MM.ROOT_ID, T_root_from_world=T, walk_kf=[MM.OFFWALK_ID], direct_kf=[])      # 8 points, 3 table entries, no rows
    reg = KeyframeRegistrar(gpu_ctx[0], CAM, max_requests=2, **caps)
    try:
        outs, raws, lists = _by_map(reg, dmap, [MM.scene_request(scene, mode), small_q])
        assert outs[0].status == REG_OVER_CAPACITY and outs[1].status == M.FEW_MATCHES_PASS1 and list(outs[1].kf_ids) == [MM.ROOT_ID, MM.OFFWALK_ID]
        res = np.frombuffer(raws[0][0], np.int32)
        assert res[0] == REG_OVER_CAPACITY and not res[1:].any()
        for blob in raws[0][1:] + lists[0][:2]:
            assert not np.frombuffer(blob, np.uint8).any()
        assert lists[0][2] == 0
        _, alone, alone_lists = _by_map(reg, dmap, [small_q])
        assert alone[0] == raws[1] and alone_lists[0] == lists[1]
    finally:
        reg.close()


def test_point_ids_at_the_edges_of_the_bitmap_words_and_of_the_compaction_block(gpu_ctx, registrar, device_scene, scene):
    """The source list is a bitmap over point ids, listed one trip per 512 words of 32 ids: the second trip starts at point id 16384.  The scene's first 33 points
    under ids on both sides of every word edge and of that block edge, in a map with room for 20 000 points: both modes against the stateless call, and a registrar
    whose source capacity ends inside the second trip (31 of 33: the entry of id 16384 is the last one written) is answered over capacity"""
    from scavislam_amd.ctypes_types import REG_OVER_CAPACITY
    from scavislam_amd.register import KeyframeRegistrar
    MAXP = 20000
    pt_ids = [0, 31, 32, 63, 64, 16383, 16384, 16385, MAXP - 1] + list(range(100, 124))
    ids = MM.scene_ids(scene)
    n = len(ids)
    model, dmap = MM.MapModel(), DeviceMap(gpu_ctx[0], device_scene, scene, max_keyframes=64, max_points=MAXP, max_observations=4096)
    small = None
    try:
        pts = np.array(scene["src"][:len(pt_ids)])
        pts["kf_index"] = [ids[int(e)] for e in pts["kf_index"]]
        op, ok = [], []
        for i, p in enumerate(pt_ids):
            for e in scene["obs_kf"][scene["obs_begin"][i]:scene["obs_begin"][i + 1]]:
                op.append(p); ok.append(ids[int(e)])
            op.append(p); ok.append(MM.ALL_ID)
        for m in (model, dmap):
            m.add_keyframes(ids + [MM.ALL_ID], [scene["kf_T"][e] for e in range(n)] + [scene["kf_T"][1]], entry=list(range(n)) + [1])
            m.add_points(pt_ids, pts)
            m.add_observations(op, ok)
            m.set_window([ids[e] for e in range(n) if int(scene["flags"][e]) & M.IN_WINDOW])
        qs = [MM.scene_request(scene, M.LOCAL), MM.scene_request(scene, M.LOOP)]
        for q in qs:                                                                     # every point is a source point of either request
            assert model.source_points(q["mode"], q["root_kf"], q["walk_kf"], q["direct_kf"]) == sorted(pt_ids)
        outs, _ = _check_against_stateless(registrar, device_scene, model, dmap, scene, qs)
        assert all(o.status != REG_OVER_CAPACITY for o in outs) and {16384, 16385, MAXP - 1} & set(int(p) for p in outs[0].point_ids)
        small = KeyframeRegistrar(gpu_ctx[0], CAM, max_requests=2, max_points=31, max_keyframes=8, max_observers=4096)
        outs, raws, lists = _by_map(small, dmap, qs)
        for i in range(2):
            res = np.frombuffer(raws[i][0], np.int32)
            assert outs[i].status == REG_OVER_CAPACITY and res[0] == REG_OVER_CAPACITY and not res[1:].any()
            for blob in raws[i][1:] + lists[i][:2]:
                assert not np.frombuffer(blob, np.uint8).any()
            assert lists[i][2] == 0
    finally:
        if small is not None:
            small.close()
        dmap.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_updates_and_requests_leave_the_map_as_it_was(gpu_ctx, registrar, device_scene, scene, both):
    from scavislam_amd.capi import SvsError
    model, dmap = both
    q = MM.scene_request(scene, M.LOCAL)
    _, before, before_lists = _by_map(registrar, dmap, [q])
    info = dmap.info()
    pt = np.array(scene["src"][:2])
    pt["kf_index"] = MM.ROOT_ID
    unknown_anchor = pt.copy(); unknown_anchor["kf_index"][1] = 9
    low = [scene["fast_thr"][0], scene["fast_thr"][1], np.full(4, 9)]
    invalid, capacity = "status 1", "status 4"
    cases = [(invalid, lambda: dmap.add_keyframes([MM.ROOT_ID], [M.I12], entry=[1])),                      # a keyframe already present
             (invalid, lambda: dmap.add_keyframes([60, 60], [M.I12, M.I12], entry=[1, 1])),                # an id twice in one call
             (invalid, lambda: dmap.add_keyframes([61], [M.I12], entry=[1], fast_thr=[low])),              # a threshold below 10
             (capacity, lambda: dmap.add_keyframes([62, MAP_CAPS["max_keyframes"]], [M.I12, M.I12], entry=[1, 1])),
             (invalid, lambda: dmap.add_points([1900, 1901], unknown_anchor)),                             # an anchor that is not in the map
             (invalid, lambda: dmap.add_points([1900, 1000], pt)),                                         # a point already present
             (capacity, lambda: dmap.add_points([1900, MAP_CAPS["max_points"]], pt)),
             (invalid, lambda: dmap.add_observations([1000, 1999], [MM.ROOT_ID, MM.ROOT_ID])),             # an unknown point
             (invalid, lambda: dmap.add_observations([1000, 1001], [MM.ROOT_ID, 9])),                      # an unknown keyframe
             (invalid, lambda: dmap.set_poses([MM.ROOT_ID, 9], [M.I12, M.I12])),
             (invalid, lambda: dmap.set_points([1000, 1999], np.zeros((2, 3)))),
             (invalid, lambda: dmap.set_window([MM.ROOT_ID, 9])),
             (invalid, lambda: registrar.register_map_batch(dmap.map, [dict(q, root_kf=9)])),
             (invalid, lambda: registrar.register_map_batch(dmap.map, [dict(q, walk_kf=q["walk_kf"] + [9])])),
             (invalid, lambda: registrar.register_map_batch(dmap.map, [dict(q, direct_kf=[MAP_CAPS["max_keyframes"] + 5])])),
             (capacity, lambda: registrar.register_map_batch(dmap.map, [q] * 9))]
    for code, call in cases:
        with pytest.raises(SvsError, match=code):
            call()
        assert dmap.info() == info
    tiny = DeviceMap(gpu_ctx[0], device_scene, scene, max_keyframes=4, max_points=4, max_observations=1)
    try:
        tiny.add_keyframes([0], [M.I12], entry=[1])
        pt["kf_index"] = 0
        tiny.add_points([1, 2], pt)
        with pytest.raises(SvsError, match=capacity):
            tiny.add_observations([1, 2, 1, 1], [0, 0, 0, 0])      # two distinct pairs, room for one
        assert tiny.info() == (1, 2, 0)
        tiny.add_observations([1, 1, 1], [0, 0, 0])
        assert tiny.info() == (1, 2, 1)
    finally:
        tiny.close()
    _, after, after_lists = _by_map(registrar, dmap, [q])
    assert after == before and after_lists == before_lists


# ---- 7. resources ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_map_gives_back_everything_it_held(gpu_ctx, registrar, device_scene, scene, few_ids, exit3_ids):
    ctx = gpu_ctx[0]
    names = ("live_device_bytes", "live_pinned_bytes", "live_sync_objects")
    before = [ctx.get_stat(n) for n in names]
    model, dmap = _fill_both(ctx, device_scene, scene, few_ids, exit3_ids)
    held = [ctx.get_stat(n) for n in names]
    registrar.register_map_batch(dmap.map, [MM.scene_request(scene, M.LOCAL)])
    dmap.close()
    assert held[0] > before[0] and held[1] > before[1] and held[2] == before[2] + 1
    assert [ctx.get_stat(n) for n in names] == before


# ---- 8. the C++ adaptor ------------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_adaptor_agrees_with_the_c_call(gpu_ctx, tmp_path):
    """tests/cpp/register_map_smoke.cpp: BackendMap and BackendRegistration::registerFrames of include/scavislam_hip.hpp against svs_map_* /
    svs_reg_register_map_batch called directly, and against the stateless adaptor call on the same scene"""
    exe = tmp_path / "register_map_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "register_map_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("REGISTER_MAP ")]
    assert tok and tok[0].split()[1] == "ok", out
    assert int(tok[0].split()[2]) >= 15 and int(tok[0].split()[3]) >= 15      # strength of the local neighbour, track points of the loop
