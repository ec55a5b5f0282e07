"""The keyframe decision on the device (svs_frontend_set_vertex_table + svs_frontend_decide_keyframes) against the reference's OWN keyframe logic, live: the 200-frame
sequence at 512 x 384 runs through the reference's loop with the one-call binding in place (oracle/_ref/libsvs_hipbranch_seq_onecall.so, as tests/test_gpu_sequence.py
runs it) -- shallWeSwitchKeyframe, shallWeDropNewKeyframe, addNewKeyframe and processMatchedPoints there are the reference's lines -- and every recorded call is
replayed through a second front end with the decision stage behind each step.  The vertex table of a frame is rebuilt from what the replay itself knows: the recorded
kept poses, the slot order, and the lists and strength_to_neighbors THIS stage produced at the earlier drops (the first keyframe's feature set is empty).

Bars.  Per frame, identical: dropped / switched, the keyframe switched to, n_new + n_track against the accepted lines the loop drew.  T_cur_after against the loop's
pose after its logic: the reference multiplies through its SE3 stand-in, the stage through pose.h's row sums, so a switch is not bit-equal by construction.
Measured on this run: the largest deviation over the 199 steps (6 drops, 5 switches) is 0.0 -- the stand-in forms the same row sums (profiles/keyframe_decide.md).
The bar is ten times the measured value, i.e. 0: every element equal; far below the 1e-9 seq_common.compare uses where both builds took the same steps.  The stage is read-only: every replayed step returns the bits the loop (which never ran the stage) consumed.  At the first drop the downloaded lists
go into svs_map_add_keyframe and the map must equal a twin built from lists the model made from svs_frontend_results."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_model as KM
import seq_common as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_BAR = 0.0      # ten times the largest deviation measured on this run (0.0); at most 1e-9
MAX_KEYFRAMES = 32


def _have(name):
    import oracle as O
    return os.path.exists(os.path.join(os.path.dirname(O.__file__), "_ref", name))


def _twin_maps_equal(ctx, oldkey, newkey, T_rel, lists_a, lists_b, cam):
    """svs_map_add_keyframe with the downloaded lists = the same call with the model's lists, read back"""
    import torch
    from scavislam_amd.ctypes_types import KEYFRAME_DTYPE
    from scavislam_amd.register import ResidentMap
    image = torch.zeros(256, dtype=torch.uint8, device="cuda")       # the map stores the frames' pointers and never follows them here
    kf = np.zeros(1, KEYFRAME_DTYPE)
    kf["pyr"], kf["stride"] = image.data_ptr(), 16
    back = []
    for new, track in (lists_a, lists_b):
        rm = ResidentMap(ctx, max_keyframes=4096, max_points=1 << 15, max_observations=1 << 16)      # (frame and point ids come from one counter)
        try:
            rm.reserve_edges(64)
            rm.add_first_keyframe(oldkey, kf, (image.data_ptr(), 4), [[25], [25], [25]])
            out = rm.add_keyframe(newkey, oldkey, T_rel, kf, (image.data_ptr(), 4), [[25], [25], [25]], new, track, 15, cam["w"] // 2, cam["h"] // 2)
            ids, meas, n = rm.get_feature_table(newkey)
            back.append((out["new_kept"].tobytes(), ids.tobytes(), meas.tobytes(), n, rm.get_points(new["point_id"]).tobytes(), rm.get_poses([newkey]).tobytes(), rm.info()))
        finally:
            rm.close()
    assert back[0] == back[1], "the map built from the downloaded lists differs from its twin"
    return back[0][3]


def test_every_decision_of_the_200_frame_sequence_equals_the_references(gpu_ctx):
    if not _have("libsvs_hipbranch_seq_onecall.so"):
        pytest.skip("oracle/_ref/libsvs_hipbranch_seq_onecall.so not present (built by oracle/Makefile where the reference lies; travels prebuilt)")
    import oracle as O
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import level_cams
    from scavislam_amd.frontend import StereoFrontend
    ctx, _ = gpu_ctx
    camname = "newcollege"
    cam = S.cam_of(camname)
    assert (cam["w"], cam["h"]) == (512, 384)
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    frames = list(S.frames(camname, S.N_FRAMES))
    seq = O.RefSequence(cams, hip_branch=True, one_call=True)
    loop, recs = [], []
    for img, disp in frames:
        loop.append(seq.step(img, disp))
        recs.append(seq.onecall_record())
    seq.close()
    assert all(r["ok"] for r in loop) and recs[0] is None and all(r is not None for r in recs[1:])

    fe = StereoFrontend(ctx, cam, max_points=16384, max_keyframes=MAX_KEYFRAMES, params=capi.FrontendParams.reference())
    fe.processFirstFrame(frames[0][0], disp=frames[0][1])
    # the vertex table as the replay knows it: creation order; the first keyframe has no features and no neighbours
    vertices = []                                                   # dicts: id, T, ids (feat_map keys), strength (keyframe ids)
    pending = dict(id=loop[0]["actkey_id"], ids=set(), strength=[])
    slot_kf = np.full(MAX_KEYFRAMES, -1, np.int32)
    act_id = loop[0]["actkey_id"]
    drops = switches = n_lists = 0
    worst = 0.0
    twin_pairs = None
    try:
        for k in range(1, S.N_FRAMES):
            rc, r = recs[k], loop[k]
            if rc["kept_slot"] >= 0:
                assert pending is not None
                fe.keepKeyframe(rc["kept_slot"], rc["kept_pose"])
                slot_kf[rc["kept_slot"]] = pending["id"]
                vertices.append(dict(pending, T=rc["kept_pose"].copy()))
                pending = None
            fe.setCandidateLists(rc["pts"], rc["group_end"])
            res, m, g = fe.processFrame(frames[k][0], rc["T_guess"], rc["T_act"], disp=frames[k][1])
            # read-only: the step behind a decide call returns what the loop, which never made one, consumed
            assert bytes(res.T_cur_from_actkey) == bytes(rc["res"].T_cur_from_actkey) and m.tobytes() == rc["matches"].tobytes(), f"frame {k}: the replayed step differs"
            index = {v["id"]: i for i, v in enumerate(vertices)}
            act = index[act_id]
            table = dict(stream=0, vertex_kf=[v["id"] for v in vertices], vertex_T=np.stack([v["T"] for v in vertices]), sets=[sorted(v["ids"]) for v in vertices], act=act,
                         neighbors=[index[i] for i in vertices[act]["strength"]], slot_kf=slot_kf)
            fe.setVertexTable([table])
            out = fe.decideKeyframes(want_lists=2)[0]
            d = out["dec"]
            assert d["valid"] == 1 and res.tracking_ok
            assert (d["decision"] == KM.KF_DROP, d["decision"] == KM.KF_SWITCH) == (r["dropped"], r["switched"]), f"frame {k}: decision {d['decision']}, the loop {r['dropped'], r['switched']}"
            accepted = sum(len(ln) for ln in r["lines"])
            assert d["n_new"] + d["n_track"] == accepted, f"frame {k}: {d['n_new']} + {d['n_track']} entries, {accepted} accepted lines"
            T_after = rc["recloud_pose"] if rc["recloud"] else r["T"].reshape(12)
            dev = float(np.abs(d["T_cur_after"] - T_after).max())
            worst = max(worst, dev)
            print(f"frame {k}: decision {d['decision']}, T_cur_after deviates {dev:.3e}")
            assert dev <= POSE_BAR, f"frame {k}: T_cur_after off by {dev}"
            # the stage's own lists against the model on the downloaded records
            want = KM.build_lists(m, rc["pts"], g, slot_kf)
            for a, b in zip((out["new"], out["track"], out["new_rec"], out["track_rec"]), want):
                assert a.tobytes() == b.tobytes(), f"frame {k}: lists differ from the model's"
            n_lists += len(want[0]) + len(want[1])
            if r["switched"]:
                assert d["closest_id"] == r["actkey_id"], f"frame {k}: switched to {d['closest_id']}, the loop to {r['actkey_id']}"
                act_id = r["actkey_id"]
                switches += 1
            if r["dropped"]:
                if drops == 0:
                    twin_pairs = _twin_maps_equal(ctx, act_id, r["actkey_id"], np.array(res.T_cur_from_actkey), (out["new"], out["track"]), want[:2], cam)
                pending = dict(id=r["actkey_id"], ids=set(int(i) for i in out["new"]["point_id"]) | set(int(i) for i in out["track"]["global_id"]),
                               strength=[int(i) for i in d["strength_kf"][:d["n_strength"]]])
                assert not d["over_capacity"] and np.abs(d["T_cur_after"] - np.array(KM.I12)).max() == 0
                act_id = r["actkey_id"]
                drops += 1
            if rc["recloud"]:
                fe.recomputeCloud(rc["recloud_pose"])
    finally:
        fe.close()
    assert drops >= 5 and switches >= 3, (drops, switches)
    assert twin_pairs is not None and twin_pairs > 0
    assert POSE_BAR <= 1e-9
    print(f"200 frames 512 x 384: {drops} drops, {switches} switches, every decision the reference's; {n_lists} list entries the model's; T_cur_after worst deviation "
          f"{worst:.3e} (bar {POSE_BAR:.1e}); the map of the first drop equals its twin ({twin_pairs} pairs in the new keyframe's table)")


def test_cpp_adaptor_decides_keyframes(gpu_ctx, tmp_path):
    """tests/cpp/keyframe_smoke.cpp: StereoFrontend::setVertexTable / decideKeyframes of include/scavislam_hip.hpp, compiled with g++ -std=c++11: the setter's
    refusals, no decision without a table, and the zeroed record of a step that matched nothing"""
    exe = tmp_path / "keyframe_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "keyframe_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.check_output([str(exe)]).decode()
    assert "KEYFRAME OK" in out, out
