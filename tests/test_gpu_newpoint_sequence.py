"""The resident newpoint_map against the reference's OWN map, live: the 200-frame sequence at 512 x 384 runs through the reference's loop with the one-call binding in
place (oracle/_ref/libsvs_hipbranch_seq_onecall.so, as tests/test_gpu_keyframe_sequence.py runs it) -- newpoint_map there is the reference's, seeded at :808, pruned
at :360-365, walked at :989-1029 -- and every recorded call is replayed through a second front end whose lists take their head from the store:
  * the records of a recorded group that the store has never held (the first time a key shows up with a non-empty group; points added to a keyframe later) are put
    from the record -- the reference's seeding order comes from third-party sampling and cannot be regenerated; they must be a PREFIX of the group (push_front);
  * behind every drop the store is pruned from the replayed step's own device records;
  * every frame's list is composed by svs_frontend_set_candidates_from_newpoints from the keys of the recorded groups and the recorded tail.
The key of a recorded group is the keyframe its records are anchored in (a new point of list k is anchored in keyframe k): the id kept in the slot their kf_index
names.  An empty recorded group is named by a key the store does not hold.

Bars.  The composed list is byte-equal to the recorded pts / group_end on every frame -- so what the prune removed is what the reference's remove_if removed, in every
list, stably; every replayed step returns the recorded pose and match bytes; n_removed at a drop = the accepted new matches of that frame.  Conditions on the run: at
least 5 drops and 3 switches, and at least one group handed over again after a prune had taken records from it."""
import os

import numpy as np
import pytest

import seq_common as S

pytestmark = pytest.mark.gpu
MAX_KEYFRAMES = 32


def _have(name):
    import oracle as O
    return os.path.exists(os.path.join(os.path.dirname(O.__file__), "_ref", name))


def test_the_store_replays_the_references_newpoint_map_over_200_frames(gpu_ctx):
    if not _have("libsvs_hipbranch_seq_onecall.so"):
        pytest.skip("oracle/_ref/libsvs_hipbranch_seq_onecall.so not present (built by oracle/Makefile where the reference lies; travels prebuilt)")
    import oracle as O
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import MATCH_OK, level_cams
    from scavislam_amd.frontend import StereoFrontend
    ctx, _ = gpu_ctx
    camname = "newcollege"
    cam = S.cam_of(camname)
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
    fe.reserveNewpoints(16384, 64)
    fe.processFirstFrame(frames[0][0], disp=frames[0][1])
    slot_kf = np.full(MAX_KEYFRAMES, -1, np.int32)
    pending_id = loop[0]["actkey_id"]
    ever = {}                                                       # key -> every point id the store was ever given for it
    shrunk = set()                                                  # keys a prune has taken records from
    drops = switches = n_put = n_pruned = handed_again = 0
    try:
        for k in range(1, S.N_FRAMES):
            rc, r = recs[k], loop[k]
            if rc["kept_slot"] >= 0:
                fe.keepKeyframe(rc["kept_slot"], rc["kept_pose"])
                slot_kf[rc["kept_slot"]] = pending_id
            pts, ge = rc["pts"], [int(e) for e in rc["group_end"]]
            keys, puts, again = [], [], False
            for g in range(len(ge) - 1):
                grp = pts[(ge[g - 1] if g else 0):ge[g]]
                if len(grp) == 0:
                    keys.append(10 ** 6 + g)                        # an absent key: an empty group
                    continue
                slot = int(grp["kf_index"][0])
                assert slot >= 0 and (grp["kf_index"] == slot).all() and slot_kf[slot] >= 0, f"frame {k} group {g}: one anchor keyframe per list, kept in a slot"
                key = int(slot_kf[slot])
                keys.append(key)
                fresh = ~np.isin(grp["point_id"], sorted(ever.setdefault(key, set())))
                if fresh.any():
                    m = int(fresh.sum())
                    assert fresh[:m].all(), f"frame {k} group {g}: the points new to list {key} are not at its front"
                    puts.append(dict(stream=0, kf_id=key, records=grp[:m]))
                    ever[key] |= set(int(i) for i in grp["point_id"][:m])
                    n_put += m
                again = again or key in shrunk
            if puts:
                fe.putNewpoints(puts)
            handed_again += int(again)
            out = fe.setCandidatesFromNewpoints([dict(stream=0, keys=keys, slot_kf=slot_kf, tail=pts[ge[-2]:])], want_records=True)[0]
            assert not out["over_capacity"] and out["n_points"] == len(pts) and out["n_head"] == ge[-2] and out["n_no_slot"] == 0
            assert out["table"][0, :len(pts)].tobytes() == pts.tobytes(), f"frame {k}: the list composed from the store differs from the recorded one"
            assert out["group_end"][0, :len(ge)].tolist() == ge, f"frame {k}: group ends {out['group_end'][0, :len(ge)]} vs the recorded {ge}"
            res, m, g = fe.processFrame(frames[k][0], rc["T_guess"], rc["T_act"], disp=frames[k][1])
            assert bytes(res.T_cur_from_actkey) == bytes(rc["res"].T_cur_from_actkey) and m.tobytes() == rc["matches"].tobytes(), f"frame {k}: the replayed step differs"
            if r["switched"]:
                switches += 1
            if r["dropped"]:
                n_new = int(((m["status"][:ge[-2]] == MATCH_OK) & (g["accepted"][:ge[-2]] != 0)).sum())
                before = fe.newpoints(want_records=False)[0]
                n_removed, counts = fe.pruneNewpoints([0])[0]
                assert n_removed == n_new, f"frame {k}: the prune removed {n_removed}, the frame matched {n_new} new points"
                shrunk |= set(int(key) for key, a, b in zip(before["keys"], before["counts"], counts) if b < a)
                n_pruned += n_removed
                pending_id = r["actkey_id"]
                drops += 1
            if rc["recloud"]:
                fe.recomputeCloud(rc["recloud_pose"])
    finally:
        fe.close()
    print(f"200 frames 512 x 384: {drops} drops, {switches} switches; {n_put} records put into {len(ever)} groups, {n_pruned} pruned; every list composed from the store is "
          f"the recorded one; {handed_again} lists held a group a prune had shrunk")
    assert drops >= 5 and switches >= 3, (drops, switches)
    assert n_pruned > 0 and handed_again >= 1
