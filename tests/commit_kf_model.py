"""The check stage of svs_map_add_keyframe_dev (map_addkf_dev.inc: map_addkf_check_kernel), twice.

  check_stage          the NumPy model of the kernel: whole-array operations and "least list index per point id" (np.minimum.at, the kernel's atomicMin), no loop
                       over entries and no arrival order.  Status, phase, first offending entry, the track flags and the id columns.
  host_restatement     what the host-list call decides about the same records, literally: addkf_check_lists and the loops in front of svs_map_add_keyframe's first
                       upload, entry by entry, returning at the first requirement that fails, with the map's sets as Python sets / dicts (hash containers).

tests/test_commit_kf_cpu.py holds the first to the second.  Only what the RECORDS decide is modelled: the refusals that need the arguments and the map's counts alone
come first in svs_map_add_keyframe_dev and are the same lines of host code in both calls (the header states the precedence).

A map here is a dict: max_pt, kf (set of keyframe ids), pt (set of point ids), pairs (set of (point, keyframe))."""
import numpy as np

OK, INVALID, CAPACITY = 0, 1, 4
PHASE_ANCHORS, PHASE_NEW, PHASE_TRACK, PHASE_OLDKEY = 1, 2, 3, 4
N_LEVELS, MAX_KF = 3, 16384
NONE = 0x7F7F7F7F


def check_stage(m, new, track, oldkey):
    """new: (point_id, anchor_id, anchor_level, feat_level) int arrays of equal length; track: (global_id, level).  -> dict(status, phase, index, flags, new_pid,
    new_anchor, track_gid)"""
    pid, anchor, la, lf = (np.asarray(a, np.int64) for a in new)
    gid, lvl = (np.asarray(a, np.int64) for a in track)
    max_pt = m["max_pt"]
    in_pt = np.zeros(max_pt, bool)
    in_pt[sorted(m["pt"])] = True
    in_kf = np.zeros(MAX_KF, bool)
    in_kf[sorted(m["kf"])] = True
    idx_new, idx_track = np.arange(len(pid)), np.arange(len(gid))
    out = dict(new_pid=pid.astype(np.int32), new_anchor=anchor.astype(np.int32), track_gid=gid.astype(np.int32))
    # the least list index of every new id inside the capacity
    first = np.full(max_pt, NONE, np.int64)
    new_in = (pid >= 0) & (pid < max_pt)
    np.minimum.at(first, pid[new_in], idx_new[new_in])
    # phase 1: anchors
    anchor_in = (anchor >= 0) & (anchor < MAX_KF)
    anchor_ok = anchor_in.copy()
    anchor_ok[anchor_in] = in_kf[anchor[anchor_in]]
    # phase 2: per entry the first rule it breaks
    code = np.zeros(len(pid), np.int64)
    known = np.zeros(len(pid), bool)
    known[new_in] = in_pt[pid[new_in]] | (first[pid[new_in]] < idx_new[new_in])
    bad_level = (la < 0) | (la >= N_LEVELS) | (lf < 0) | (lf >= N_LEVELS)
    code[bad_level] = INVALID
    code[known] = INVALID
    code[pid >= max_pt] = CAPACITY
    code[pid < 0] = INVALID
    # phase 3: track entries
    track_in = (gid >= 0) & (gid < max_pt)
    track_bad = (lvl < 0) | (lvl >= N_LEVELS)
    track_bad[track_in] |= first[gid[track_in]] != NONE
    # the flags: E, and the entry of least index per id of E
    in_e = np.zeros(len(gid), bool)
    in_e[track_in] = in_pt[gid[track_in]]
    first_t = np.full(max_pt, NONE, np.int64)
    np.minimum.at(first_t, gid[in_e], idx_track[in_e])
    flags = np.zeros(len(gid), np.int32)
    flags[in_e] = np.where(first_t[gid[in_e]] == idx_track[in_e], 3, 1)
    out["flags"] = flags
    # phase 4: oldkey a key of the table
    pair_keys = np.array(sorted(p * MAX_KF + k for p, k in m["pairs"]), np.int64)
    old_is_key = bool((anchor == oldkey).any()) or bool(np.isin(gid[in_e] * MAX_KF + oldkey, pair_keys).any())
    if not anchor_ok.all():
        out.update(status=INVALID, phase=PHASE_ANCHORS, index=int(np.argmin(anchor_ok)))
    elif code.any():
        i = int(np.argmax(code != 0))
        out.update(status=int(code[i]), phase=PHASE_NEW, index=i)
    elif track_bad.any():
        out.update(status=INVALID, phase=PHASE_TRACK, index=int(np.argmax(track_bad)))
    elif not old_is_key:
        out.update(status=INVALID, phase=PHASE_OLDKEY, index=-1)
    else:
        out.update(status=OK, phase=0, index=-1)
    return out


def host_restatement(m, new, track, oldkey, rng=None):
    """map_addkf.inc: addkf_check_lists, then the two loops and the oldkey requirement of svs_map_add_keyframe, as they stand.  The hash containers (the map's id
    sets, the set of pairs, `seen`) are rebuilt from their elements in an order shuffled by rng, so that nothing can lean on how one is walked"""
    def shuffled(items):
        items = list(items)
        if rng is not None:
            rng.shuffle(items)
        return items
    kf_in, pt_in, pairs = set(shuffled(m["kf"])), set(shuffled(m["pt"])), set(shuffled(m["pairs"]))
    max_pt = m["max_pt"]
    pid, anchor, la, lf = new
    gid, lvl = track
    n_new, n_track = len(pid), len(gid)

    def refused(status, phase, index):
        return dict(status=status, phase=phase, index=index)
    # addkf_check_lists
    for i in range(n_new):
        if not (0 <= anchor[i] < MAX_KF and int(anchor[i]) in kf_in):
            return refused(INVALID, PHASE_ANCHORS, i)
    flag = [0] * n_track
    seen = set()
    for i in range(n_track):
        g = int(gid[i])
        if g < 0 or g >= max_pt or g not in pt_in:
            continue
        if g in seen:
            flag[i] = 1
        else:
            seen.add(g)
            flag[i] = 3
        seen = set(shuffled(seen))
    # svs_map_add_keyframe, "every refusal": the stamp of the call
    old_is_key = False
    stamp = set()
    for i in range(n_new):
        p = int(pid[i])
        if not p >= 0:
            return refused(INVALID, PHASE_NEW, i)
        if not p < max_pt:
            return refused(CAPACITY, PHASE_NEW, i)
        if not (p not in pt_in and p not in stamp):
            return refused(INVALID, PHASE_NEW, i)
        stamp.add(p)
        if not (0 <= la[i] < N_LEVELS and 0 <= lf[i] < N_LEVELS):
            return refused(INVALID, PHASE_NEW, i)
        old_is_key |= int(anchor[i]) == oldkey
    for i in range(n_track):
        g = int(gid[i])
        if not 0 <= lvl[i] < N_LEVELS:
            return refused(INVALID, PHASE_TRACK, i)
        if not (g < 0 or g >= max_pt or g not in stamp):
            return refused(INVALID, PHASE_TRACK, i)
        if flag[i] & 1:
            old_is_key |= (g, oldkey) in pairs
    if not old_is_key:
        return refused(INVALID, PHASE_OLDKEY, -1)
    return dict(status=OK, phase=0, index=-1, flags=flag)


def random_case(rng, bad):
    """a small map and two lists with duplicates, foreign, negative and too large ids; bad: how many records are spoiled (0: mostly a call that passes)"""
    max_pt = int(rng.choice([64, 100, 257]))
    kfs = sorted(int(k) for k in rng.choice(np.r_[0:40, 8190:8194, 16380:16384], int(rng.integers(1, 9)), replace=False))
    pts = sorted(int(p) for p in rng.choice(max_pt, int(rng.integers(0, max_pt // 2)), replace=False))
    pairs = {(p, int(k)) for p in pts for k in rng.choice(kfs, int(rng.integers(0, min(3, len(kfs)) + 1)), replace=False)}
    m = dict(max_pt=max_pt, kf=set(kfs), pt=set(pts), pairs=pairs)
    oldkey = int(rng.choice(kfs))
    free = [p for p in range(max_pt) if p not in m["pt"]]
    n_new = int(rng.integers(0, min(len(free), 20) + 1))
    pid = rng.choice(free, n_new, replace=False).astype(np.int64) if n_new else np.zeros(0, np.int64)
    anchor = rng.choice(kfs + [oldkey] * 2, n_new).astype(np.int64)
    la, lf = rng.integers(0, N_LEVELS, n_new), rng.integers(0, N_LEVELS, n_new)
    n_track = int(rng.integers(0, 40))
    foreign = [-1, -7, -2 ** 31, max_pt, max_pt + 5, 2 ** 31 - 1] + [p for p in free if p not in set(pid.tolist())][:6]
    pool = (pts * 3 if pts else []) + foreign
    gid = rng.choice(pool, n_track).astype(np.int64)             # with replacement: ids twice and three times
    lvl = rng.integers(0, N_LEVELS, n_track)
    for _ in range(bad):
        kind = int(rng.integers(0, 9))
        if kind <= 4 and n_new:
            i = int(rng.integers(n_new))
            if kind == 0:
                anchor[i] = rng.choice([-1, MAX_KF, 2 ** 31 - 1, 41, 8195])
            elif kind == 1:
                pid[i] = rng.choice([-1, -2 ** 31, max_pt, 2 ** 31 - 1])
            elif kind == 2 and pts:
                pid[i] = rng.choice(pts)
            elif kind == 3:
                pid[i] = pid[int(rng.integers(n_new))]
            else:
                (la if rng.random() < 0.5 else lf)[i] = rng.choice([-1, N_LEVELS, 2 ** 31 - 1])
        elif kind <= 6 and n_track:
            i = int(rng.integers(n_track))
            if kind == 5:
                lvl[i] = rng.choice([-1, N_LEVELS])
            elif n_new:
                gid[i] = pid[int(rng.integers(n_new))]
        elif kind == 7:
            oldkey = int(rng.choice(kfs))
            anchor[anchor == oldkey] = kfs[0]
            if kfs[0] == oldkey:
                n_new, pid, anchor, la, lf = 0, pid[:0], anchor[:0], la[:0], lf[:0]
    return m, (pid, anchor, la, lf), (gid, lvl), oldkey


def map_bytes(d, kfs, pts):
    """every read-back of a ResidentMap the GPU tests compare, as bytes: the counts, the edge records in slot order, the poses of kfs, the records of pts, the
    binding's edge mirrors, and the feature_table of every keyframe of kfs"""
    edges = [(a, b) for a, b, _ in d.edge_log]
    out = [repr((d.info(), d.edge_info(), d.measured_info())).encode(), d.get_edges(edges).tobytes() if edges else b"", d.get_poses(kfs).tobytes(),
           d.get_points(pts).tobytes() if len(pts) else b"", repr((sorted(d.edge_keys), d.edge_log)).encode()]
    for k in kfs:
        ids, rec, n = d.get_feature_table(k)
        out += [ids.tobytes(), rec.tobytes(), repr(n).encode()]
    return out


def keyframe_bytes(d, kf_id):
    """what the map stores of a keyframe beside its pose: pyramid pointers and strides, the disparity's address and stride, the thresholds"""
    kf, disp, thr = d.get_keyframe(kf_id)
    return repr(([int(p) for p in kf["pyr"]], [int(s) for s in kf["stride"]], disp)).encode(), thr.tobytes()
