"""Host-side mirror of the back end's re-registration of a keyframe against the map.

  KeyframeRegistrar.local_register(requests)  <- Backend::localRegisterFrame   backend.cpp:549-611 (pointsVisibleInRoot :472-546, matchAndAlign :725-784,
                                                                               keyframesToRegister :615-722)
  KeyframeRegistrar.loop_closure(requests)    <- Backend::globalLoopClosure    backend.cpp:830-1001

A request of the stateless calls is one root keyframe with the candidate map points the caller's graph walk found (framesInNeighborhood, the hash-set deduplication,
registerKeyframes / addLoopClosure stay with that caller; on a ResidentMap they are frames_in_neighborhood, register_map_batch and commit).  A batch of requests is
ONE library call: one staged upload, one chain of launches, one download.  There is no CPU path: every call goes to svs_reg_* of the HIP library.

  ResidentMap                                  the map on the device (svs_map_*): keyframes, points and feature_table pairs under the graph's ids, updated incrementally
  KeyframeRegistrar.register_map_batch(map, requests)   the same registration with a request named by ids: the point walk of pointsVisibleInRoot runs on the device
  KeyframeRegistrar.commit(map, i)             registerKeyframes / addLoopClosure for request i of that batch, from the lists the registration left on the device
  ResidentMap.register_keyframes / add_loop_closure     the same two functions with the caller's own lists
"""
import ctypes as C

import numpy as np

from .ctypes_types import (BA_CONSTRAINT_DTYPE, BA_EDGE_DTYPE, CANDIDATE_DTYPE, CONS_OK, KEYFRAME_DTYPE, MAP_ADDKF_MAX_NEIGHBORS, MAP_CONS_MAX_REQUESTS, MAP_CONSTRAINT_RESULT_DTYPE, MAP_EDGE_DTYPE, MAP_KEY_DTYPE, MAP_NEW_POINT_DTYPE, MAP_TRACK_POINT_DTYPE, MAP_WALK_MAX_REQUESTS, MAP_WINDOW_MAX, MATCH_RESULT_DTYPE, REG_KF_STATS_DTYPE, REG_LOCAL, REG_LOOP, REG_OK, REG_OVER_CAPACITY,
                           REG_STAGES, SVS_MAX_CELLS, WALK_OK, Cam, MapAddKeyframeArgs, MapConstraintRequest, MapStrengthResult, MapWindowResult, RegCommitResult, RegMapRequest, RegParams, RegRequest, RegResult)


def keyframe_table(entries):
    """entries: (device pointers of the u8 pyramid [3], strides [3], T_anchor_from_w [12]) per keyframe -> KEYFRAME_DTYPE array"""
    kfs = np.zeros(len(entries), KEYFRAME_DTYPE)
    for i, (ptrs, strides, T) in enumerate(entries):
        kfs[i]["T_anchor_from_w"] = np.asarray(T, np.float64).reshape(12)
        kfs[i]["pyr"] = [int(p) for p in ptrs]
        kfs[i]["stride"] = [int(s) for s in strides]
    return kfs


class RegistrationOutput:
    """One request's outputs, cut to its n_candidates / n_kf."""

    def __init__(self, res, cand_src, matches, status_pass1, accepted, kf_stats, matches_pass1):
        for f in ("status", "n_candidates", "n_obs_pass1", "n_obs_pass2", "n_accepted", "n_qualified"):
            setattr(self, f, int(getattr(res, f)))
        self.T_newroot_from_oldroot = np.array(res.T_newroot_from_oldroot, np.float64).reshape(3, 4)
        self.T_pass1 = np.array(res.T_pass1, np.float64).reshape(3, 4)
        self.stats_pass1, self.stats_pass2 = res.stats_pass1, res.stats_pass2
        self.cand_src, self.matches, self.status_pass1, self.accepted, self.kf_stats, self.matches_pass1 = cand_src, matches, status_pass1, accepted, kf_stats, matches_pass1

    def ok(self):
        """what localRegisterFrame / globalLoopClosure return"""
        return self.status == REG_OK

    def neighborid_to_strength(self):
        """{keyframe-table entry: strength} of the keyframes that qualify (backend.cpp:707-713); loop mode: {0: strength} of the frame as a whole"""
        q = np.nonzero(self.kf_stats["qualifies"])[0]
        return {int(k): int(self.kf_stats["strength"][k]) for k in q}

    def track_points(self, src):
        """(point_id, uvu, anchor_level) of the accepted observations, in candidate order: the MyTrackPoint data of :663-667 / :945-950"""
        a = np.nonzero(self.accepted)[0]
        s = np.asarray(src)[self.cand_src[a]]
        return s["point_id"].copy(), self.matches["obs"][a].copy(), s["anchor_level"].copy()


class KeyframeRegistrar:
    def __init__(self, ctx, cam, max_requests=8, max_points=4096, max_keyframes=64, max_observers=None, params=None):
        self.ctx, self.h = ctx, None
        self.cam = cam if isinstance(cam, Cam) else Cam(cam["f"], cam["cx"], cam["cy"], cam["b"], int(cam["w"]), int(cam["h"]))
        self.max_requests, self.max_points, self.max_keyframes = int(max_requests), int(max_points), int(max_keyframes)
        self.max_observers = int(max_observers if max_observers is not None else 4 * max_points)
        self.params = params or RegParams.reference()
        h = C.c_void_p()
        ctx.call("svs_reg_create", C.byref(self.cam), self.max_requests, self.max_points, self.max_keyframes, self.max_observers, C.byref(h))
        self.h = h
        ctx.children.add(self)
        self.raw = None      # the full-length rows of the last call (tests: byte comparisons)
        self.commit_raw = None   # the arrays of the last commit as the library wrote them

    def _request(self, q, mode, keep):
        r = RegRequest()
        kfs = np.ascontiguousarray(q["kfs"], KEYFRAME_DTYPE)
        flags = np.ascontiguousarray(q["flags"], np.uint8)
        src = np.ascontiguousarray(q["src"], CANDIDATE_DTYPE)
        if len(flags) != len(kfs):
            raise ValueError("one flag byte per keyframe-table entry expected")
        keep += [kfs, flags, src]
        r.mode, r.n_kf, r.n_src, r.root_kf = mode, len(kfs), len(src), int(q["root_kf"])
        r.d_root_disp, r.root_disp_stride = int(q["root_disp"][0]), int(q["root_disp"][1])
        for l in range(3):
            t = np.asarray(q["fast_thr"][l], np.int32).reshape(-1)
            if len(t) > SVS_MAX_CELLS:
                raise ValueError("at most SVS_MAX_CELLS thresholds per level")
            for c in range(SVS_MAX_CELLS):
                r.fast_thr[l][c] = int(t[c]) if c < len(t) else 25
        T = np.asarray(q["T_root_from_world"], np.float64).reshape(12)
        for k in range(12):
            r.T_root_from_world[k] = float(T[k])
        r.h_kfs, r.h_kf_flags, r.h_src = kfs.ctypes.data, flags.ctypes.data, src.ctypes.data if len(src) else None
        if mode == REG_LOCAL:
            ob = np.ascontiguousarray(q["obs_begin"], np.int32)
            ok = np.ascontiguousarray(q["obs_kf"], np.int32)
            if len(ob) != len(src) + 1:
                raise ValueError("obs_begin must have n_src + 1 entries")
            keep += [ob, ok]
            r.h_obs_begin, r.h_obs_kf = ob.ctypes.data, ok.ctypes.data if len(ok) else None
        return r

    def register_batch(self, requests, modes, params=None, want_pass1=False):
        """requests: dicts with kfs (KEYFRAME_DTYPE, see keyframe_table), flags (REG_KF_* bits per entry), root_kf, root_disp (device pointer, stride), fast_thr
        (per level the stored thresholds), T_root_from_world, src (CANDIDATE_DTYPE, kf_index = table entry of the anchor) and, local mode, obs_begin / obs_kf"""
        n = len(requests)
        keep = []
        arr = (RegRequest * max(n, 1))()
        for i, (q, m) in enumerate(zip(requests, modes)):
            arr[i] = self._request(q, m, keep)
        prm = params or self.params
        res = (RegResult * max(n, 1))()
        MP, MK = self.max_points, self.max_keyframes
        csrc = np.empty((n, MP), np.int32)
        m2 = np.empty((n, MP), MATCH_RESULT_DTYPE)
        st1 = np.empty((n, MP), np.int32)
        acc = np.empty((n, MP), np.int32)
        kfst = np.empty((n, MK), REG_KF_STATS_DTYPE)
        m1 = np.empty((n, MP), MATCH_RESULT_DTYPE) if want_pass1 else None
        self.ctx.check(self.ctx.lib.svs_reg_register_batch(self.h, n, arr, C.byref(prm), res, csrc.ctypes.data, m2.ctypes.data, st1.ctypes.data, acc.ctypes.data,
                                                           kfst.ctypes.data, m1.ctypes.data if want_pass1 else None))
        self.raw = dict(results=bytes(res)[:n * C.sizeof(RegResult)], cand_src=csrc, matches=m2, status_pass1=st1, accepted=acc, kf_stats=kfst, matches_pass1=m1)
        out = []
        for i in range(n):
            k, nk = res[i].n_candidates, arr[i].n_kf
            out.append(RegistrationOutput(res[i], csrc[i, :k], m2[i, :k], st1[i, :k], acc[i, :k], kfst[i, :nk], m1[i, :k] if want_pass1 else None))
        return out

    def register_map_batch(self, resident_map, requests, params=None, want_pass1=False):
        """requests: dicts with mode, root_kf (id), T_root_from_world, walk_kf (ids: framesInNeighborhood(root) / [the query keyframe]) and direct_kf (ids:
        directNeighborsOf(root)).  The outputs are those of register_batch on the request the map's walk builds; each carries point_ids (per candidate) and
        kf_ids (per table entry).  A request whose built tables exceed this registrar's capacities comes back with status REG_OVER_CAPACITY and empty rows"""
        n = len(requests)
        keep = []
        arr = (RegMapRequest * max(n, 1))()
        for i, q in enumerate(requests):
            walk = np.ascontiguousarray(q["walk_kf"], np.int32).reshape(-1)
            direct = np.ascontiguousarray(q.get("direct_kf", ()), np.int32).reshape(-1)
            keep += [walk, direct]
            r = arr[i]
            r.mode, r.root_kf, r.n_walk, r.n_direct = int(q["mode"]), int(q["root_kf"]), len(walk), len(direct)
            T = np.asarray(q["T_root_from_world"], np.float64).reshape(12)
            for k in range(12):
                r.T_root_from_world[k] = float(T[k])
            r.h_walk_kf, r.h_direct_kf = walk.ctypes.data if len(walk) else None, direct.ctypes.data if len(direct) else None
        prm = params or self.params
        res = (RegResult * max(n, 1))()
        MP, MK = self.max_points, self.max_keyframes
        csrc = np.empty((n, MP), np.int32)
        m2 = np.empty((n, MP), MATCH_RESULT_DTYPE)
        st1 = np.empty((n, MP), np.int32)
        acc = np.empty((n, MP), np.int32)
        kfst = np.empty((n, MK), REG_KF_STATS_DTYPE)
        m1 = np.empty((n, MP), MATCH_RESULT_DTYPE) if want_pass1 else None
        pid = np.empty((n, MP), np.int32)
        kfid = np.empty((n, MK), np.int32)
        nkf = np.empty(n, np.int32)
        self.ctx.check(self.ctx.lib.svs_reg_register_map_batch(self.h, resident_map.h, n, arr, C.byref(prm), res, csrc.ctypes.data, m2.ctypes.data, st1.ctypes.data,
                                                               acc.ctypes.data, kfst.ctypes.data, m1.ctypes.data if want_pass1 else None, pid.ctypes.data,
                                                               kfid.ctypes.data, nkf.ctypes.data))
        self.raw = dict(results=bytes(res)[:n * C.sizeof(RegResult)], cand_src=csrc, matches=m2, status_pass1=st1, accepted=acc, kf_stats=kfst, matches_pass1=m1,
                        point_ids=pid, kf_ids=kfid, n_kf=nkf)
        out = []
        for i in range(n):
            k, nk = res[i].n_candidates, int(nkf[i])
            o = RegistrationOutput(res[i], csrc[i, :k], m2[i, :k], st1[i, :k], acc[i, :k], kfst[i, :nk], m1[i, :k] if want_pass1 else None)
            o.point_ids, o.kf_ids = pid[i, :k], kfid[i, :nk]
            out.append(o)
        return out

    def local_register(self, requests, **kw):
        return self.register_batch(requests, [REG_LOCAL] * len(requests), **kw)

    def loop_closure(self, requests, **kw):
        return self.register_batch(requests, [REG_LOOP] * len(requests), **kw)

    def commit(self, resident_map, index, cached=None, missing_cap=16, resolve_missing=True):
        """registerKeyframes / addLoopClosure for request `index` of the last register_map_batch on resident_map, with the lists taken where the registration left
        them on the device (svs_reg_commit).  Returns a dict: committed (False: the request's status was not REG_OK, the map is unchanged), mode, root_id (the
        keyframe that took the pairs), other_id (loop mode: the query keyframe), T_new [12], track_point_ids, track_added, n_pairs_added, edges [(kf1, kf2) as
        computeConstraint took them], edge_strength, edge_results (as compute_constraints returns them) and missing.  resolve_missing=True completes the edges that
        lacked an anchor through absolute_poses and a storing compute_constraints, as ResidentMap.add_keyframe does"""
        cids, cT = _cached_arrays(cached)
        MK, MP, cap = self.max_keyframes, max(self.max_points, 1), int(missing_cap)
        res = RegCommitResult()
        ekf, est = np.full(MK, -1, np.int32), np.zeros(MK, np.int32)
        cons = np.zeros(MK, MAP_CONSTRAINT_RESULT_DTYPE)
        missing = np.full((MK, cap), -1, np.int32)
        tid, tadd = np.full(MP, -1, np.int32), np.zeros(MP, np.int32)
        self.ctx.check(self.ctx.lib.svs_reg_commit(self.h, resident_map.h, int(index), len(cids), cids.ctypes.data if len(cids) else None,
                                                   cT.ctypes.data if len(cids) else None, cap, C.byref(res), ekf.ctypes.data, est.ctypes.data, cons.ctypes.data,
                                                   missing.ctypes.data if cap else None, MP, tid.ctypes.data, tadd.ctypes.data))
        self.commit_raw = dict(result=bytes(res), edge_kf=ekf, edge_strength=est, results=cons, missing=missing, track_point_ids=tid, track_added=tadd)
        return resident_map._commit_out(res, ekf, est, cons, missing, tid[:res.n_track].copy(), tadd[:res.n_track].astype(bool), cached, cap, resolve_missing)

    def set_timing(self, on=True):
        self.ctx.check(self.ctx.lib.svs_reg_set_timing(self.h, int(on)))

    def stage_times_ms(self):
        """(cull, FAST, match 1, refinement 1, match 2, refinement 2, gate) of the last call, from events; zeros unless set_timing(True)"""
        ms = (C.c_float * REG_STAGES)()
        self.ctx.check(self.ctx.lib.svs_reg_stage_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def close(self):
        if self.h:
            self.ctx.lib.svs_reg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _cached_arrays(cached):
    """{anchor id: T[12]} -> (ids ascending, T [n, 12]) as the library takes a cached list"""
    cached = cached or {}
    ids = np.array(sorted(int(c) for c in cached), np.int32)
    T = np.ascontiguousarray([np.asarray(cached[int(c)], np.float64).reshape(12) for c in ids], np.float64).reshape(len(ids), 12)
    return ids, T


def _inner_pairs_with_edge(window, edge_keys):
    ids, types = window
    inner = sorted(int(k) for k, t in zip(ids, types) if int(t) == 0)
    return [(a, b) for i, a in enumerate(inner) for b in inner[i + 1:] if (a, b) in edge_keys]


def entering_inner_pairs(new_window, edge_keys):
    """unmargPosesEnteringInnerW (slam_graph.cpp:728-759): every edge between two INNER keyframes of the window, once, as (lo, hi) ascending"""
    return _inner_pairs_with_edge(new_window, edge_keys)


def left_inner_pairs(old_window, new_window, edge_keys):
    """margPosesLeftInnerWindow (:848-904): every edge between two INNER keyframes of the old window of which at least one is not INNER now, once, as (lo, hi)
    ascending.  The reference computes both orientations and keeps the one its hash order visits last; here kf1 is the smaller id"""
    inner_now = {int(k) for k, t in zip(*new_window) if int(t) == 0}
    return [(a, b) for a, b in _inner_pairs_with_edge(old_window, edge_keys) if a not in inner_now or b not in inner_now]


class ResidentMap:
    """svs_map: the back end's map in device memory, under the graph's own ids (dense, below the capacities).  Every update is one staged upload, asynchronous
    on the context's stream, and is refused as a whole (SvsError, the map unchanged) on an unknown, repeated or out-of-range id."""

    def __init__(self, ctx, max_keyframes=1024, max_points=1 << 16, max_observations=1 << 19):
        self.ctx, self.h = ctx, None
        h = C.c_void_p()
        ctx.call("svs_map_create", int(max_keyframes), int(max_points), int(max_observations), C.byref(h))
        self.h = h
        self.window_shape = None
        self.edge_keys = set()               # (lo, hi) of every edge: what update_marginalization selects its pairs from
        self.edge_log = []                   # (a, b, strength) in slot order: what neighbors_of_root orders the root's row by
        ctx.children.add(self)

    def _call(self, name, *args):
        self.ctx.check(getattr(self.ctx.lib, name)(self.h, *args))

    def add_keyframes(self, ids, kfs, disp, fast_thr):
        """kfs: KEYFRAME_DTYPE (see keyframe_table: T_me_from_world, pyramid device pointers and strides); disp: (device pointer, stride) of the level-0 f32
        disparity per keyframe; fast_thr: per keyframe, per level, the stored thresholds (cells beyond a level's grid are filled with 25)"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        kfs = np.ascontiguousarray(kfs, KEYFRAME_DTYPE).reshape(-1)
        n = len(ids)
        if not (len(kfs) == len(disp) == len(fast_thr) == n):
            raise ValueError("one keyframe record, disparity and threshold set per id expected")
        ptr = np.array([int(d[0]) for d in disp], np.uint64)
        stride = np.array([int(d[1]) for d in disp], np.int32)
        thr = np.full((n, 3, SVS_MAX_CELLS), 25, np.int32)
        for i, per_level in enumerate(fast_thr):
            for l in range(3):
                t = np.asarray(per_level[l], np.int32).reshape(-1)
                if len(t) > SVS_MAX_CELLS:
                    raise ValueError("at most SVS_MAX_CELLS thresholds per level")
                thr[i, l, :len(t)] = t
        self._call("svs_map_add_keyframes", n, ids.ctypes.data, kfs.ctypes.data, ptr.ctypes.data, stride.ctypes.data, thr.ctypes.data)

    def add_points(self, ids, points):
        """points: CANDIDATE_DTYPE with kf_index = the ID of the anchor keyframe"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        pts = np.ascontiguousarray(points, CANDIDATE_DTYPE).reshape(-1)
        if len(pts) != len(ids):
            raise ValueError("one point record per id expected")
        self._call("svs_map_add_points", len(ids), ids.ctypes.data, pts.ctypes.data)

    def add_observations(self, point_ids, kf_ids):
        """point point_ids[i] is in the feature_table of keyframe kf_ids[i]; pairs already present are ignored"""
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        if len(p) != len(k):
            raise ValueError("pairs expected")
        self._call("svs_map_add_observations", len(p), p.ctypes.data, k.ctypes.data)

    def add_measured_observations(self, point_ids, kf_ids, center, level):
        """add_observations for a caller that also optimises: every new pair brings feat.center [3] and feat.level (0 .. 2); the map keeps one BA observation
        record per new pair on the device (svs_map_add_measured_observations)"""
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        c = np.ascontiguousarray(center, np.float64).reshape(-1, 3)
        l = np.ascontiguousarray(level, np.int32).reshape(-1)
        if not (len(p) == len(k) == len(c) == len(l)):
            raise ValueError("one keyframe, centre and level per point expected")
        self._call("svs_map_add_measured_observations", len(p), p.ctypes.data, k.ctypes.data, c.ctypes.data, l.ctypes.data)

    def measured_info(self):
        """(pairs with a measurement, pairs without one)"""
        a, b = C.c_int32(), C.c_int32()
        self._call("svs_map_measured_info", C.byref(a), C.byref(b))
        return a.value, b.value

    def prepare_window(self, kf_ids, kf_type, edge_pairs=(), set_window_flags=True, window_cap=MAP_WINDOW_MAX):
        """computeActivePointsAndExtendOuterWindow on the device (svs_map_prepare_window): kf_ids / kf_type (0 INNER, 1 OUTER) are double_window_ before the
        extension, edge_pairs [n, 2] the edge_table_ entries with an end in an INNER keyframe.  Returns (MapWindowResult, final window ids, types); the two
        arrays are empty and n_active is -1 when the final window exceeds window_cap"""
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        t = np.ascontiguousarray(kf_type, np.int32).reshape(-1)
        e = np.ascontiguousarray(edge_pairs, np.int32).reshape(-1, 2)
        if len(k) != len(t):
            raise ValueError("one type per keyframe expected")
        cap = int(window_cap)
        res = MapWindowResult()
        wid, wtype = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), -1, np.int32)
        self._call("svs_map_prepare_window", len(k), k.ctypes.data, t.ctypes.data, len(e), e.ctypes.data if len(e) else None, int(bool(set_window_flags)), cap,
                   C.byref(res), wid.ctypes.data, wtype.ctypes.data)
        n = res.n_window if res.n_active >= 0 else 0
        self.window_shape = (res.n_window, res.n_active) if res.n_active >= 0 else None      # what SlamGraphOptimizer.windowFromMap sizes its state by
        return res, wid[:n].copy(), wtype[:n].copy()

    def set_poses(self, kf_ids, poses):
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        T = np.ascontiguousarray(poses, np.float64).reshape(len(k), 12)
        self._call("svs_map_set_poses", len(k), k.ctypes.data, T.ctypes.data)

    def set_points(self, point_ids, xyz_anchor):
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        x = np.ascontiguousarray(xyz_anchor, np.float64).reshape(len(p), 3)
        self._call("svs_map_set_points", len(p), p.ctypes.data, x.ctypes.data)

    def set_window(self, kf_ids):
        """graph_.double_window(): exactly these keyframes are in the window afterwards"""
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        self._call("svs_map_set_window", len(k), k.ctypes.data)

    # ---- the pose graph's edges (EdgeTable, slam_graph.hpp:197-363) and their constraints (computeConstraint, slam_graph.cpp:787-846)
    def reserve_edges(self, max_edges):
        """room for the edge table (once); without it every edge call is refused"""
        self._call("svs_map_reserve_edges", int(max_edges))

    def add_edges(self, pairs, strength, edge_type):
        """insertEdge for pairs [n, 2] (either orientation); a new edge is not marginalised"""
        e = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(strength, np.int32), (len(e),)))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(edge_type, np.int32), (len(e),)))
        self._call("svs_map_add_edges", len(e), e.ctypes.data, s.ctypes.data, t.ctypes.data)
        self.edge_keys.update((int(min(a, b)), int(max(a, b))) for a, b in e)
        self.edge_log += [(int(a), int(b), int(st)) for (a, b), st in zip(e, s)]

    def set_constraints(self, cons):
        """setConstraint with the caller's values: BA_CONSTRAINT_DTYPE, pose1 / pose2 name the edge, T_21 = T_pose2_from_pose1; marks the edges marginalised"""
        c = np.ascontiguousarray(cons, BA_CONSTRAINT_DTYPE).reshape(-1)
        self._call("svs_map_set_constraints", len(c), c.ctypes.data)

    def unmarginalize(self, pairs):
        """unMarginalize: clears the flag only"""
        e = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self._call("svs_map_unmarginalize", len(e), e.ctypes.data)

    def get_edges(self, pairs):
        """blocking read-back of the records (MAP_EDGE_DTYPE: T_lo_from_hi, ONE info for both directions)"""
        e = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros(len(e), MAP_EDGE_DTYPE)
        self._call("svs_map_get_edges", len(e), e.ctypes.data, out.ctypes.data)
        return out

    def edge_info(self):
        """(edges, marginalised edges): the host-side counts"""
        a, b = C.c_int32(), C.c_int32()
        self._call("svs_map_edge_info", C.byref(a), C.byref(b))
        return a.value, b.value

    def compute_constraints(self, requests, missing_cap=16, depth_cap=0):
        """svs_map_compute_constraints: computeConstraint for a batch, one blocking call.  A request is a dict: kf1, kf2, store (False), overrides ([(id, T[12])], at
        most two: the request's pose of that keyframe, also as an anchor), cached ({anchor id: T_anchor_from_world[12]}: the caller's computeAbsolutePose results).
        Returns one dict per request: status (CONS_OK / CONS_EMPTY / CONS_MISSING_ANCHOR), strength, median, norm_dist, T_12 [12], info [36], n_missing, missing
        (ascending ids, at most missing_cap) and, with depth_cap > 0, depths (ascending point id).  self.raw keeps the three arrays as the library wrote them"""
        n = len(requests)
        arr = (MapConstraintRequest * max(n, 1))()
        keep = []
        for i, q in enumerate(requests):
            r = arr[i]
            r.kf1, r.kf2, r.store = int(q["kf1"]), int(q["kf2"]), int(bool(q.get("store", False)))
            ov = list(q.get("overrides", ()))
            if len(ov) > 2:
                raise ValueError("at most two pose overrides per request")
            r.n_override = len(ov)
            for k, (kid, T) in enumerate(ov):
                r.override_id[k] = int(kid)
                r.override_T[k][:] = np.asarray(T, np.float64).reshape(12).tolist()
            cached = q.get("cached") or {}
            ids = np.array(sorted(int(k) for k in cached), np.int32)
            T = np.ascontiguousarray([np.asarray(cached[int(k)], np.float64).reshape(12) for k in ids], np.float64).reshape(len(ids), 12)
            keep.append((ids, T))
            r.n_cached = len(ids)
            r.cached_ids, r.cached_T = (ids.ctypes.data, T.ctypes.data) if len(ids) else (None, None)
        res = np.zeros(n, MAP_CONSTRAINT_RESULT_DTYPE)
        missing = np.full((n, int(missing_cap)), -1, np.int32)
        depths = np.zeros((n, int(depth_cap)), np.float64)
        self._call("svs_map_compute_constraints", n, arr, int(missing_cap), res.ctypes.data, missing.ctypes.data if missing_cap else None, int(depth_cap),
                   depths.ctypes.data if depth_cap else None)
        self.raw = dict(results=res, missing=missing, depths=depths)
        out = []
        for i in range(n):
            o = dict(status=int(res[i]["status"]), strength=int(res[i]["strength"]), n_missing=int(res[i]["n_missing"]), median=float(res[i]["median"]),
                     norm_dist=float(res[i]["norm_dist"]), T_12=res[i]["T_12"].copy(), info=res[i]["info"].copy(),
                     missing=missing[i, :min(int(res[i]["n_missing"]), int(missing_cap))].copy())
            if depth_cap:
                o["depths"] = depths[i, :o["strength"] if o["status"] == CONS_OK else 0].copy()
            out.append(o)
        return out

    def update_marginalization(self, old_window, new_window, cached=None, missing_cap=64, resolve_missing=False):
        """unmargPosesEnteringInnerW (slam_graph.cpp:728-759) and margPosesLeftInnerWindow (:848-904): windows are (ids, types) with 0 INNER / 1 OUTER, the pairs are
        selected on the host from the edge keys; one unmarginalize, then one storing compute_constraints.  The map's window flags must be those of new_window
        (computeConstraint asks double_window_ for an anchor's pose).  Returns (results, missing): `missing` is the sorted union of the anchors some request
        lacked -- the caller adds their computeAbsolutePose results to `cached` and repeats; a repeat unmarginalises and recomputes the same pairs.
        resolve_missing=True answers `missing` itself through absolute_poses and repeats until no request lacks an anchor it can find a path for"""
        enter = entering_inner_pairs(new_window, self.edge_keys)
        left = left_inner_pairs(old_window, new_window, self.edge_keys)
        if enter:
            self.unmarginalize(enter)
        res = self.compute_constraints([dict(kf1=a, kf2=b, store=True, cached=cached) for a, b in left], missing_cap=missing_cap) if left else []
        missing = sorted({int(k) for o in res for k in o["missing"]})
        if resolve_missing:
            cached = dict(cached or {})
            while missing:
                poses = [o for at in range(0, len(missing), MAP_WALK_MAX_REQUESTS) for o in self.absolute_poses(missing[at:at + MAP_WALK_MAX_REQUESTS])]
                found = {k: o["T"] for k, o in zip(missing, poses) if o["status"] == WALK_OK}
                if not found:
                    break                    # no path to the window (the reference asserts): the caller sees them in `missing`
                cached.update(found)
                res = self.compute_constraints([dict(kf1=a, kf2=b, store=True, cached=cached) for a, b in left], missing_cap=missing_cap)
                missing = sorted({int(k) for o in res for k in o["missing"]})
        return res, missing

    # ---- the pose graph's walks (slam_graph.cpp:64-140, :555-596, :665-725, :762-782): visit order is that of the reference's queue, see include/scavislam_hip.h
    def initial_windows(self, roots, inner_size, double_size, window_cap=None):
        """computeInitialDoubleWin per root -> [(ids in visit order, types 0 INNER / 1 OUTER)]"""
        r = np.ascontiguousarray(roots, np.int32).reshape(-1)
        cap = int(double_size if window_cap is None else window_cap)
        count = np.zeros(len(r), np.int32)
        ids, types = np.full((len(r), max(cap, 1)), -1, np.int32), np.full((len(r), max(cap, 1)), -1, np.int32)
        self._call("svs_map_initial_windows", len(r), r.ctypes.data, int(inner_size), int(double_size), cap, count.ctypes.data, ids.ctypes.data, types.ctypes.data)
        self.raw = dict(count=count, ids=ids, types=types)
        return [(ids[i, :count[i]].copy(), types[i, :count[i]].copy()) for i in range(len(r))]

    def frames_in_neighborhood(self, roots, size):
        """framesInNeighborhood per root -> [ids in visit order]: usable as walk_kf of Registrar.register_map_batch"""
        r = np.ascontiguousarray(roots, np.int32).reshape(-1)
        count = np.zeros(len(r), np.int32)
        ids = np.full((len(r), max(int(size), 1)), -1, np.int32)
        self._call("svs_map_frames_in_neighborhood", len(r), r.ctypes.data, int(size), count.ctypes.data, ids.ctypes.data)
        self.raw = dict(count=count, ids=ids)
        return [ids[i, :count[i]].copy() for i in range(len(r))]

    def absolute_poses(self, kf_ids, path_cap=0):
        """shortestPathToWindow + computeAbsolutePose per keyframe -> [dict(status WALK_OK / WALK_NO_PATH, path_len, T [12], path (the first path_cap ids))]"""
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        cap = int(path_cap)
        status, plen = np.zeros(len(k), np.int32), np.zeros(len(k), np.int32)
        T = np.zeros((len(k), 12), np.float64)
        path = np.full((len(k), cap), -1, np.int32)
        self._call("svs_map_absolute_poses", len(k), k.ctypes.data, cap, status.ctypes.data, plen.ctypes.data, T.ctypes.data, path.ctypes.data if cap else None)
        self.raw = dict(status=status, path_len=plen, T=T, path=path)
        return [dict(status=int(status[i]), path_len=int(plen[i]), T=T[i].copy(), path=path[i, :min(int(plen[i]), cap)].copy()) for i in range(len(k))]

    def reinitialize_poses(self, root_id, old_window, loop_id=-1, changed_cap=None):
        """reinitializePoses over the keyframes in the (new) window; writes the map's poses -> (changed ids in visit order, their total count)"""
        old = np.ascontiguousarray(old_window, np.int32).reshape(-1)
        cap = int(self.info()[0] if changed_cap is None else changed_cap)
        n = C.c_int32()
        changed = np.full(max(cap, 1), -1, np.int32)
        self._call("svs_map_reinitialize_poses", int(root_id), int(loop_id), len(old), old.ctypes.data if len(old) else None, cap, C.byref(n),
                   changed.ctypes.data if cap else None)
        return changed[:min(n.value, cap)].copy(), n.value

    def get_poses(self, kf_ids):
        """blocking read-back of T_me_from_world [n, 12]"""
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        T = np.zeros((len(k), 12), np.float64)
        self._call("svs_map_get_poses", len(k), k.ctypes.data, T.ctypes.data)
        return T

    def prepare_window_from_root(self, root_id, inner_size, double_size, set_window_flags=True, window_cap=MAP_WINDOW_MAX):
        """prepare_window with the initial window and the pairs found on the device from root_id; the same return values"""
        cap = int(window_cap)
        res = MapWindowResult()
        wid, wtype = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), -1, np.int32)
        self._call("svs_map_prepare_window_from_root", int(root_id), int(inner_size), int(double_size), int(bool(set_window_flags)), cap, C.byref(res),
                   wid.ctypes.data, wtype.ctypes.data)
        n = res.n_window if res.n_active >= 0 else 0
        self.window_shape = (res.n_window, res.n_active) if res.n_active >= 0 else None
        return res, wid[:n].copy(), wtype[:n].copy()

    def neighbors_of_root(self, root_id, max_num_neighbors):
        """findNeighborsOfRoot (backend.cpp:287-309) on the host's mirror of the edges: the root's row in ASCENDING (strength, slot), in-window keyframes only.
        The reference compares its count before it increments it, so up to max_num_neighbors + 1 ids come back"""
        root = int(root_id)
        row = sorted((s, slot, b if a == root else a) for slot, (a, b, s) in enumerate(self.edge_log) if root in (a, b))
        ids = np.array([u for _, _, u in row], np.int32)
        if not len(ids):
            return ids
        in_window = [w for at in range(0, len(ids), MAP_WALK_MAX_REQUESTS) for w in self.frames_in_neighborhood(ids[at:at + MAP_WALK_MAX_REQUESTS], 1)]
        out = []
        for u, w in zip(ids.tolist(), in_window):
            if len(w):
                out.append(u)
                if len(out) > int(max_num_neighbors):
                    break
        return np.array(out, np.int32)

    # ---- inserting a keyframe (SlamGraph::addKeyframe, slam_graph.cpp:143-186; computeStrength :467-552): see include/scavislam_hip.h
    @staticmethod
    def _fast_thr(per_level):
        thr = np.full((3, SVS_MAX_CELLS), 25, np.int32)
        for l in range(3):
            t = np.asarray(per_level[l], np.int32).reshape(-1)
            if len(t) > SVS_MAX_CELLS:
                raise ValueError("at most SVS_MAX_CELLS thresholds per level")
            thr[l, :len(t)] = t
        return thr

    def _strength_out(self, res, keys, exists):
        n = 0 if res.over_capacity else res.n_keys
        self.raw = dict(keys=keys, track_exists=exists, n_keys=res.n_keys, m=res.m, over_capacity=res.over_capacity)
        return dict(n_keys=int(res.n_keys), m=int(res.m), over_capacity=bool(res.over_capacity), keys=keys[:n].copy(), track_exists=exists.astype(bool),
                    neighborid_to_strength={int(k["kf_id"]): int(k["strength"]) for k in keys[:n]})

    def compute_strength(self, new_points, track_points, covis_thr, half_width, half_height):
        """computeStrength on the device, the map unchanged: new_points MAP_NEW_POINT_DTYPE (anchor_id is read), track_points MAP_TRACK_POINT_DTYPE.  Returns a
        dict: keys (MAP_KEY_DTYPE, ascending kf_id: strength before the clamp of oldkey, the four class totals), neighborid_to_strength, track_exists, m, n_keys,
        over_capacity (more than MAP_ADDKF_MAX_NEIGHBORS keys: only n_keys is known)"""
        np_ = np.ascontiguousarray(new_points, MAP_NEW_POINT_DTYPE).reshape(-1)
        tp = np.ascontiguousarray(track_points, MAP_TRACK_POINT_DTYPE).reshape(-1)
        res = MapStrengthResult()
        keys = np.zeros(MAP_ADDKF_MAX_NEIGHBORS, MAP_KEY_DTYPE)
        exists = np.zeros(len(tp), np.int32)
        self._call("svs_map_compute_strength", len(np_), np_.ctypes.data if len(np_) else None, len(tp), tp.ctypes.data if len(tp) else None, int(covis_thr),
                   int(half_width), int(half_height), C.byref(res), keys.ctypes.data, exists.ctypes.data if len(tp) else None)
        return self._strength_out(res, keys, exists)

    def add_first_keyframe(self, kf_id, kf, disp, fast_thr):
        """addFirstKeyframe: identity pose; refused unless the map is empty.  kf: one KEYFRAME_DTYPE record (its pose is ignored), disp (device pointer, stride)"""
        k = np.ascontiguousarray(kf, KEYFRAME_DTYPE).reshape(-1)[:1].copy()
        thr = self._fast_thr(fast_thr)
        self._call("svs_map_add_first_keyframe", int(kf_id), k.ctypes.data, C.c_void_p(int(disp[0])), int(disp[1]), thr.ctypes.data)

    def add_keyframe(self, newkey_id, oldkey_id, T_newkey_from_oldkey, kf, disp, fast_thr, new_points, track_points, covis_thr, half_width, half_height,
                     cached=None, missing_cap=16, resolve_missing=False):
        """SlamGraph::addKeyframe in one blocking call (svs_map_add_keyframe).  kf: one KEYFRAME_DTYPE record (pyramid; its pose is ignored), disp: (device
        pointer, stride), fast_thr: per level; new_points MAP_NEW_POINT_DTYPE, track_points MAP_TRACK_POINT_DTYPE; cached {anchor id: T[12]} as compute_constraints
        takes it.  Returns a dict: keys / neighborid_to_strength (AFTER the clamp of oldkey; keys["edge"] marks the new edges), new_kept, track_exists, m,
        over_capacity (then the map is unchanged), edges [(key, newkey)], edge_results (one dict per new edge as compute_constraints returns them), missing
        (sorted union), exclude_set and do_loop_detection (addKeyframeToPlaceRecog, backend.cpp:407-430).  resolve_missing=True completes the edges that lacked
        an anchor through absolute_poses and a storing compute_constraints, as update_marginalization does"""
        np_ = np.ascontiguousarray(new_points, MAP_NEW_POINT_DTYPE).reshape(-1)
        tp = np.ascontiguousarray(track_points, MAP_TRACK_POINT_DTYPE).reshape(-1)
        return self._add_keyframe(newkey_id, oldkey_id, T_newkey_from_oldkey, kf, disp, fast_thr, len(np_), len(tp), covis_thr, half_width, half_height, cached,
                                  missing_cap, resolve_missing, host=(np_, tp))

    def add_keyframe_dev(self, newkey_id, oldkey_id, T_newkey_from_oldkey, kf, disp, fast_thr, d_new, n_new, d_track, n_track, covis_thr, half_width, half_height,
                         cached=None, missing_cap=16, resolve_missing=False):
        """add_keyframe with the two lists in device memory of the map's context (svs_map_add_keyframe_dev): d_new / d_track are device addresses of n_new
        MAP_NEW_POINT_DTYPE / n_track MAP_TRACK_POINT_DTYPE records, complete on the context's stream.  No list record crosses the bus; every refusal about the
        records is decided on the device.  Returns what add_keyframe returns"""
        return self._add_keyframe(newkey_id, oldkey_id, T_newkey_from_oldkey, kf, disp, fast_thr, int(n_new), int(n_track), covis_thr, half_width, half_height, cached,
                                  missing_cap, resolve_missing, dev=(int(d_new) if n_new else 0, int(d_track) if n_track else 0))

    def _add_keyframe(self, newkey_id, oldkey_id, T_newkey_from_oldkey, kf, disp, fast_thr, n_new, n_track, covis_thr, half_width, half_height, cached, missing_cap,
                      resolve_missing, host=None, dev=None, call=None):
        """the two calls above, and StereoFrontend.commitKeyframe (call: the library call, given the output arrays)"""
        k = np.ascontiguousarray(kf, KEYFRAME_DTYPE).reshape(-1)[0] if kf is not None else None
        thr = self._fast_thr(fast_thr) if fast_thr is not None else None
        cached = cached or {}
        cids = np.array(sorted(int(c) for c in cached), np.int32)
        cT = np.ascontiguousarray([np.asarray(cached[int(c)], np.float64).reshape(12) for c in cids], np.float64).reshape(len(cids), 12)
        a = MapAddKeyframeArgs()
        a.newkey_id, a.oldkey_id, a.covis_thr, a.half_width, a.half_height = int(newkey_id), int(oldkey_id), int(covis_thr), int(half_width), int(half_height)
        a.disp_stride, a.n_new, a.n_track = int(disp[1]), n_new, n_track
        if call is None:
            a.T_newkey_from_oldkey[:] = np.asarray(T_newkey_from_oldkey, np.float64).reshape(12).tolist()
            a.keyframe.pyr[:] = [int(p) for p in k["pyr"]]
            a.keyframe.stride[:] = [int(v) for v in k["stride"]]
        a.disp, a.fast_thr = int(disp[0]), (thr.ctypes.data if thr is not None else None)
        if host is not None:
            a.new_points, a.track_points = (host[0].ctypes.data if n_new else None), (host[1].ctypes.data if n_track else None)
        a.cached_ids, a.cached_T, a.n_cached = (cids.ctypes.data if len(cids) else None), (cT.ctypes.data if len(cids) else None), len(cids)
        res = MapStrengthResult()
        keys = np.zeros(MAP_ADDKF_MAX_NEIGHBORS, MAP_KEY_DTYPE)
        kept, exists = np.zeros(n_new, np.int32), np.zeros(n_track, np.int32)
        n_kf = self.info()[0]
        edge_cap = max(1, min(n_kf, MAP_ADDKF_MAX_NEIGHBORS))      # every key is a keyframe of the map; the library writes the first n_edges entries only
        cons = np.zeros(edge_cap, MAP_CONSTRAINT_RESULT_DTYPE)
        cap = int(missing_cap)
        missing = np.full((edge_cap, cap), -1, np.int32)
        outs = (cap, C.byref(res), keys.ctypes.data, kept.ctypes.data if n_new else None, exists.ctypes.data if n_track else None, cons.ctypes.data,
                missing.ctypes.data if cap else None)
        if call is not None:
            call(a, outs)
        elif dev is not None:
            self._call("svs_map_add_keyframe_dev", C.byref(a), C.c_void_p(dev[0]), C.c_void_p(dev[1]), *outs)
        else:
            self._call("svs_map_add_keyframe", C.byref(a), *outs)
        out = self._strength_out(res, keys, exists)
        raw = dict(self.raw, new_kept=kept, results=cons, missing=missing)      # as the library wrote them (resolve_missing's calls leave their own behind)
        out["new_kept"] = kept.astype(bool)
        nbrs = [int(q["kf_id"]) for q in out["keys"] if q["edge"]]
        out["edges"] = [(q, int(newkey_id)) for q in nbrs]
        results = []
        for i in range(len(nbrs)):
            results.append(dict(status=int(cons[i]["status"]), strength=int(cons[i]["strength"]), n_missing=int(cons[i]["n_missing"]), median=float(cons[i]["median"]),
                                norm_dist=float(cons[i]["norm_dist"]), T_12=cons[i]["T_12"].copy(), info=cons[i]["info"].copy(),
                                missing=missing[i, :min(int(cons[i]["n_missing"]), cap)].copy()))
        if not out["over_capacity"]:
            self.window_shape = None
            self.edge_keys.update((min(q, int(newkey_id)), max(q, int(newkey_id))) for q in nbrs)
            self.edge_log += [(q, int(newkey_id), int(s["strength"])) for q, s in zip(nbrs, (x for x in out["keys"] if x["edge"]))]
        miss = sorted({int(v) for o in results for v in o["missing"]})
        if resolve_missing:
            results, miss = self.complete_constraints(out["edges"], results, cached, missing_cap=max(cap, 1))
        self.raw = raw
        out["edge_results"], out["missing"] = results, miss
        out["exclude_set"] = {int(newkey_id)} | set(nbrs)
        out["do_loop_detection"] = len(out["exclude_set"]) < n_kf + (0 if out["over_capacity"] else 1)      # (against vertex_table().size() after the insertion)
        return out

    def complete_constraints(self, pairs, results, cached=None, missing_cap=16, overrides=()):
        """the edges of `pairs` whose result lacks anchors: their poses through absolute_poses, then a storing compute_constraints, until no request lacks an
        anchor that has a path to the window (update_marginalization's resolve_missing) -> (results, the anchors still missing).  overrides: the pose overrides
        every repeated request carries (registerKeyframes / addLoopClosure: the root at its new pose)"""
        results, cached = list(results), dict(cached or {})
        miss = sorted({int(v) for o in results for v in o["missing"]})
        while miss:
            poses = [o for at in range(0, len(miss), MAP_WALK_MAX_REQUESTS) for o in self.absolute_poses(miss[at:at + MAP_WALK_MAX_REQUESTS])]
            found = {q: o["T"] for q, o in zip(miss, poses) if o["status"] == WALK_OK}
            if not found:
                break                        # no path to the window (the reference asserts): the caller sees them in `missing`
            cached.update(found)
            todo = [i for i, o in enumerate(results) if o["n_missing"]]
            for at in range(0, len(todo), MAP_CONS_MAX_REQUESTS):
                part = todo[at:at + MAP_CONS_MAX_REQUESTS]
                again = self.compute_constraints([dict(kf1=pairs[i][0], kf2=pairs[i][1], store=True, cached=cached, overrides=overrides) for i in part],
                                                 missing_cap=missing_cap)
                for i, o in zip(part, again):
                    results[i] = o
            miss = sorted({int(v) for o in results for v in o["missing"]})
        return results, miss

    # ---- committing a registration or a loop closure (SlamGraph::registerKeyframes / addLoopClosure, slam_graph.cpp:188-251): see include/scavislam_hip.h
    def _commit_out(self, res, ekf, est, cons, missing, track_ids, track_added, cached, cap, resolve_missing):
        """the result of one of the three commit calls as a dict; follows the edge mirrors and completes the missing anchors"""
        n_e = int(res.n_edges)
        pair_kf, T_new = int(res.root_id), np.array(res.T_new, np.float64)
        others = [int(k) for k in ekf[:n_e]]
        edges = [(pair_kf, o) if res.mode == REG_LOOP else (o, pair_kf) for o in others]      # (kf1, kf2) of computeConstraint
        results = [dict(status=int(cons[i]["status"]), strength=int(cons[i]["strength"]), n_missing=int(cons[i]["n_missing"]), median=float(cons[i]["median"]),
                        norm_dist=float(cons[i]["norm_dist"]), T_12=cons[i]["T_12"].copy(), info=cons[i]["info"].copy(),
                        missing=missing[i, :min(int(cons[i]["n_missing"]), cap)].copy()) for i in range(n_e)]
        if res.committed:
            if res.n_pairs_added:
                self.window_shape = None
            self.edge_keys.update((min(o, pair_kf), max(o, pair_kf)) for o in others)
            self.edge_log += [(o, pair_kf, int(s)) for o, s in zip(others, est[:n_e])]
        miss = sorted({int(v) for o in results for v in o["missing"]})
        if resolve_missing and miss:
            results, miss = self.complete_constraints(edges, results, cached, missing_cap=max(cap, 1), overrides=[(pair_kf, T_new)])
        return dict(committed=bool(res.committed), status=int(res.status), mode=int(res.mode), root_id=pair_kf, other_id=int(res.other_id), T_new=T_new,
                    n_track=int(res.n_track), n_pairs_added=int(res.n_pairs_added), track_point_ids=track_ids, track_added=track_added, edges=edges,
                    edge_strength=[int(s) for s in est[:n_e]], edge_results=results, missing=miss)

    def register_keyframes(self, root_id, T_newroot_from_w, neighborid_to_strength, track_points, covis_thr, cached=None, missing_cap=16, resolve_missing=True):
        """SlamGraph::registerKeyframes with the caller's own lists (svs_map_register_keyframes): neighborid_to_strength {keyframe id: strength} (addNewEdges' test
        strength >= covis_thr is applied here; the edges come in ascending id), track_points MAP_TRACK_POINT_DTYPE.  Returns what KeyframeRegistrar.commit returns"""
        tp = np.ascontiguousarray(track_points, MAP_TRACK_POINT_DTYPE).reshape(-1)
        nb = np.array([int(k) for k in neighborid_to_strength], np.int32)
        st = np.array([int(neighborid_to_strength[k]) for k in neighborid_to_strength], np.int32)
        T = np.ascontiguousarray(T_newroot_from_w, np.float64).reshape(12)
        cids, cT = _cached_arrays(cached)
        cap, n = int(missing_cap), max(len(nb), 1)
        res = RegCommitResult()
        ekf, cons, missing, added = np.full(n, -1, np.int32), np.zeros(n, MAP_CONSTRAINT_RESULT_DTYPE), np.full((n, cap), -1, np.int32), np.zeros(len(tp), np.int32)
        self._call("svs_map_register_keyframes", int(root_id), T.ctypes.data, len(nb), nb.ctypes.data if len(nb) else None, st.ctypes.data if len(nb) else None,
                   int(covis_thr), len(tp), tp.ctypes.data if len(tp) else None, len(cids), cids.ctypes.data if len(cids) else None,
                   cT.ctypes.data if len(cids) else None, cap, C.byref(res), ekf.ctypes.data, cons.ctypes.data, missing.ctypes.data if cap else None,
                   added.ctypes.data if len(tp) else None)
        by_id = {int(k): int(v) for k, v in zip(nb, st)}
        est = np.array([by_id[int(k)] for k in ekf[:res.n_edges]], np.int32)
        self.raw = dict(result=bytes(res), edge_kf=ekf, results=cons, missing=missing, track_added=added)
        return self._commit_out(res, ekf, est, cons, missing, tp["global_id"].copy(), added.astype(bool), cached, cap, resolve_missing)

    def add_loop_closure(self, root_id, loop_id, T_newloop_from_w, track_points, cached=None, missing_cap=16, resolve_missing=True):
        """SlamGraph::addLoopClosure with the caller's own list (svs_map_add_loop_closure): the pairs go to loop_id, the APPEARANCE edge (root_id, loop_id) has
        strength len(track_points).  Returns what KeyframeRegistrar.commit returns"""
        tp = np.ascontiguousarray(track_points, MAP_TRACK_POINT_DTYPE).reshape(-1)
        T = np.ascontiguousarray(T_newloop_from_w, np.float64).reshape(12)
        cids, cT = _cached_arrays(cached)
        cap = int(missing_cap)
        res = RegCommitResult()
        cons, missing, added = np.zeros(1, MAP_CONSTRAINT_RESULT_DTYPE), np.full((1, cap), -1, np.int32), np.zeros(len(tp), np.int32)
        self._call("svs_map_add_loop_closure", int(root_id), int(loop_id), T.ctypes.data, len(tp), tp.ctypes.data if len(tp) else None, len(cids),
                   cids.ctypes.data if len(cids) else None, cT.ctypes.data if len(cids) else None, cap, C.byref(res), cons.ctypes.data,
                   missing.ctypes.data if cap else None, added.ctypes.data if len(tp) else None)
        self.raw = dict(result=bytes(res), results=cons, missing=missing, track_added=added)
        return self._commit_out(res, np.array([int(root_id)], np.int32), np.array([len(tp)], np.int32), cons, missing, tp["global_id"].copy(), added.astype(bool),
                                cached, cap, resolve_missing)

    def get_points(self, point_ids):
        """blocking read-back of the stored point records (CANDIDATE_DTYPE, kf_index = the anchor's id)"""
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        out = np.zeros(len(p), CANDIDATE_DTYPE)
        self._call("svs_map_get_points", len(p), p.ctypes.data, out.ctypes.data)
        return out

    def get_keyframe(self, kf_id):
        """blocking read-back of what the map stores of a keyframe -> (one KEYFRAME_DTYPE record, (disparity device pointer, stride), thresholds [3][SVS_MAX_CELLS])"""
        kf, thr = np.zeros(1, KEYFRAME_DTYPE), np.zeros((3, SVS_MAX_CELLS), np.int32)
        disp, stride = C.c_void_p(), C.c_int32()
        self._call("svs_map_get_keyframe", int(kf_id), kf.ctypes.data, C.byref(disp), C.byref(stride), thr.ctypes.data)
        return kf[0], (disp.value or 0, stride.value), thr

    def get_feature_table(self, kf_id, cap=None):
        """blocking read-back of a keyframe's feature_table -> (point ids ascending, BA_EDGE_DTYPE measurement records, the table's length).  A pair without a
        measurement has obs and info zero and anchor = -1"""
        cap = int(self.info()[1] if cap is None else cap)
        n = C.c_int32()
        ids, rec = np.full(max(cap, 1), -1, np.int32), np.zeros(max(cap, 1), BA_EDGE_DTYPE)
        self._call("svs_map_get_feature_table", int(kf_id), cap, C.byref(n), ids.ctypes.data, rec.ctypes.data)
        k = min(n.value, cap)
        return ids[:k].copy(), rec[:k].copy(), n.value

    def info(self):
        """(keyframes, points, distinct observations)"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._call("svs_map_info", C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def close(self):
        if self.h:
            self.ctx.lib.svs_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
