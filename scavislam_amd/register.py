"""Host-side mirror of the back end's re-registration of a keyframe against the map.

  KeyframeRegistrar.local_register(requests)  <- Backend::localRegisterFrame   backend.cpp:549-611 (pointsVisibleInRoot :472-546, matchAndAlign :725-784,
                                                                               keyframesToRegister :615-722)
  KeyframeRegistrar.loop_closure(requests)    <- Backend::globalLoopClosure    backend.cpp:830-1001

A request is one root keyframe with the candidate map points the caller's graph walk found (framesInNeighborhood, the hash-set deduplication, registerKeyframes /
addLoopClosure stay with the caller).  A batch of requests is ONE library call: one staged upload, one chain of launches, one download.  There is no CPU path:
every call goes to svs_reg_* of the HIP library.
"""
import ctypes as C

import numpy as np

from .ctypes_types import (CANDIDATE_DTYPE, KEYFRAME_DTYPE, MATCH_RESULT_DTYPE, REG_KF_STATS_DTYPE, REG_LOCAL, REG_LOOP, REG_OK, REG_STAGES, SVS_MAX_CELLS, Cam,
                           RegParams, RegRequest, RegResult)


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

    def local_register(self, requests, **kw):
        return self.register_batch(requests, [REG_LOCAL] * len(requests), **kw)

    def loop_closure(self, requests, **kw):
        return self.register_batch(requests, [REG_LOOP] * len(requests), **kw)

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
