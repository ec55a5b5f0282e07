"""Host-side mirror of the loop-closure geometric check.

  GeometricChecker.check(query, train)  <- PlaceRecognizer::geometricCheck   placerecognizer.cpp:175-202
  GeometricChecker.set_place(...)       <- location_map_.insert(...)         placerecognizer.cpp:299

Detection, description (SURF) and the bag-of-words index stay with the caller; this class takes a Place the way geometricCheck consumes it
(descriptors, uvu_0_vec, optionally xyz_vec) and keeps it on the device.  There is no CPU path: every call goes to svs_loop_* of the HIP library.
"""
import ctypes as C

import numpy as np

from .ctypes_types import Cam, LoopCheck, LoopResult


class LoopCheckOutput:
    """One check's outputs, cut to its n_matches / n_hyp."""

    def __init__(self, res, train_idx, distance, inlier, samples, hyp_inliers):
        self.n_matches, self.n_inliers, self.best_hyp, self.n_invalid_hyp = res.n_matches, res.n_inliers, res.best_hyp, res.n_invalid_hyp
        self.T_query_from_train = np.array(res.T_query_from_train, np.float64).reshape(3, 4)
        self.train_idx, self.distance, self.inlier, self.samples, self.hyp_inliers = train_idx, distance, inlier, samples, hyp_inliers

    def detected(self, min_inliers=30):
        """the caller's test of placerecognizer.cpp:198"""
        return self.n_inliers > min_inliers


class GeometricChecker:
    def __init__(self, ctx, cam, desc_dim=64, max_desc=2048, max_places=64, max_hyp=100, max_checks=32):
        self.ctx, self.h = ctx, None
        self.cam = cam if isinstance(cam, Cam) else Cam(cam["f"], cam["cx"], cam["cy"], cam["b"], int(cam.get("w", 0)), int(cam.get("h", 0)))
        self.desc_dim, self.max_desc, self.max_places, self.max_hyp, self.max_checks = desc_dim, max_desc, max_places, max_hyp, max_checks
        h = C.c_void_p()
        ctx.call("svs_loop_create", C.byref(self.cam), desc_dim, max_desc, max_places, max_hyp, max_checks, C.byref(h))
        self.h = h
        ctx.children.add(self)
        self.raw = None      # the full-length rows of the last check_batch (tests: byte comparisons)

    def set_place(self, slot, descriptors, uvu, xyz=None):
        d = np.ascontiguousarray(descriptors, np.float32)
        u = np.ascontiguousarray(uvu, np.float64)
        x = None if xyz is None else np.ascontiguousarray(xyz, np.float64)
        n = d.shape[0] if d.ndim == 2 else 0
        if n and (d.shape[1] != self.desc_dim or u.shape != (n, 3) or (x is not None and x.shape != (n, 3))):
            raise ValueError("descriptors [n][desc_dim], uvu [n][3], xyz [n][3] expected")
        self.ctx.check(self.ctx.lib.svs_loop_set_place(self.h, int(slot), int(n), d.ctypes.data, u.ctypes.data, None if x is None else x.ctypes.data))

    def check_batch(self, checks, n_hyp=100, pixel_thr=2.5, seed=0):
        """checks: (query_slot, train_slot) pairs or dicts with query, train and optionally n_hyp, pixel_thr, seed, samples ([n_hyp][3] match indices)"""
        n = len(checks)
        arr = (LoopCheck * max(n, 1))()
        keep = []
        for i, c in enumerate(checks):
            c = c if isinstance(c, dict) else dict(query=c[0], train=c[1])
            smp = c.get("samples")
            H = int(c.get("n_hyp", n_hyp if smp is None else len(smp)))
            ptr = None
            if smp is not None:
                smp = np.ascontiguousarray(smp, np.int32)
                if smp.shape != (H, 3):
                    raise ValueError("samples must be [n_hyp][3]")
                keep.append(smp)
                ptr = smp.ctypes.data
            arr[i] = LoopCheck(int(c["query"]), int(c["train"]), H, float(c.get("pixel_thr", pixel_thr)), int(c.get("seed", seed)) & (2 ** 64 - 1), ptr)
        res = (LoopResult * max(n, 1))()
        tidx = np.empty((n, self.max_desc), np.int32)
        dist = np.empty((n, self.max_desc), np.float32)
        inl = np.empty((n, self.max_desc), np.uint8)
        smp_out = np.empty((n, self.max_hyp, 3), np.int32)
        hinl = np.empty((n, self.max_hyp), np.int32)
        self.ctx.check(self.ctx.lib.svs_loop_check_batch(self.h, n, arr, res, tidx.ctypes.data, dist.ctypes.data, inl.ctypes.data, smp_out.ctypes.data,
                                                         hinl.ctypes.data))
        self.raw = dict(results=bytes(res)[:n * C.sizeof(LoopResult)], train_idx=tidx, distance=dist, inlier=inl, samples=smp_out, hyp_inliers=hinl)
        out = []
        for i in range(n):
            m, H = res[i].n_matches, arr[i].n_hyp
            out.append(LoopCheckOutput(res[i], tidx[i, :m], dist[i, :m], inl[i, :m].astype(bool), smp_out[i, :H], hinl[i, :H]))
        return out

    def check(self, query, train, **kw):
        return self.check_batch([dict(query=query, train=train, **kw)])[0]

    def set_timing(self, on=True):
        self.ctx.check(self.ctx.lib.svs_loop_set_timing(self.h, int(on)))

    def stage_times_ms(self):
        """(distance stage, RANSAC stage) of the last check_batch, from events; zeros unless set_timing(True)"""
        ms = (C.c_float * 2)()
        self.ctx.check(self.ctx.lib.svs_loop_stage_times(self.h, ms))
        return float(ms[0]), float(ms[1])

    def close(self):
        if self.h:
            self.ctx.lib.svs_loop_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
