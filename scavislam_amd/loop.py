"""Host-side mirror of the loop-closure geometric check.

  GeometricChecker.check(query, train)  <- PlaceRecognizer::geometricCheck   placerecognizer.cpp:175-202
  GeometricChecker.set_place(...)       <- location_map_.insert(...)         placerecognizer.cpp:299

  GeometricChecker.set_vocabulary(w)    <- words_ / flann_index_             placerecognizer.cpp:55-75
  GeometricChecker.add_locations(...)   <- addLocation from :248 to :318     visual words, inverted index, TF-IDF scores, the candidate test
  train_vocabulary(ctx, descriptors, n) <- calculateWordsAndSaveThem         create_dictionary.cpp:144-177 (flat Lloyd + k-means++ instead of the tree cut)

  SurfExtractor.extract(images, disp)   <- surf.detect / the disparity filter / surf_ext.compute   placerecognizer.cpp:212-246
  GeometricChecker.set_place_from_surf  <- the same insert, device to device

GeometricChecker takes a Place the way geometricCheck consumes it (descriptors, uvu_0_vec, optionally xyz_vec) and keeps it on the device; SurfExtractor makes
one from a keyframe's level-0 image and disparity that are already there.  There is no CPU path: every call goes to svs_loop_* of the HIP library.
"""
import ctypes as C
import time

import numpy as np

from .ctypes_types import SURF_KEYPOINT_DTYPE, SURF_STAGES, Cam, LoopCheck, LoopLocation, LoopLocationResult, LoopResult, SurfParams, VocabParams, VocabResult


class LoopCheckOutput:
    """One check's outputs, cut to its n_matches / n_hyp."""

    def __init__(self, res, train_idx, distance, inlier, samples, hyp_inliers):
        self.n_matches, self.n_inliers, self.best_hyp, self.n_invalid_hyp = res.n_matches, res.n_inliers, res.best_hyp, res.n_invalid_hyp
        self.T_query_from_train = np.array(res.T_query_from_train, np.float64).reshape(3, 4)
        self.train_idx, self.distance, self.inlier, self.samples, self.hyp_inliers = train_idx, distance, inlier, samples, hyp_inliers

    def detected(self, min_inliers=30):
        """the caller's test of placerecognizer.cpp:198"""
        return self.n_inliers > min_inliers


class LocationOutput:
    """One added location: the fields of svs_loop_location_result, its words / squared distances cut to its descriptor count, its score row."""

    def __init__(self, slot, res, word, word_d2, scores):
        self.slot = slot
        self.number_of_words, self.n_scored, self.best_slot, self.best_score, self.candidate = (res.number_of_words, res.n_scored, res.best_slot,
                                                                                                np.float32(res.best_score), bool(res.candidate))
        self.word, self.word_d2, self.scores = word, word_d2, scores


class LocationBatch(list):
    """The LocationOutputs of one add_locations call, in call order."""

    def candidates(self):
        """(query_slot, best_slot) of the locations whose best score passed min_score: what check_batch takes"""
        return [(o.slot, o.best_slot) for o in self if o.candidate]


class VocabularyOutput:
    """What svs_vocab_train returns: words [n_words_out][desc_dim] (set_vocabulary takes them as they are), seed_index [n_words] (-1 behind n_seeded),
    assign / assign_d2 [n] against the words as returned, count [n_words_out], changed [iterations_run], result (the svs_vocab_result fields).
    raw: the full-length arrays as the library wrote them (tests: byte comparisons)"""

    def __init__(self, res, words, seed_index, assign, assign_d2, count, changed):
        self.result = res
        self.n_words_out, self.n_seeded, self.iterations_run, self.converged, self.n_empty, self.inertia_q28 = (
            res.n_words_out, res.n_seeded, res.iterations_run, bool(res.converged), res.n_empty, int(res.inertia_q28))
        self.raw = dict(words=words, seed_index=seed_index, assign=assign, assign_d2=assign_d2, count=count, changed=changed)
        self.words, self.seed_index, self.assign, self.assign_d2 = words[:res.n_words_out], seed_index, assign, assign_d2
        self.count, self.changed = count[:res.n_words_out], changed[:res.iterations_run]

    def raw_bytes(self):
        r = self.result
        head = np.array([r.n_words_out, r.n_seeded, r.iterations_run, r.converged, r.n_empty, r.inertia_q28 & 0xffffffff, r.inertia_q28 >> 32], np.int64)
        return [head.tobytes()] + [self.raw[k].tobytes() for k in ("words", "seed_index", "assign", "assign_d2", "count", "changed")]


def train_vocabulary(ctx, descriptors, n_words, iterations=11, seed=0, init=None, drop_empty=True):
    """k-means++ seeding and Lloyd iterations on the device (svs_vocab_train; the header has the semantics).  descriptors [n][64 or 128] f32 with |x| < 4,
    init: [n_words][desc_dim] start centres instead of the seeding.  Blocking; returns a VocabularyOutput"""
    d = np.ascontiguousarray(descriptors, np.float32)
    if d.ndim != 2:
        raise ValueError("descriptors [n][desc_dim] expected")
    n, K = d.shape
    nw = int(n_words)
    ini = None
    if init is not None:
        ini = np.ascontiguousarray(init, np.float32)
        if ini.shape != (nw, K):
            raise ValueError("init [n_words][desc_dim] expected")
    prm = VocabParams(nw, int(iterations), int(seed) & (2 ** 64 - 1), None if ini is None else ini.ctypes.data, int(bool(drop_empty)))
    res = VocabResult()
    m = max(nw, 0)
    words = np.zeros((m, K), np.float32)
    seed_index = np.full(m, -1, np.int32)
    assign = np.full(n, -1, np.int32)
    d2 = np.zeros(n, np.float32)
    count = np.zeros(m, np.int32)
    changed = np.full(max(int(iterations), 0), -1, np.int32)
    ctx.call("svs_vocab_train", int(K), int(n), d.ctypes.data, C.byref(prm), words.ctypes.data, C.byref(res), seed_index.ctypes.data, assign.ctypes.data,
             d2.ctypes.data, count.ctypes.data, changed.ctypes.data)
    return VocabularyOutput(res, words, seed_index, assign, d2, count, changed)


def vocabulary_stage_times_ms(ctx):
    """(seeding, assignment, update) of the context's last train_vocabulary, from events: the launches of all iterations summed"""
    ms = (C.c_float * 3)()
    ctx.call("svs_vocab_stage_times", ms)
    return float(ms[0]), float(ms[1]), float(ms[2])


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
        self.raw_index = None      # the same of the last add_locations
        self.n_place = {}      # descriptors per loaded slot

    def set_place(self, slot, descriptors, uvu, xyz=None):
        d = np.ascontiguousarray(descriptors, np.float32)
        u = np.ascontiguousarray(uvu, np.float64)
        x = None if xyz is None else np.ascontiguousarray(xyz, np.float64)
        n = d.shape[0] if d.ndim == 2 else 0
        if n and (d.shape[1] != self.desc_dim or u.shape != (n, 3) or (x is not None and x.shape != (n, 3))):
            raise ValueError("descriptors [n][desc_dim], uvu [n][3], xyz [n][3] expected")
        self.ctx.check(self.ctx.lib.svs_loop_set_place(self.h, int(slot), int(n), d.ctypes.data, u.ctypes.data, None if x is None else x.ctypes.data))
        self.n_place[int(slot)] = int(n)

    def set_place_from_surf(self, slot, surf, image_index):
        """the place of image `image_index` of surf's last extract(), device to device (svs_loop_set_place_from_surf)"""
        self.ctx.check(self.ctx.lib.svs_loop_set_place_from_surf(self.h, int(slot), surf.h, int(image_index)))
        self.n_place[int(slot)] = int(surf.last_count[int(image_index)])

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

    def set_vocabulary(self, words):
        """words [n_words][desc_dim] f32 (the rows of surfwords10000.png); resets the index to empty"""
        w = np.ascontiguousarray(words, np.float32)
        if w.ndim != 2 or w.shape[1] != self.desc_dim:
            raise ValueError("words [n_words][desc_dim] expected")
        self.ctx.check(self.ctx.lib.svs_loop_set_vocabulary(self.h, int(w.shape[0]), w.ctypes.data))
        self.n_words = int(w.shape[0])

    def add_locations(self, locations, do_loop_detection=True, radius=0.1, min_score=2.0):
        """locations: slots or dicts with slot and optionally exclude (slots), do_loop_detection, radius, min_score; the places were loaded with set_place.
        Returns a LocationBatch; .candidates() goes straight to check_batch"""
        n = len(locations)
        arr = (LoopLocation * max(n, 1))()
        keep, slots = [], []
        for i, c in enumerate(locations):
            c = c if isinstance(c, dict) else dict(slot=c)
            ex = np.ascontiguousarray(c.get("exclude", ()), np.int32).reshape(-1)
            keep.append(ex)
            slots.append(int(c["slot"]))
            arr[i] = LoopLocation(slots[-1], int(bool(c.get("do_loop_detection", do_loop_detection))), ex.ctypes.data if len(ex) else None, len(ex),
                                  float(c.get("radius", radius)), float(c.get("min_score", min_score)))
        res = (LoopLocationResult * max(n, 1))()
        word = np.empty((n, self.max_desc), np.int32)
        d2 = np.empty((n, self.max_desc), np.float32)
        scores = np.empty((n, self.max_places), np.float32)
        self.ctx.check(self.ctx.lib.svs_loop_add_locations(self.h, n, arr, res, word.ctypes.data, d2.ctypes.data, scores.ctypes.data))
        self.raw_index = dict(results=bytes(res)[:n * C.sizeof(LoopLocationResult)], word=word, word_d2=d2, scores=scores)
        out = LocationBatch()
        for i in range(n):
            m = self.n_place[slots[i]]
            out.append(LocationOutput(slots[i], res[i], word[i, :m], d2[i, :m], scores[i]))
        return out

    def index_stage_times_ms(self):
        """(words stage, scoring stage) of the last add_locations, from events; zeros unless set_timing(True)"""
        ms = (C.c_float * 2)()
        self.ctx.check(self.ctx.lib.svs_loop_index_stage_times(self.h, ms))
        return float(ms[0]), float(ms[1])

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


class SurfPlace:
    """One image's outputs of SurfExtractor.extract, cut to its count: keypoints (SURF_KEYPOINT_DTYPE), uvu [n][3] f64, descriptors [n][64] f32, overflow"""

    def __init__(self, keypoints, uvu, descriptors, overflow):
        self.keypoints, self.uvu, self.descriptors, self.overflow = keypoints, uvu, descriptors, bool(overflow)

    def __len__(self):
        return len(self.keypoints)


class SurfExtractor:
    """svs_surf_*: SURF detection, the disparity filter and description of a batch of keyframes on the device (the header has the semantics)."""

    def __init__(self, ctx, cam, w, h, max_batch=1, max_keypoints=2048, params=None):
        self.ctx, self.h = ctx, None
        self.cam = cam if isinstance(cam, Cam) else Cam(cam["f"], cam["cx"], cam["cy"], cam["b"], int(w), int(h))
        self.w, self.hgt, self.max_batch, self.max_keypoints = int(w), int(h), int(max_batch), int(max_keypoints)
        self.params = params or SurfParams.reference()
        h_ = C.c_void_p()
        ctx.call("svs_surf_create", C.byref(self.cam), self.w, self.hgt, self.max_batch, self.max_keypoints, C.byref(self.params), C.byref(h_))
        self.h = h_
        ctx.children.add(self)
        self.last_count = np.zeros(0, np.int32)
        self.raw = None      # the full-length arrays of the last extract (tests: byte comparisons)

    def extract_device(self, d_img, stride, bstride, d_disp, dstride, d_bstride, n_batch):
        """device pointers (ints): u8 images (strides in bytes), f32 disparity (strides in floats; 0 / None without).  Blocking; returns [SurfPlace]"""
        n, m = int(n_batch), self.max_keypoints
        count, over = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        kp = np.zeros((max(n, 1), m), SURF_KEYPOINT_DTYPE)
        uvu = np.zeros((max(n, 1), m, 3), np.float64)
        desc = np.zeros((max(n, 1), m, 64), np.float32)
        t0 = time.perf_counter()
        rc = self.ctx.lib.svs_surf_extract(self.h, d_img, int(stride), int(bstride), d_disp or None, int(dstride), int(d_bstride), n, count.ctypes.data,
                                           over.ctypes.data, kp.ctypes.data, uvu.ctypes.data, desc.ctypes.data)
        self.last_call_ms = (time.perf_counter() - t0) * 1e3      # wall time of the blocking library call alone
        self.ctx.check(rc)
        self.last_count = count[:n].copy()
        self.raw = dict(count=count, overflow=over, keypoints=kp, uvu=uvu, descriptors=desc)
        return [SurfPlace(kp[b, :count[b]], uvu[b, :count[b]], desc[b, :count[b]], over[b]) for b in range(n)]

    def extract(self, images, disp=None, stride=None):
        """images [n][h][w] u8 and disp [n][h][w] f32 on the host (convenience: uploaded through torch, `stride` pads the device rows)"""
        import torch
        img = np.ascontiguousarray(images, np.uint8)
        n, h, w = img.shape
        st = int(stride or w)
        pad = np.zeros((n, h, st), np.uint8)
        pad[:, :, :w] = img
        d_img = torch.as_tensor(pad).cuda()
        d_disp = None
        if disp is not None:
            dp = np.full((n, h, st), np.nan, np.float32)
            dp[:, :, :w] = np.ascontiguousarray(disp, np.float32)
            d_disp = torch.as_tensor(dp).cuda()
        torch.cuda.synchronize()
        out = self.extract_device(d_img.data_ptr(), st, h * st, d_disp.data_ptr() if d_disp is not None else None, st, h * st, n)
        return out

    def set_timing(self, on=True):
        self.ctx.check(self.ctx.lib.svs_surf_set_timing(self.h, int(on)))

    def stage_times_ms(self):
        """(integral, responses, maxima, order, orientation + descriptor, compaction) of the last extract, from events; zeros unless set_timing(True)"""
        ms = (C.c_float * SURF_STAGES)()
        self.ctx.check(self.ctx.lib.svs_surf_stage_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def close(self):
        if self.h:
            self.ctx.lib.svs_surf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
