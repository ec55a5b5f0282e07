"""Every path svs_stereo_compute can take, and every parameter of the block matcher, against the oracle restatement of cv::StereoBM (bit-exact: an integer
pipeline).  tests/test_gpu_stereo.py runs the reference parameters on frames up to 640 pixels wide with pyramid strides; here the dispatch of csrc/stereo.hip
(svs_stereo_compute; the kernels are in csrc/stereo_prefilter.inc, stereo_search.inc and stereo_speckle.inc) is
walked on purpose: the whole-frame speckle filter (rows too wide for strips, short frames, huge windows, and forced beside the strip filter), many small strips,
the one-row left-right check of rows wider than 2048 pixels, both prefilter kernels, unaligned pointers and three different strides, the tile edges of the
block-matching kernels, handles reused on changing frames, and the widest row create accepts.

Which path ran is ASSERTED through the context's counters (svs_ctx_get_stat "stereo_*"), and after every call the error mask of the speckle filter's bounded
walks must be 0: the strip filter's and, since its union-find is bounded too, the whole-frame filter's.  Before a comparison the test checks on the ORACLE's output alone that the case has work for the stage it is about (pixels kept and removed by the
speckle filter, pixels removed by the left-right check, small components across strip boundaries): the counts measured when the test was written stand in the
docstrings.  Inputs: tests/stereo_cases.py (a rendered pair of Scene(7) with uniform integer noise on both images; noise against its own roll)."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases as SC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5      # no disparity: results are multiples of 1/16 in [-1, 32)
COUNTERS = ("stereo_prefilter16_calls", "stereo_prefilter4_calls", "stereo_strip_filter_calls", "stereo_strip_filter_strips", "stereo_frame_filter_calls",
            "stereo_validate_wide_calls")
SVS_ERR_UNSUPPORTED = 5
MAX_W = 20164            # 8 w + 8 ceil(w / 64) <= 160 KB (include/scavislam_hip.h: svs_stereo_create)


def _round_up(a, b):
    return (a + b - 1) // b * b


def spk_row_bytes(w):
    """LDS bytes of one strip row (csrc/stereo.hip: spk_row_bytes, SPK_NS)"""
    return _round_up(w, 4) * 6 + (320 if (w + 63) // 64 <= 10 else 0)


def strips_of(w, h, strip_kb=151):
    rows = min(h, strip_kb * 1024 // spk_row_bytes(w))
    assert rows >= 16, "the handle would take the whole-frame path"
    return rows, (h + rows - 1) // rows


def _stats(ctx):
    return {n: ctx.get_stat(n) for n in COUNTERS}


def _error_mask(ctx):
    return ctx.get_stat("stereo_speckle_error_mask")


class Handle:
    """svs_stereo of the C API (the environment switches are read when it is created)"""

    def __init__(self, ctx, w, h, max_batch, prm):
        self.ctx, self.w, self.h, self.max_batch, self.prm = ctx, w, h, max_batch, prm
        self.h_ = C.c_void_p()
        ctx.call("svs_stereo_create", w, h, max_batch, C.byref(prm), C.byref(self.h_))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.h_:
            self.ctx.lib.svs_stereo_destroy(self.h_)
            self.h_ = None


def _compute(gpu_ctx, hd, pairs, strides=None, offsets=(0, 0), slack=(0, 0, 0), dguard=32, fill_seed=0):
    """one svs_stereo_compute on buffers laid out as asked: strides = (lstride, rstride, dstride) in elements (default: the width rounded up to 64, as the frame
    pyramids have it), offsets = bytes added to the left / right pointer, slack = extra elements between the batch slots of left / right / output.  The input
    buffers are filled with random bytes (fill_seed) around the images; the output buffer -- `dguard` floats, the hd.max_batch slots, 32 floats -- is filled with
    SENTINEL, and every element outside the [len(pairs)][h][w] rectangle must still hold it afterwards.  -> list of [h, w] float32"""
    import torch
    ctx, stream = gpu_ctx
    w, h, n = hd.w, hd.h, len(pairs)
    ls, rs, ds = strides or (_round_up(w, 64),) * 3
    lb, rb, db = h * ls + slack[0], h * rs + slack[1], h * ds + slack[2]
    rng = np.random.default_rng(1000 + fill_seed)
    bufs = []
    for side, (stride, bstride, off) in enumerate(((ls, lb, offsets[0]), (rs, rb, offsets[1]))):
        a = rng.integers(0, 256, 64 + off + n * bstride + 64).astype(np.uint8)
        for b, pair in enumerate(pairs):
            img = np.ascontiguousarray(pair[side], np.uint8)
            assert img.shape == (h, w)
            rows = 64 + off + b * bstride + np.arange(h)[:, None] * stride + np.arange(w)[None, :]
            a[rows] = img
        bufs.append(a)
    out = np.full(dguard + hd.max_batch * db + 32, SENTINEL, np.float32)
    with torch.cuda.stream(stream):
        d_l, d_r, d_o = (torch.as_tensor(a).cuda() for a in (bufs[0], bufs[1], out))
    assert d_l.data_ptr() % 16 == 0 and d_r.data_ptr() % 16 == 0 and d_o.data_ptr() % 16 == 0      # so that `offsets` / `dguard` decide the alignment
    ctx.check(ctx.lib.svs_stereo_compute(hd.h_, d_l.data_ptr() + 64 + offsets[0], ls, lb, d_r.data_ptr() + 64 + offsets[1], rs, rb,
                                         d_o.data_ptr() + 4 * dguard, ds, db, n))
    ctx.sync()
    res = d_o.cpu().numpy()
    inside = (dguard + np.arange(n)[:, None, None] * db + np.arange(h)[None, :, None] * ds + np.arange(w)[None, None, :])
    outside = np.ones(res.size, bool)
    outside[inside.ravel()] = False
    touched = np.flatnonzero(outside & (res != np.float32(SENTINEL)))
    assert touched.size == 0, f"{touched.size} elements outside the {n} x {h} x {w} result were written, first at {touched[:8] - dguard} (slot stride {db}, row stride {ds})"
    return [res[inside[b]] for b in range(n)]


def _run(gpu_ctx, pairs, prm, max_batch=None, **layout):
    """create, compute, destroy -> (results, counter steps of the call); the error mask must be 0"""
    ctx, _ = gpu_ctx
    h, w = pairs[0][0].shape
    before = _stats(ctx)
    with Handle(ctx, w, h, max_batch or len(pairs), prm) as hd:
        got = _compute(gpu_ctx, hd, pairs, **layout)
    after = _stats(ctx)
    assert _error_mask(ctx) == 0, "a bounded walk of the speckle filter (strip or whole-frame) gave up"
    return got, {k: after[k] - before[k] for k in COUNTERS}


def _assert_equal(got, pairs, prm, what=""):
    import oracle as O
    refs = []
    for i, ((l, r), g) in enumerate(zip(pairs, got)):
        ref = O.stereo_bm(l, r, prm)
        assert g.dtype == np.float32 and g.shape == ref.shape
        assert np.array_equal(g, ref), f"{what} pair {i}: {(g != ref).sum()} px differ from the oracle, first at {np.argwhere(g != ref)[:4].tolist()}"
        refs.append(ref)
    return refs


def _speckle_work(l, r, prm, keep=0.05, remove=0.01):
    """the oracle's speckle stage keeps >= 5 % of the frame and removes >= 1 % of it -> (bm valid, removed by the LR check, kept, removed by the speckle stage)"""
    c = SC.counts(l, r, prm)
    n = l.size
    assert c[2] >= keep * n and c[3] >= remove * n, f"vacuous speckle case: kept {c[2]}, removed {c[3]} of {n} px"
    return c


def _lr_work(l, r, prm):
    c = SC.counts(l, r, prm)
    assert c[1] >= 10, f"vacuous left-right case: the check removes {c[1]} px"
    return c


def _straddling(l, r, prm, rows, at_least=4):
    val = SC.stages(l, r, prm)[1]
    k = SC.straddling_small_components(val, rows, prm.speckle_window, prm.speckle_range)
    assert k >= at_least, f"vacuous multi-strip case: {k} small components across a strip boundary"
    return k


# ---- a. the whole-frame speckle filter where the dispatch chooses it by itself -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,amp,window", [(1616, 24, 6, 30), (1618, 20, 6, 100), (64, 12, 25, 100), (322, 250, 0, 20000)])
def test_frame_filter_natural_fallbacks(gpu_ctx, w, h, amp, window):
    """rows wider than the 1610 pixels of which 16 fit LDS (w % 4 = 0: stereo_ccl_merge4_kernel + stereo_finish4_kernel; w % 4 = 2: stereo_ccl_merge_kernel +
    stereo_finish_kernel), a frame of fewer than 16 rows, and a window beyond what the strip filter's saturating counts hold (>= 16368).
    Oracle alone, (valid after block matching, removed by the left-right check, kept, removed by the speckle filter):
    1616 x 24 +-6 window 30: 12330 / 551 / 5725 / 6054;  1618 x 20 +-6 window 100: 10464 / 512 / 3265 / 6687;  64 x 12 +-25: 327 / 6 / 305 / 16;
    322 x 250 clean, window 20000: 67331 / 260 / 66206 / 865."""
    l, r = SC.rendered_pair(w, h, amp, seed=1)
    prm = SC.params(speckle_window=window)
    _speckle_work(l, r, prm)
    got, d = _run(gpu_ctx, [(l, r)], prm)
    assert d["stereo_frame_filter_calls"] == 1 and d["stereo_strip_filter_calls"] == 0
    assert _error_mask(gpu_ctx[0]) == 0, "a bounded union-find walk of the whole-frame filter gave up"
    _assert_equal(got, [(l, r)], prm)


def test_frame_filter_huge_window_filters_everything(gpu_ctx):
    """window 20000 on 96 x 80 (+-25): no component is that large -- the expected result is a frame without a single disparity (oracle: 2982 valid pixels go in,
    0 come out), through the whole-frame path"""
    import oracle as O
    l, r = SC.rendered_pair(96, 80, 25, seed=1)
    prm = SC.params(speckle_window=20000)
    c = SC.counts(l, r, prm)
    assert c[0] - c[1] > 2000 and c[2] == 0
    got, d = _run(gpu_ctx, [(l, r)], prm)
    assert d["stereo_frame_filter_calls"] == 1 and d["stereo_strip_filter_calls"] == 0
    assert (got[0] == -1).all() and np.array_equal(got[0], O.stereo_bm(l, r, prm))


# ---- b. the two speckle filters on the same frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,amp,seed", [(96, 80, 25, 2), (101, 61, 25, 2), (322, 250, 12, 1), (640, 48, 12, 1)])
def test_frame_filter_forced_against_strip_filter(gpu_ctx, monkeypatch, w, h, amp, seed):
    """the same frame through the strip filter (as dispatched) and through the whole-frame filter (SVS_STEREO_FRAME_CCL=1): both equal the oracle, the counters
    show two different paths.  322 x 250 is 4 strips of 68 rows and 640 x 48 is 2 of 37 as dispatched; the two small frames are one strip.
    Oracle alone (valid / removed by LR / kept / removed by speckle; small components across a strip boundary): 96 x 80 +-25: 2945 / 138 / 1881 / 926;
    101 x 61 +-25: 2491 / 62 / 1885 / 544;  322 x 250 +-12: 44371 / 1346 / 37477 / 5548, 20 across;  640 x 48 +-12: 13433 / 748 / 7298 / 5387, 30 across."""
    l, r = SC.rendered_pair(w, h, amp, seed=seed)
    prm = SC.params()
    _speckle_work(l, r, prm)
    _lr_work(l, r, prm)
    rows, n_strips = strips_of(w, h)
    if n_strips > 1:
        _straddling(l, r, prm, rows)
    got, d = _run(gpu_ctx, [(l, r)], prm)
    assert d["stereo_strip_filter_calls"] == 1 and d["stereo_frame_filter_calls"] == 0 and d["stereo_strip_filter_strips"] == n_strips
    _assert_equal(got, [(l, r)], prm, "strip filter,")
    monkeypatch.setenv("SVS_STEREO_FRAME_CCL", "1")
    got2, d2 = _run(gpu_ctx, [(l, r)], prm)
    assert d2["stereo_frame_filter_calls"] == 1 and d2["stereo_strip_filter_calls"] == 0
    assert _error_mask(gpu_ctx[0]) == 0, "a bounded union-find walk of the whole-frame filter gave up"      # (_run has asserted it already: said again where it matters)
    _assert_equal(got2, [(l, r)], prm, "whole-frame filter,")


# ---- c. many small strips -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,amp,seed", [(96, 80, 25, 2), (101, 61, 25, 10), (96, 80, 12, 6), (101, 61, 12, 14)])
def test_strip_filter_many_small_strips(gpu_ctx, monkeypatch, w, h, amp, seed):
    """SVS_STEREO_STRIP_KB=16: strips of 18 rows (96 wide, 5 strips) and 17 rows (101 wide, 4 strips), windows 1, 30, 100, 1000 x ranges 8, 32.  Window 1000
    is more than half a strip: whatever touches a boundary stays undecided and goes through stereo_speckle_merge_kernel / stereo_speckle_resolve_kernel.
    Oracle alone, per (window, range) in the order of the loops, (kept % of the frame, pixels removed by the speckle stage, components of <= window pixels across a
    strip boundary):
      96 x 80 +-25 seed 2:   (35.4, 85, 0) (35.5, 78, 0) (27.8, 674, 11) (27.8, 669, 11) (24.5, 928, 11) (24.5, 926, 11) (24.5, 928, 11) (24.5, 926, 11)
      101 x 61 +-25 seed 10: (37.5, 67, 0) (37.5, 64, 0) (30.9, 473, 7) (31.0, 464, 6) (27.3, 693, 8) (28.0, 653, 7) (27.3, 693, 8) (28.0, 653, 7)
      96 x 80 +-12 seed 6:   (53.0, 36, 0) (53.1, 32, 0) (50.4, 238, 4) (50.4, 236, 4) (50.4, 238, 4) (50.4, 236, 4) (50.4, 238, 4) (50.4, 236, 4)
      101 x 61 +-12 seed 14: (58.4, 14, 0) (58.4, 13, 0) (56.3, 140, 4) (56.4, 136, 4) (56.3, 140, 4) (56.4, 136, 4) (56.3, 140, 4) (56.4, 136, 4)
    Asserted per combination: >= 5 % kept; for the windows >= 30, >= 1 % removed and >= 4 components across a boundary (the seeds are chosen so that the oracle's
    output has them: with +-12 most seeds give 1-3).  Window 1 cannot meet two of the conditions on these inputs and is asked for their nearest form:
      * a component of one pixel cannot lie across a boundary: the test counts the single-pixel components ON the rows next to a boundary instead (the ones the
        strip filter has to leave undecided): 7 / 6 (range 8 / 32), 4 / 4, 3 / 3, 2 / 2 in the order of the cases above; asked: >= 4 with +-25, >= 1 with +-12;
      * window 1 removes >= 1 % of the frame only with +-25 of noise (asserted there).  With +-12 it removes 0.1-0.5 % -- at most 31 px of the 62 needed at 101 x 61
        over the noise seeds 1..40 at each of four camera poses -- so there the test asks for >= 8 px."""
    monkeypatch.setenv("SVS_STEREO_STRIP_KB", "16")
    rows, n_strips = strips_of(w, h, 16)
    assert (rows, n_strips) == {96: (18, 5), 101: (17, 4)}[w]
    l, r = SC.rendered_pair(w, h, amp, seed=seed)
    for window in (1, 30, 100, 1000):
        for rng in (8, 32):
            prm = SC.params(speckle_window=window, speckle_range=rng)
            if window == 1:
                c = _speckle_work(l, r, prm, remove=0.01 if amp == 25 else 0.0)
                assert c[3] >= 8, c
                val, fin = SC.stages(l, r, prm)[1:]
                gone = (val != -16) & (fin == -16)      # the single-pixel components
                edge = np.zeros(h, bool)
                edge[rows - 1::rows] = edge[rows::rows] = True
                assert gone[edge].sum() >= (4 if amp == 25 else 1), gone[edge].sum()
            else:
                _speckle_work(l, r, prm)
                _straddling(l, r, prm, rows)
            got, d = _run(gpu_ctx, [(l, r)], prm)
            assert d["stereo_strip_filter_calls"] == 1 and d["stereo_frame_filter_calls"] == 0 and d["stereo_strip_filter_strips"] == n_strips
            _assert_equal(got, [(l, r)], prm, f"window {window} range {rng},")


def test_strip_filter_wide_rows_in_several_strips(gpu_ctx, monkeypatch):
    """752 pixels are 12 segments of 64: more than the 10 the strip kernel's run pass holds in registers, so this is its stepwise pass (and the passes after it without
    the per-row masks), which 640-wide frames never take.  SVS_STEREO_STRIP_KB=71 makes strips of 16 rows: 752 x 50 is 4 strips (the last of 2 rows).
    Oracle alone, +-6: 21680 valid / 527 removed by LR / 17455 kept / 3698 removed by speckle; 78 small components across a strip boundary."""
    monkeypatch.setenv("SVS_STEREO_STRIP_KB", "71")
    w, h = 752, 50
    assert strips_of(w, h, 71) == (16, 4) and spk_row_bytes(w) == 752 * 6
    l, r = SC.rendered_pair(w, h, 6, seed=1)
    prm = SC.params()
    _speckle_work(l, r, prm)
    _lr_work(l, r, prm)
    _straddling(l, r, prm, 16)
    got, d = _run(gpu_ctx, [(l, r)], prm)
    assert d["stereo_strip_filter_calls"] == 1 and d["stereo_frame_filter_calls"] == 0 and d["stereo_strip_filter_strips"] == 4
    _assert_equal(got, [(l, r)], prm)


# ---- d. the parameters, on the path 640 x 480 takes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(96, 80), (203, 97)])
def test_parameters_on_the_default_path(gpu_ctx, w, h):
    """the 20 parameter sets that tests/test_oracle_cpu.py pins to the NumPy model (stereo_cases.covering_grid: every value of uniqueness_ratio {0, 5, 15, 60},
    texture_threshold {0, 10, 400}, disp12_max_diff {-1, 0, 1, 4}, speckle_window {0, 1, 30, 100, 3000}, speckle_range {0, 8, 32, 512}, every pair within a stage),
    with prefilter_cap 31 (SADs below 4096: 16-bit keys in the winner search) and 63 (32-bit keys) in turn -- every uniqueness value meets both.  One strip each:
    the strip filter whenever the speckle stage is on.  +-25 of noise, seed 2.  Not every set has work for every stage (range 0 with a window >= 30, window 3000 and
    texture_threshold 400 leave nothing on these inputs), so the sets that have are counted -- oracle alone, of the 20: the speckle stage keeps >= 5 % and removes >= 1 %
    of the frame in 7 sets (96 x 80) / 8 sets (203 x 97); the left-right check removes >= 10 px in 13 / 13 of the 15 sets that have it on."""
    grid = SC.covering_grid()
    l, r = SC.rendered_pair(w, h, 25, seed=2)
    n_speckle = n_lr = 0
    seen = set()
    for i, g in enumerate(grid):
        prm = SC.params(prefilter_cap=(31, 63)[i % 2], **g)
        seen.add((prm.prefilter_cap, prm.uniqueness_ratio))
        c = SC.counts(l, r, prm)
        n_speckle += c[2] >= 0.05 * l.size and c[3] >= 0.01 * l.size
        n_lr += c[1] >= 10
        got, d = _run(gpu_ctx, [(l, r)], prm)
        on = prm.speckle_window > 0
        assert d["stereo_strip_filter_calls"] == int(on) and d["stereo_frame_filter_calls"] == 0 and d["stereo_validate_wide_calls"] == 0
        _assert_equal(got, [(l, r)], prm, f"{g} cap {prm.prefilter_cap},")
    assert {(c, u) for c in (31, 63) for u in SC.UNIQUENESS} <= seen
    assert n_speckle >= SPECKLE_SETS[w] and n_lr >= LR_SETS[w], (n_speckle, n_lr)


SPECKLE_SETS = {96: 7, 203: 8}      # sets with work for the stage, counted on the oracle's output (docstring above)
LR_SETS = {96: 13, 203: 13}


# ---- e. the left-right check of rows wider than 2048 pixels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2052, 2054])
def test_wide_left_right_check(gpu_ctx, w):
    """one row per workgroup (w > 2048), four pixels per lane and load (w % 4 = 0) and one (w % 4 = 2); first without the speckle filter -- the check's output as it
    is -- then with it (window 30; 8 rows: the whole-frame path).  Oracle alone, clean rendered pair: 2052 x 8: 7372 valid, the check removes 284, the speckle
    filter keeps 3854 and removes 3234;  2054 x 8: 7625 / 326 / 4217 / 3082."""
    l, r = SC.rendered_pair(w, 8, 0)
    for window in (0, 30):
        prm = SC.params(speckle_window=window)
        _lr_work(l, r, prm)
        if window:
            _speckle_work(l, r, prm)
        got, d = _run(gpu_ctx, [(l, r)], prm)
        assert d["stereo_validate_wide_calls"] == 1 and d["stereo_frame_filter_calls"] == int(window > 0) and d["stereo_strip_filter_calls"] == 0
        _assert_equal(got, [(l, r)], prm, f"window {window},")


# ---- f. the prefilter kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [64, 160, 320])
def test_prefilter_kernels_on_aligned_rows(gpu_ctx, monkeypatch, w):
    """rows of 16 n pixels on aligned buffers: stereo_prefilter16_kernel as dispatched, stereo_prefilter_kernel under SVS_STEREO_PREFILTER4=1; both equal the oracle
    (h = 42 and 41: a last row group of 2 rows and of 1, the odd height's flat last row).  Two frames per call: the noisy pair and the clean one."""
    for h in (42, 41):
        pairs = [SC.rendered_pair(w, h, 12, seed=1), SC.rendered_pair(w, h, 0)]
        prm = SC.params()
        got, d = _run(gpu_ctx, pairs, prm)
        assert d["stereo_prefilter16_calls"] == 1 and d["stereo_prefilter4_calls"] == 0
        refs = _assert_equal(got, pairs, prm, "16-pixel kernel,")
        assert min((ref >= 0).mean() for ref in refs) > 0.05
        with monkeypatch.context() as m:
            m.setenv("SVS_STEREO_PREFILTER4", "1")
            got, d = _run(gpu_ctx, pairs, prm)
        assert d["stereo_prefilter4_calls"] == 1 and d["stereo_prefilter16_calls"] == 0
        _assert_equal(got, pairs, prm, "4-pixel kernel,")


@pytest.mark.parametrize("off", [1, 2, 3])
def test_prefilter_unaligned_pointers_and_three_strides(gpu_ctx, off):
    """svs_stereo_compute on raw buffers: left and right pointers `off` and (off % 3) + 1 bytes past a 16-byte boundary, strides w + 1 / w + 7 / w + 5 (none a multiple
    of 4), slack between the batch slots, a handle of 3 slots called with 2 frames.  160 x 41: the width alone would allow the 16-pixel kernel, so the generic one must be
    chosen for the alignment.  The result equals the oracle, does not depend on what stands in the padding of the inputs (two fills), and nothing outside the 2 x h x w
    result is written: row padding, slot gaps, the third slot, the guards (_compute)."""
    w, h = 160, 41
    pairs = [SC.rendered_pair(w, h, 12, seed=1), SC.noise_roll_pair(w, h, 7, seed=off)]
    prm = SC.params()
    layout = dict(strides=(w + 1, w + 7, w + 5), offsets=(off, off % 3 + 1), slack=(3, 9, 6), dguard=33)
    got, d = _run(gpu_ctx, pairs, prm, max_batch=3, fill_seed=1, **layout)
    assert d["stereo_prefilter4_calls"] == 1 and d["stereo_prefilter16_calls"] == 0
    refs = _assert_equal(got, pairs, prm)
    assert min((ref >= 0).mean() for ref in refs) > 0.05
    got2, _ = _run(gpu_ctx, pairs, prm, max_batch=3, fill_seed=2, **layout)
    assert all(np.array_equal(a, b) for a, b in zip(got, got2))


# ---- g. nothing outside the frame is written, nothing outside it is read ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,strip_kb,dstride,dguard", [(96, 80, 16, 108, 32), (96, 80, 16, 108, 33), (101, 61, 16, 106, 32), (64, 12, None, 76, 33), (1618, 20, None, 1623, 32)])
def test_output_and_input_padding(gpu_ctx, monkeypatch, w, h, strip_kb, dstride, dguard):
    """a multi-strip handle (5 strips of 96 x 80 with the 16-byte stores of the strip kernel's conversion -- output rows of 108 floats on a 16-byte aligned buffer --
    and with the same rows 4 bytes off that alignment; 4 strips of 101 x 61, single stores) and a whole-frame handle (stereo_finish4_kernel on 64 x 12,
    stereo_finish_kernel on 1618 x 20): 3 slots, 2 frames, a sentinel in every float of the output buffer.  _compute asserts that only the 2 x h x w rectangle changed;
    two different fills of the input padding give the same, correct result."""
    if strip_kb:
        monkeypatch.setenv("SVS_STEREO_STRIP_KB", str(strip_kb))
    amp = 25 if w < 200 else 6
    prm = SC.params()
    pairs = [SC.rendered_pair(w, h, amp, seed=2), SC.rendered_pair(w, h, amp, seed=3)]
    layout = dict(strides=(w + 8, w + 4, dstride), slack=(16, 4, 8 if dstride % 4 == 0 else 7), dguard=dguard)
    got, d = _run(gpu_ctx, pairs, prm, max_batch=3, fill_seed=1, **layout)
    assert d["stereo_strip_filter_calls"] == int(bool(strip_kb)) and d["stereo_frame_filter_calls"] == int(not strip_kb)
    refs = _assert_equal(got, pairs, prm)
    assert max((ref >= 0).mean() for ref in refs) > 0.05
    got2, _ = _run(gpu_ctx, pairs, prm, max_batch=3, fill_seed=2, **layout)
    assert all(np.array_equal(a, b) for a, b in zip(got, got2))


# ---- h. the tile edges of the block-matching kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(98, 97), (99, 102), (162, 65), (38, 2), (39, 3), (38, 16), (41, 20)])
def test_block_matching_tile_edges(gpu_ctx, w, h):
    """stereo_bm_kernel gives a wave 64 output columns and 96 rows, stereo_bm_edge_kernel a workgroup 64 rows of the three leftmost columns: 98 and 99 wide are
    exactly one wave of columns and one column more, 97 and 102 rows one strip of rows plus 1 and plus 6, 65 rows one edge block plus 1; 38 is the narrowest frame
    (only the edge kernel's columns exist), heights 2 and 3 the shortest (3: the flat last row of odd heights), 41 wide has one column for the wave kernel.
    Inputs: the rendered pair, and noise against its own roll by 0, 1, 30 and 31 pixels -- winners at both ends of the search range, where the parabola mirrors its
    missing neighbour.  Reference parameters, and the same frames without left-right check and speckle filter (the frames of a few rows are smaller than the speckle
    window: with it they come out empty): in that raw output of the oracle at least 40 % of the searched pixels of every roll pair lie within half a pixel of its
    shift (measured: 98 % and more on the three larger frames, 43 % at 38 x 2 with shift 31, where 7 columns x 2 rows are searched)."""
    shifts = (0, 1, 30, 31)
    pairs = [SC.rendered_pair(w, h, 0)] + [SC.noise_roll_pair(w, h, s, seed=w + s) for s in shifts]
    for prm in (SC.params(), SC.params(disp12_max_diff=-1, speckle_window=0)):
        got, d = _run(gpu_ctx, pairs, prm)
        refs = _assert_equal(got, pairs, prm)
        if prm.speckle_window == 0:
            for s, ref in zip(shifts, refs[1:]):
                assert (np.abs(ref[:, 31:] - s) <= 0.5).mean() >= 0.4, (s, (np.abs(ref[:, 31:] - s) <= 0.5).mean())


# ---- i. one handle, changing frames -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,strip_kb", [(96, 80, 16), (101, 61, 16), (1618, 20, None)])
def test_one_handle_on_changing_frames(gpu_ctx, monkeypatch, w, h, strip_kb):
    """the label / count / boundary-row / pending-list buffers of a handle persist across calls: four calls on one handle of 3 slots with 3, 1, 2 and 3 frames, no
    frame used twice (noise +-25 and +-12 alternating, seeds 20..28), every call equal to the oracle on its own frames -- nothing a slot held before shows.  A
    multi-strip handle (5 / 4 strips) and a whole-frame one."""
    if strip_kb:
        monkeypatch.setenv("SVS_STEREO_STRIP_KB", str(strip_kb))
    ctx, _ = gpu_ctx
    prm = SC.params()
    seed = 20
    with Handle(ctx, w, h, 3, prm) as hd:
        for n in (3, 1, 2, 3):
            pairs = []
            for _ in range(n):
                pairs.append(SC.rendered_pair(w, h, (25, 12)[seed % 2] if w < 200 else 6, seed=seed))
                seed += 1
            before = _stats(ctx)
            got = _compute(gpu_ctx, hd, pairs)
            after = _stats(ctx)
            assert _error_mask(ctx) == 0
            assert after["stereo_strip_filter_calls"] - before["stereo_strip_filter_calls"] == int(bool(strip_kb))
            assert after["stereo_frame_filter_calls"] - before["stereo_frame_filter_calls"] == int(not strip_kb)
            refs = _assert_equal(got, pairs, prm, f"call with {n} frames,")
            assert max((ref >= 0).mean() for ref in refs) > 0.05


# ---- svs_stereo_create refuses what svs_stereo_compute could not launch ------------------------------------------------------------------------------------------
def test_create_refuses_rows_that_do_not_fit_lds(gpu_ctx):
    """stereo_ccl_runs_kernel asks for 8 w + 8 ceil(w / 64) bytes of LDS and stereo_validate_kernel for 8 w (w > 2048); a workgroup has 160 KB, so
    20164 pixels is the widest row: 8 * 20164 + 8 * 316 = 163840.  One pixel more is SVS_ERR_UNSUPPORTED with the bound in the message and nothing allocated; at the
    bound a frame of 4 rows goes through the left-right check and the speckle filter (window 10) and equals the oracle.
    Oracle alone at 20164 x 4, clean rendered pair: 24969 valid, the check removes 2559, the speckle filter keeps 6281 and removes 16129 of 80656 px."""
    ctx, _ = gpu_ctx
    assert 8 * MAX_W + 8 * ((MAX_W + 63) // 64) <= 160 * 1024 < 8 * (MAX_W + 1) + 8 * ((MAX_W + 64) // 64)
    prm = SC.params(speckle_window=10)
    live = ctx.get_stat("live_device_bytes")
    h_ = C.c_void_p()
    rc = ctx.lib.svs_stereo_create(ctx.h, MAX_W + 1, 4, 1, C.byref(prm), C.byref(h_))
    assert rc == SVS_ERR_UNSUPPORTED and not h_.value
    assert str(MAX_W) in ctx.lib.svs_last_error(ctx.h).decode()
    assert ctx.get_stat("live_device_bytes") == live
    l, r = SC.rendered_pair(MAX_W, 4, 0)
    _lr_work(l, r, prm)
    _speckle_work(l, r, prm)
    got, d = _run(gpu_ctx, [(l, r)], prm)
    assert d["stereo_validate_wide_calls"] == 1 and d["stereo_frame_filter_calls"] == 1 and d["stereo_strip_filter_calls"] == 0
    _assert_equal(got, [(l, r)], prm)
    # the LDS a kernel may ask for is a property of the kernel, not of a handle: a narrower handle (9000 pixels: 72 KB) created AFTER the widest one must not take
    # away what that one needs at launch
    with Handle(ctx, MAX_W, 4, 1, prm) as wide, Handle(ctx, 9000, 4, 1, prm):
        _assert_equal(_compute(gpu_ctx, wide, [(l, r)]), [(l, r)], prm, "after a narrower handle was created,")
    assert _error_mask(ctx) == 0
