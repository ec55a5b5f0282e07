"""Input shared by the block-matching tests at disparity counts other than 32 (tests/test_stereo_ndisp_cpu.py: oracle against the NumPy model;
tests/test_gpu_stereo_ndisp.py: the HIP kernels against the oracle).  The rendered pairs of tests/stereo_cases.py never reach disparity 32, so a search over N > 32
disparities would find all of its winners in the part of the range the 32-disparity kernels already cover.  Here the winners are spread over the whole range:
bands of nine rows of one noise image, each rolled by its own shift between 0 and N - 1."""
import functools

import numpy as np

import stereo_cases as SC

BAND = 9
NOISE = 6
# stereo_cases.counts of tests/np_model.py alone on banded_pair(N) at the reference parameters: (valid after block matching, removed by the left-right check,
# kept by the speckle filter, removed by the speckle filter), and how many of the kept values are >= 32 pixels
MODEL_COUNTS = {16: (6802, 10, 6672, 120, 0), 48: (6618, 59, 6425, 134, 1756), 64: (6390, 39, 6177, 174, 2848), 160: (6222, 30, 5949, 243, 4322)}


def size_for(ndisp):
    """(w, h) of the full cases: 72 x 101 = 7272 searched pixels"""
    return ndisp + 71, 101


def band_shifts(ndisp, h):
    n_bands = (h + BAND - 1) // BAND
    return [k * (ndisp - 1) // max(n_bands - 1, 1) for k in range(n_bands)]


@functools.lru_cache(maxsize=None)
def _banded(ndisp, w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    r = a.copy()
    for k, s in enumerate(band_shifts(ndisp, h)):
        r[BAND * k:BAND * (k + 1)] = np.roll(a[BAND * k:BAND * (k + 1)], -s, axis=1)
    r = np.clip(r.astype(np.int32) + rng.integers(-NOISE, NOISE + 1, r.shape), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    r.setflags(write=False)
    return a, r


def banded_pair(ndisp, w=None, h=None, seed=0):
    """left: noise; right: band k (rows 9 k .. 9 k + 8) is the left band rolled s_k = k (N - 1) // (n_bands - 1) pixels to the left -- the first band's winner is
    disparity 0, the last band's N - 1 -- plus uniform integer noise of +-6 on the right image, clipped"""
    fw, fh = size_for(ndisp)
    return _banded(ndisp, w or fw, h or fh, seed)


def params(ndisp, **kw):
    return SC.params(num_disparities=ndisp, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_stages(ndisp, w, h, seed, key):
    l, r = _banded(ndisp, w, h, seed)
    return SC.stages(l, r, params(ndisp, **dict(key)))


def oracle_stages(ndisp, w=None, h=None, seed=0, **kw):
    """the oracle's (raw, after the left-right check, after the speckle filter) 16-bit planes of banded_pair, computed once per case and shared"""
    fw, fh = size_for(ndisp)
    return _oracle_stages(ndisp, w or fw, h or fh, seed, tuple(sorted(kw.items())))


def work(stages, ndisp):
    """(valid after block matching, removed by the left-right check, kept, removed by the speckle filter, kept values >= 32 pixels)"""
    d16, val, fin = stages
    return (int((d16 != -16).sum()), int((d16 != -16).sum() - (val != -16).sum()), int((fin != -16).sum()), int((val != -16).sum() - (fin != -16).sum()),
            int((fin >= 32 * 16).sum()))


def assert_has_work(stages, ndisp):
    """on the ORACLE's output alone, before anything is compared: the case has work for every stage, and for N >= 48 beyond what 32 disparities reach"""
    c = work(stages, ndisp)
    assert c[0] >= 5000 and c[1] >= 5 and c[3] >= 100, f"vacuous case at {ndisp} disparities: {c}"
    assert ndisp < 48 or c[4] >= 1000, f"{ndisp} disparities: only {c[4]} final values >= 32"
    return c
