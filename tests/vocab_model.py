"""NumPy / Python-integer restatement of svs_vocab_train (k-means++ seeding, Lloyd iterations with fixed-point sums): the yardstick of tests/test_vocab_cpu.py
and tests/test_gpu_vocab.py.  Written from the header's text (include/scavislam_hip.h, svs_vocab_train), not from the kernels:

  seed_kmeanspp()   the seeding: f64 weights in component order, uint64 fixed-point weights, the counter-based draw, the prefix search
  assign()          the exact nearest centre on f64 distances (loop_model.sqdist) with the bound of an f32 chain (loop_model.match_bound)
  update_add_at()   the fixed-point update with np.add.at on int64
  update_python()   the same with plain Python integers: an independent second restatement
  train()           the whole call
  case_*()          the seeded inputs of the GPU tests
"""
import functools

import numpy as np

import loop_model as L
import place_model as M

M64 = L.M64
W_SCALE = 2.0 ** 28          # weights and inertia
Q_SCALE = 2.0 ** 38          # components
F32 = np.float32


def mulhi32(a, b):
    return (a * b) >> 32


def mulhi64(a, b):
    return (a * b) >> 64


# ---- seeding -------------------------------------------------------------------------------------------------------------------------------------------------
def seq_sqdist(X, y):
    """s = 0.0; for k: d = (double)x[k] - (double)y[k]; s = s + d * d -- for every row of X, in component order"""
    X = np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    s = np.zeros(len(X))
    for k in range(X.shape[1]):
        d = X[:, k] - y[k]
        s = s + d * d
    return s


def first_index(seed, n):
    return mulhi32(L.splitmix64(seed & M64) >> 32, n)


def seed_kmeanspp(X, n_words, seed):
    """(seed_index [n_words] with -1 behind n_seeded, n_seeded)"""
    X = np.asarray(X, np.float32)
    n = len(X)
    idx = np.full(n_words, -1, np.int32)
    idx[0] = first_index(seed, n)
    w = np.full(n, np.inf)
    for c in range(1, n_words):
        last = int(idx[c - 1])
        w = np.minimum(w, seq_sqdist(X, X[last]))
        w[last] = 0.0
        W = (w * W_SCALE).astype(np.uint64)                      # truncation; < 2^41 each
        cs = np.cumsum(W, dtype=np.uint64)                       # < 2^62: exact
        T = int(cs[-1])
        assert T == sum(int(v) for v in W)
        if T == 0:
            return idx, c
        r = mulhi64(L.splitmix64((seed ^ ((1 << 62) | c)) & M64), T)
        idx[c] = int(np.searchsorted(cs, np.uint64(r), side="right"))      # the smallest i whose inclusive prefix sum exceeds r
    return idx, n_words


# ---- assignment ----------------------------------------------------------------------------------------------------------------------------------------------
def assign(X, words):
    """word [n] (the lowest index of the minimum), the f64 distance matrix D and the bound B [n] of an f32 chain"""
    D = L.sqdist(X, words)
    return np.argmin(D, axis=1).astype(np.int32), D, L.match_bound(X, words)


def gap_ratio(D, B):
    """min over the points of (second best - best) / (2 B): above 1, the near-tie band is empty and the device's words must EQUAL the model's"""
    if D.shape[1] < 2:
        return np.inf
    srt = np.sort(D, axis=1)
    return float(((srt[:, 1] - srt[:, 0]) / (2 * B)).min())


# ---- update --------------------------------------------------------------------------------------------------------------------------------------------------
def quantise(X):
    return np.rint(np.asarray(X, np.float32).astype(np.float64) * Q_SCALE).astype(np.int64)


def update_add_at(X, a, words):
    """(new words f32, count): c[k] = (float)(((double)sum_q / (double)count) * 2^-38); a word without members keeps its centre"""
    words = np.asarray(words, np.float32)
    sums = np.zeros(words.shape, np.int64)
    np.add.at(sums, a, quantise(X))
    cnt = np.bincount(a, minlength=len(words)).astype(np.int32)
    out = words.copy()
    m = cnt > 0
    out[m] = ((sums[m].astype(np.float64) / cnt[m].astype(np.float64)[:, None]) * (1.0 / Q_SCALE)).astype(np.float32)
    return out, cnt


def update_python(X, a, words):
    words = np.asarray(words, np.float32)
    k, K = words.shape
    sums = [[0] * K for _ in range(k)]
    cnt = [0] * k
    for i, x in enumerate(np.asarray(X, np.float32)):
        j = int(a[i])
        cnt[j] += 1
        row = sums[j]
        for c in range(K):
            row[c] += int(np.rint(float(x[c]) * Q_SCALE))
    out = words.copy()
    for j in range(k):
        if cnt[j]:
            for c in range(K):
                out[j, c] = F32((float(sums[j][c]) / float(cnt[j])) * (1.0 / Q_SCALE))
    return out, np.asarray(cnt, np.int32)


def inertia_q28(d2):
    """sum of (uint64)((double)d2 * 2^28) over f32 distances"""
    return sum(int(v) for v in (np.asarray(d2, np.float32).astype(np.float64) * W_SCALE).astype(np.uint64))


# ---- the call ------------------------------------------------------------------------------------------------------------------------------------------------
def train(X, n_words, iterations=11, seed=0, init=None, drop_empty=True, update=update_add_at):
    """dict: words, seed_index, n_seeded, assign, D (final f64 distances), B, count, changed, iterations_run, converged, n_empty, gaps (gap_ratio of every
    assignment made, the final one last), inertia (f64, of every iteration's assignment)"""
    X = np.asarray(X, np.float32)
    if init is None:
        sidx, n_seeded = seed_kmeanspp(X, n_words, seed)
        words = X[sidx[:n_seeded]].copy()
    else:
        sidx, n_seeded = np.full(n_words, -1, np.int32), 0
        words = np.asarray(init, np.float32).copy()
    prev = np.full(len(X), -1, np.int32)
    changed, gaps, inertia, cnt, converged = [], [], [], None, False
    for _ in range(iterations):
        a, D, B = assign(X, words)
        gaps.append(gap_ratio(D, B))
        inertia.append(float(D.min(axis=1).sum()))
        changed.append(int((a != prev).sum()))
        words, cnt = update(X, a, words)
        prev = a
        if changed[-1] == 0:
            converged = True
            break
    n_empty = 0
    if cnt is not None:
        n_empty = int((cnt == 0).sum())
        if drop_empty:
            words = words[cnt > 0]
    a, D, B = assign(X, words)
    gaps.append(gap_ratio(D, B))
    return dict(words=words, seed_index=sidx, n_seeded=n_seeded, assign=a, D=D, B=B, count=np.bincount(a, minlength=len(words)).astype(np.int32),
                changed=np.asarray(changed, np.int32), iterations_run=len(changed), converged=converged, n_empty=n_empty, gaps=gaps, inertia=inertia)


# ---- the scenarios -------------------------------------------------------------------------------------------------------------------------------------------
def unit_rows(seed, n, K):
    a = np.random.default_rng(seed).normal(size=(n, K))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def points(base, N, s):
    """N descriptors around rows of base: place_model.descriptors with default_rng(s)"""
    rng = np.random.default_rng(s)
    return np.ascontiguousarray(M.descriptors(rng, base, rng.integers(0, len(base), N)))


BASE128_SEED = 235         # of the 50 unit rows the K = 128 points lie around: the first seed whose run leaves a word EMPTY with the near-tie band empty
# (name, K, data seed, N, n_words, training seed)
RUN_CASES = [("k64-s1", 64, 1, 700, 24, 1235), ("k64-s2", 64, 2, 700, 24, 1236), ("k64-s3", 64, 3, 700, 24, 1237), ("k128-s6", 128, 6, 333, 33, 1240)]


def case_points(K, s, N):
    base = M.fixture_words()[:40] if K == 64 else unit_rows(BASE128_SEED, 50, 128)
    return points(base, N, s)


def case_chunks():
    """more than one vocabulary chunk: 257 caller-given centres, one iteration"""
    init = np.ascontiguousarray(M.fixture_words()[:257])
    return points(init, 700, 23), init


def case_large():
    return points(M.fixture_words()[:400], 2999, 31), 300, 77


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def case_run(name, drop_empty=True):
    """the model's run of a RUN_CASES entry: computed once, shared by the CPU and the GPU tests, read-only"""
    _, K, s, N, nw, ts = next(c for c in RUN_CASES if c[0] == name)
    X = case_points(K, s, N)
    X.setflags(write=False)
    return X, _freeze(train(X, nw, 11, ts, drop_empty=drop_empty))
