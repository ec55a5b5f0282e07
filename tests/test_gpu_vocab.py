"""svs_vocab_train (k-means++ seeding and Lloyd iterations on the device) against the restatement tests/vocab_model.py.

Bounds.  The seeding is integer arithmetic on f64 sums formed in a fixed order: the indices must be EQUAL.  The assignment is an f32 chain whose error
B_i = (K + 4) 2^-23 (|x_i|^2 + max_j |c_j|^2) bounds (loop_model.match_bound): where the model's best two distances are further apart than 2 B for every point
in every assignment of the run (asserted on the model as a PRECONDITION) the words of the points, and with them the fixed-point centres, must be EQUAL bit
for bit.  inertia_q28 is a sum over the device's own f32 distances: it is held EQUAL to the header's formula on h_assign_d2, and those distances are held to
the bound B against the model's."""
import os
import subprocess

import numpy as np
import pytest

import loop_model as L
import place_model as M
import vocab_model as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from scavislam_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def train(ctx, X, n_words, **kw):
    from scavislam_amd.loop import train_vocabulary
    return train_vocabulary(ctx, X, n_words, **kw)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_final_assignment(out, X, band_empty=True):
    """h_assign / h_assign_d2 / h_count / inertia_q28 against the words as returned.  band_empty: the case has no near-tie, the words are EQUAL to the model's;
    otherwise (raw seeds as words: a case the issue holds to its seed indices only) every choice lies inside the 2 B band"""
    a, D, B = V.assign(X, out.words)
    if band_empty:
        assert V.gap_ratio(D, B) > 1.0
        assert np.array_equal(out.assign, a)
    else:
        assert (D[np.arange(len(X)), out.assign] <= D.min(axis=1) + 2 * B).all()
        a = out.assign
    best = D[np.arange(len(X)), a]
    assert (np.abs(out.assign_d2.astype(np.float64) - best) <= B + 2.0 ** -22 * best).all()
    assert np.array_equal(out.count, np.bincount(a, minlength=len(out.words)))
    assert out.inertia_q28 == V.inertia_q28(out.assign_d2)
    assert (out.raw["words"][out.n_words_out:] == 0).all() and (out.raw["count"][out.n_words_out:] == 0).all()


# ---- 1. seeding ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,s,N,nw", [(64, 1, 700, 24), (128, 6, 333, 33)])
def test_seeding_equals_the_model(ctx, K, s, N, nw):
    X = V.case_points(K, s, N)
    for seed in (0, 1234 + s, 2 ** 64 - 1):
        out = train(ctx, X, nw, iterations=0, seed=seed)
        idx, ns = V.seed_kmeanspp(X, nw, seed)
        assert np.array_equal(out.seed_index, idx), seed
        assert (out.n_seeded, out.n_words_out, out.iterations_run, out.converged, out.n_empty) == (ns, nw, 0, False, 0)
        assert np.array_equal(u32(out.words), u32(X[idx]))
        assert len(out.changed) == 0
    assert_final_assignment(out, X, band_empty=False)


def test_seeding_ends_on_duplicates(ctx):
    rows = V.case_points(64, 3, 5)
    same = np.repeat(rows[:1], 333, axis=0)
    out = train(ctx, same, 7, iterations=3, seed=4)
    assert out.n_seeded == 1 and out.n_words_out == 1 and out.seed_index[0] == V.first_index(4, 333) and (out.seed_index[1:] == -1).all()
    assert (out.assign == 0).all() and out.count.tolist() == [333] and out.iterations_run == 2 and out.converged and out.changed.tolist() == [333, 0]
    X = np.repeat(rows, 67, axis=0)[np.random.default_rng(0).permutation(335)]
    out = train(ctx, X, 9, iterations=0, seed=4)
    idx, ns = V.seed_kmeanspp(X, 9, 4)
    assert ns == 5 and out.n_seeded == 5 and out.n_words_out == 5 and np.array_equal(out.seed_index, idx)


# ---- 2. whole runs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,drop", [("k64-s1", True), ("k64-s2", True), ("k64-s3", True), ("k128-s6", True), ("k128-s6", False)])
def test_whole_run_equals_the_model(ctx, name, drop):
    _, K, s, N, nw, ts = next(c for c in V.RUN_CASES if c[0] == name)
    X, m = V.case_run(name, drop)
    assert min(m["gaps"]) > 1.0, "precondition: a near-tie in the model's run (pick another seed, never a looser band)"
    out = train(ctx, X, nw, iterations=11, seed=ts, drop_empty=drop)
    print(name, "iterations", out.iterations_run, "changed", out.changed.tolist(), "empty", out.n_empty, "inertia_q28", out.inertia_q28)
    assert np.array_equal(out.seed_index, m["seed_index"]) and out.n_seeded == m["n_seeded"]
    assert (out.iterations_run, out.converged, out.n_empty) == (m["iterations_run"], m["converged"], m["n_empty"])
    assert np.array_equal(out.changed, m["changed"]) and (out.raw["changed"][out.iterations_run:] == -1).all()
    assert out.n_words_out == len(m["words"]) and np.array_equal(u32(out.words), u32(m["words"]))
    assert np.array_equal(out.assign, m["assign"]) and np.array_equal(out.count, m["count"])
    assert_final_assignment(out, X)
    if name == "k128-s6":
        assert out.n_empty == 1 and out.n_words_out == (32 if drop else 33)
    _cache[(name, drop)] = out.raw_bytes()


def test_more_than_one_chunk_of_words(ctx):
    X, init = V.case_chunks()
    m = V.train(X, len(init), 1, 0, init=init, drop_empty=False)
    assert min(m["gaps"]) > 1.0 and m["n_empty"] == 20
    out = train(ctx, X, len(init), iterations=1, init=init, drop_empty=False)
    assert (out.n_seeded, out.iterations_run, out.n_empty, out.n_words_out) == (0, 1, 20, 257) and (out.seed_index == -1).all() and out.changed.tolist() == [700]
    a0, _, _ = V.assign(X, init)                               # the iteration's assignment: the model's, hence (band empty) the device's
    w, cnt = V.update_python(X, a0, init)
    assert np.array_equal(u32(out.words), u32(w))
    empty = cnt == 0
    assert empty.sum() == 20 and np.array_equal(u32(out.words[empty]), u32(init[empty]))
    assert np.array_equal(out.assign, m["assign"]) and out.assign.max() >= 256
    assert_final_assignment(out, X)


# ---- 3. near-ties: one call = chained calls, every choice inside the band ---------------------------------------------------------------------------------------
def test_one_call_equals_eleven_chained_calls(ctx):
    X, nw, ts = V.case_large()
    one = train(ctx, X, nw, iterations=11, seed=ts, drop_empty=False)
    assert one.n_seeded == nw
    seeded = train(ctx, X, nw, iterations=0, seed=ts)         # its assignment is the one iteration 0 makes
    words, prev, chg = seeded.words, seeded.assign, []
    for t in range(11):
        out = train(ctx, X, nw, iterations=1, init=words, drop_empty=False)
        D = L.sqdist(X, out.words)
        B = L.match_bound(X, out.words)
        chosen = D[np.arange(len(X)), out.assign]
        assert (chosen <= D.min(axis=1) + 2 * B).all(), f"chained call {t}: a point's word is outside the 2 B band"
        chg.append(int((out.assign != prev).sum()))      # call t returns the assignment iteration t + 1 makes
        prev, words = out.assign, out.words
    r = one.iterations_run
    assert one.changed[1:].tolist() == chg[:r - 1]
    for key in ("words", "assign", "assign_d2", "count"):
        assert one.raw[key].tobytes() == out.raw[key].tobytes(), key
    assert one.inertia_q28 == out.inertia_q28 and one.n_empty == out.n_empty


# ---- 4. the index sees the same words ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k64-s1", "k128-s6"])
def test_index_assigns_the_same_words(ctx, name):
    from scavislam_amd.loop import GeometricChecker
    _, K, s, N, nw, ts = next(c for c in V.RUN_CASES if c[0] == name)
    X = V.case_points(K, s, N)
    out = train(ctx, X, nw, seed=ts)
    gc = GeometricChecker(ctx, L.CAM, desc_dim=K, max_desc=N, max_places=1, max_hyp=100, max_checks=1)
    gc.set_vocabulary(out.words)
    u = np.linspace(50.0, 400.0, N)
    gc.set_place(0, X, np.stack([u, u, u - 20.0], 1))
    loc = gc.add_locations([0], radius=float("inf"), do_loop_detection=False)[0]
    assert np.array_equal(loc.word, out.assign)
    assert np.array_equal(u32(loc.word_d2), u32(out.assign_d2))
    gc.close()


# ---- 5. repetition -----------------------------------------------------------------------------------------------------------------------------------------------
def test_another_context_gives_identical_bytes():
    from scavislam_amd import capi
    c2 = capi.Context(0)
    try:
        for name, drop in (("k64-s1", True), ("k128-s6", False)):
            _, K, s, N, nw, ts = next(c for c in V.RUN_CASES if c[0] == name)
            X = V.case_points(K, s, N)
            a = train(c2, X, nw, iterations=11, seed=ts, drop_empty=drop).raw_bytes()
            b = _cache.get((name, drop)) or train(c2, X, nw, iterations=11, seed=ts, drop_empty=drop).raw_bytes()
            assert a == b, name
    finally:
        c2.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import ctypes as C
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import VocabParams, VocabResult
    X = V.case_points(64, 1, 100)
    live = ctx.get_stat("live_device_bytes")

    def status(code, n=100, K=64, n_words=10, iterations=11, desc=X, init=None):
        prm = VocabParams(n_words, iterations, 0, None if init is None else init.ctypes.data, 1)
        res = VocabResult()
        with pytest.raises(SvsError) as e:
            ctx.call("svs_vocab_train", K, n, desc.ctypes.data, C.byref(prm), None, C.byref(res), None, None, None, None, None)
        assert str(e.value).startswith(f"status {code}:"), str(e.value)
        assert ctx.get_stat("live_device_bytes") == live      # refused before anything was allocated or uploaded

    status(1, K=32)
    status(1, K=96)
    status(1, n=0)
    status(1, n_words=0)
    status(1, n_words=101)
    status(1, iterations=-1)
    for bad in (np.nan, np.inf, -np.inf, 4.0, -4.0):
        Y = X.copy()
        Y[99, 63] = bad
        status(1, desc=Y)
        status(1, init=Y[90:100])
    status(4, n=(1 << 21) + 1)                                # (refused before h_desc is read)
    status(4, n=1 << 21, n_words=(1 << 20) + 1)
    Y = X.copy()
    Y[99, 63] = np.float32(3.9999998)                         # the largest component that is taken
    out = train(ctx, Y, 10, iterations=1)
    assert out.n_words_out == 10 and out.iterations_run == 1


# ---- 7. the C++ adaptor ------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_adaptor_prints_the_same_words(ctx, tmp_path):
    exe = tmp_path / "vocab_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vocab_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    X = V.case_points(64, 2, 700)
    with open(tmp_path / "vocab.bin", "wb") as f:
        f.write(np.array([64, 700, 24, 11], np.int32).tobytes())
        f.write(np.array([1236], np.uint64).tobytes())
        f.write(X.tobytes())
    lines = [l.split() for l in subprocess.check_output([str(exe), str(tmp_path / "vocab.bin")]).decode().splitlines()]
    out = train(ctx, X, 24, iterations=11, seed=1236)
    res = [l for l in lines if l[0] == "RES"][0]
    assert [int(t) for t in res[1:]] == [out.n_words_out, out.n_seeded, out.iterations_run, int(out.converged), out.n_empty, out.inertia_q28]
    words = np.array([[int(t, 16) for t in l[2:]] for l in lines if l[0] == "WORD"], np.uint32)
    assert words.shape == (24, 64) and np.array_equal(words, u32(out.words))
    assert M.fixture_words().shape[1] == 64
