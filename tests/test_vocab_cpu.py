"""The restatement of svs_vocab_train (tests/vocab_model.py) against itself, and the preconditions of tests/test_gpu_vocab.py on the model: no GPU."""
import os
import re

import numpy as np

import place_model as M
import vocab_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_updates_are_equal():
    for K, s, N, k in ((64, 1, 300, 17), (128, 6, 120, 9)):
        X = V.case_points(K, s, N)
        words = X[:k].copy()
        words[k - 1] = 3.5                                    # far from every point: a word without members keeps its centre
        a, _, _ = V.assign(X, words)
        w1, c1 = V.update_add_at(X, a, words)
        w2, c2 = V.update_python(X, a, words)
        assert c1[k - 1] == 0 and np.array_equal(w1[k - 1], words[k - 1])
        assert np.array_equal(c1, c2) and np.array_equal(w1.view(np.uint32), w2.view(np.uint32))
        assert not np.array_equal(w1[:k - 1], words[:k - 1])


def test_seeds_are_pairwise_distinct_on_distinct_points():
    for K, s, N, k in ((64, 1, 700, 24), (128, 6, 333, 33), (64, 2, 40, 40)):
        X = V.case_points(K, s, N)
        assert len(np.unique(X, axis=0)) == N
        idx, ns = V.seed_kmeanspp(X, k, 99 + s)
        assert ns == k and len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < N
        assert idx[0] == V.first_index(99 + s, N)


def test_total_zero_ends_the_seeding_on_duplicates():
    rows = V.case_points(64, 3, 5)
    X = np.repeat(rows, 7, axis=0)[np.random.default_rng(0).permutation(35)]
    idx, ns = V.seed_kmeanspp(X, 9, 4)
    assert ns == 5 and (idx[5:] == -1).all() and len(np.unique(X[idx[:5]], axis=0)) == 5
    idx, ns = V.seed_kmeanspp(np.repeat(rows[:1], 50, axis=0), 4, 4)
    assert ns == 1 and idx[0] == V.first_index(4, 50) and (idx[1:] == -1).all()
    r = V.train(np.repeat(rows[:1], 50, axis=0), 4, 3, 4)
    assert r["n_seeded"] == 1 and len(r["words"]) == 1 and r["iterations_run"] == 2 and r["converged"] and (r["assign"] == 0).all()


def test_inertia_does_not_rise():
    """Lloyd: each step lowers the sum unless the rounding of a centre to f32 raises it, by at most count K (2^-24 |c|)^2 per word"""
    for name, K, s, N, nw, ts in V.RUN_CASES:
        X, r = V.case_run(name)
        tol = N * K * 2.0 ** -44
        assert len(r["inertia"]) == r["iterations_run"] >= 3
        for a, b in zip(r["inertia"], r["inertia"][1:]):
            assert b <= a + tol, (name, a, b)
        assert r["inertia"][-1] < r["inertia"][0]


def test_preconditions_of_the_gpu_cases_hold_on_the_model():
    want = {"k64-s1": (11, True, 0), "k64-s2": (8, True, 0), "k64-s3": (8, True, 0), "k128-s6": (4, True, 1)}
    for name, K, s, N, nw, ts in V.RUN_CASES:
        X, r = V.case_run(name)
        print(name, "smallest gap / 2B", min(r["gaps"]), "iterations", r["iterations_run"], "empty", r["n_empty"])
        assert min(r["gaps"]) > 1.0, name                     # the near-tie band is empty in every assignment made
        assert (r["iterations_run"], r["converged"], r["n_empty"]) == want[name], name
        assert r["n_seeded"] == nw and len(r["words"]) == nw - r["n_empty"]
        assert N % 64 and N % 256 and r["changed"][0] == N
    _, keep = V.case_run("k128-s6", False)
    assert len(keep["words"]) == 33 and int((keep["count"] == 0).sum()) >= 1 and min(keep["gaps"]) > 1.0
    X, init = V.case_chunks()
    r = V.train(X, len(init), 1, 0, init=init, drop_empty=False)
    assert len(init) == 257 and min(r["gaps"]) > 1.0 and r["n_empty"] == 20 and r["assign"].max() == 256      # the second chunk of words is reached
    X, nw, ts = V.case_large()
    r = V.train(X, nw, 11, ts, drop_empty=False)
    assert min(r["gaps"]) < 1.0 and r["n_seeded"] == nw      # near-ties are certain: this case is held to the 2 B band, not to equality


def test_header_declares_the_trainer_and_capi_binds_it():
    from scavislam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("svs_vocab_train", "svs_vocab_params_default", "svs_vocab_stage_times"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS
    assert "svs_vocab_train" in capi._SIGS and len(capi._SIGS["svs_vocab_train"]) == 12
    lib = capi.load()
    from scavislam_amd.ctypes_types import VocabParams
    p = VocabParams()
    lib.svs_vocab_params_default(__import__("ctypes").byref(p))
    assert (p.n_words, p.iterations, p.seed, p.h_init, p.drop_empty) == (10000, 11, 0, None, 1)
    from scavislam_amd.loop import train_vocabulary      # noqa: F401
    assert M.fixture_words().shape == (1024, 64)
