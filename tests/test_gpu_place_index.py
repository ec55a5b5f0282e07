"""The place index on the device (svs_loop_set_vocabulary / svs_loop_add_locations: visual words, inverted index, TF-IDF scores; the front half of
PlaceRecognizer::addLocation) against the NumPy restatement tests/place_model.py.  The stages are judged separately: the model's index runs on the device's
own words.

Bounds.  Words: B_i = (K + 4) 2^-23 (|q_i|^2 + max_j |w_j|^2) (loop_model.match_bound) bounds the error of a K-term f32 chain.  Every case asserts as a
PRECONDITION, on the model, that no descriptor has its best two distances within 2 B of each other or its best within B of the radius: the bands are empty, so
the words must be EQUAL and no case is left out.  Scores: sequential f32 sums, quotient / product / sum rounded on their own -- compared as uint32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loop_model as L
import place_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 12
NQ = (67, 200, 330)          # none a multiple of the 32-query tile
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from scavislam_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def checker(ctx, K=64, max_desc=330, max_places=P, max_checks=P):
    from scavislam_amd.loop import GeometricChecker
    return GeometricChecker(ctx, L.CAM, desc_dim=K, max_desc=max_desc, max_places=max_places, max_hyp=100, max_checks=max_checks)


def unit_rows(seed, n, K):
    a = np.random.default_rng(seed).normal(size=(n, K))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def vocabulary(name):
    if name not in _cache:
        V = M.fixture_words()
        v = {"fixture1024": V, "fixture1000": V[:1000], "fixture129": V[:129], "seeded300x128": None, "seeded9983": None}[name]
        if name == "seeded300x128":
            v = unit_rows(31, 300, 128)
        if name == "seeded9983":
            v = unit_rows(32, 9983, 64)
        v = np.ascontiguousarray(v)
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name]


def scenario():
    """the twelve places on the fixture, shared and read-only"""
    if "scenario" not in _cache:
        pl = M.make_places(vocabulary("fixture1024"))
        for p in pl:
            for a in p.values():
                a.setflags(write=False)
        _cache["scenario"] = pl
    return _cache["scenario"]


def locs(places=range(P), **kw):
    return [dict(slot=p, exclude=M.excludes(p), **kw) for p in places]


def load_scenario(gc, places=None):
    gc.set_vocabulary(vocabulary("fixture1024"))
    for p, pl in enumerate(places or scenario()):
        gc.set_place(p, pl["desc"], pl["uvu"])


def model_run(outs, calls, max_places=P):
    """the literal model on the device's own words; calls: dicts as add_locations takes them"""
    ix = M.LiteralIndex(len(vocabulary("fixture1024")))
    return [ix.add_location(c["slot"], o.word, c.get("do_loop_detection", True), c.get("exclude", ())) for o, c in zip(outs, calls)]


def assert_equals_model(outs, model, max_places=P):
    for k, (o, m) in enumerate(zip(outs, model)):
        assert np.array_equal(o.scores.view(np.uint32), M.scores_row(m["stats"], max_places).view(np.uint32)), f"location {k}: scores differ"
        assert (o.number_of_words, o.n_scored, o.best_slot, o.candidate) == (m["number_of_words"], m["n_scored"], m["best_slot"], m["candidate"]), k
        assert np.float32(o.best_score).view(np.uint32) == np.float32(m["best_score"]).view(np.uint32), k


def raw_bytes(gc, k):
    from scavislam_amd.ctypes_types import LoopLocationResult
    sz = C.sizeof(LoopLocationResult)
    return [gc.raw_index["results"][k * sz:(k + 1) * sz]] + [gc.raw_index[key][k].tobytes() for key in ("word", "word_d2", "scores")]


# ---- 1. words ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture1024", "fixture1000", "fixture129", "seeded300x128", "seeded9983"])
def test_words_equal_the_exact_search(ctx, name):
    V = vocabulary(name)
    K = V.shape[1]
    rng = np.random.default_rng(78)
    gc = checker(ctx, K=K, max_places=3, max_checks=3)
    gc.set_vocabulary(V)
    descs = [M.descriptors(rng, V, rng.integers(0, len(V), n)) for n in NQ]
    for s, d in enumerate(descs):
        u = rng.uniform(50, 400, len(d))
        gc.set_place(s, d, np.stack([u, u, u - 20.0], 1))
    outs = gc.add_locations([0, 1, 2], do_loop_detection=False)
    for d, o in zip(descs, outs):
        w, D, B = M.words(d, V)
        assert M.bands_empty(D, B) == (True, True), "precondition: a descriptor near a tie or near the radius (change the seed)"
        far = np.arange(len(d)) % 5 == 4
        assert (w[far] == -1).all() and (w[~far] >= 0).all(), "precondition: sigma 0.02 inside the radius, 0.08 outside"
        assert o.word.shape == (len(d),) and np.array_equal(o.word, w)
        best = D.min(axis=1)
        err = np.abs(o.word_d2.astype(np.float64) - best)
        print(name, len(d), "max d2 error / bound:", (err / (B + 2.0 ** -22 * best)).max())
        assert (err <= B + 2.0 ** -22 * best).all()
        assert o.number_of_words == int((w >= 0).sum()) and o.n_scored == 0 and o.best_slot == -1 and not o.candidate
    assert (gc.raw_index["word"][0, NQ[0]:] == -1).all() and (gc.raw_index["word_d2"][0, NQ[0]:] == 0).all()      # the padding behind a place's count
    gc.close()


def test_exact_tie_across_chunks_goes_to_the_lowest_word(ctx):
    """the first and the last of 9 983 words are one row whose arithmetic is exact in any order (four halves): both chunks form the same key"""
    V = vocabulary("seeded9983").copy()
    row = np.zeros(64, np.float32)
    row[[3, 17, 40, 63]] = 0.5
    V[0] = V[-1] = row
    rng = np.random.default_rng(5)
    d = M.descriptors(rng, V, rng.integers(1, len(V) - 1, 67))
    d[0] = row
    gc = checker(ctx, max_places=1, max_checks=1)
    gc.set_vocabulary(V)
    gc.set_place(0, d, np.stack([np.full(67, 300.0), np.full(67, 200.0), np.full(67, 280.0)], 1))
    o = gc.add_locations([0], do_loop_detection=False)[0]
    assert o.word[0] == 0 and o.word_d2[0] == 0.0
    w, D, B = M.words(d[1:], V)
    assert M.bands_empty(D, B) == (True, True) and np.array_equal(o.word[1:], w)
    gc.close()


# ---- 2. scoring ------------------------------------------------------------------------------------------------------------------------------------------------
def test_scores_equal_the_sequential_float_model(ctx):
    gc = checker(ctx)
    load_scenario(gc)
    calls = locs()
    outs = gc.add_locations(calls)
    V = vocabulary("fixture1024")
    for pl, o in zip(scenario(), outs):
        w, D, B = M.words(pl["desc"], V)
        assert M.bands_empty(D, B) == (True, True) and np.array_equal(o.word, w)
    model = model_run(outs, calls)
    # preconditions on the model: place 9 finds place 2 (3.10), nothing else comes near 2; at least one score is order-sensitive
    assert model[9]["best_slot"] == 2 and model[9]["candidate"] and abs(float(model[9]["best_score"]) - 3.0954) < 5e-3
    assert max(float(v) for p, m in enumerate(model) for s, v in m["stats"].items() if (p, s) != (9, 2)) < 1.5
    assert any(np.float32(np.sum(np.asarray(t, np.float64))) != m["stats"][s] for m in model for s, t in m["terms"].items())
    assert any(len(o.word[o.word >= 0]) > len(set(o.word[o.word >= 0].tolist())) for o in outs)      # words repeat inside a place
    assert_equals_model(outs, model)
    assert outs.candidates() == [(9, 2)]
    _cache["scenario_bytes"] = [raw_bytes(gc, k) for k in range(P)]
    gc.close()


def test_excluded_place_is_no_candidate(ctx):
    gc = checker(ctx)
    load_scenario(gc)
    calls = locs()
    calls[9]["exclude"] = M.excludes(9) + [2]
    outs = gc.add_locations(calls)
    model = model_run(outs, calls)
    assert not model[9]["candidate"] and 2 not in model[9]["stats"]
    assert_equals_model(outs, model)
    assert outs[9].scores[2] == 0 and outs.candidates() == []
    gc.close()


def test_location_added_without_detection_is_seen_later(ctx):
    gc = checker(ctx)
    load_scenario(gc)
    calls = locs()
    for p in (2, 5):
        calls[p]["do_loop_detection"] = False
    outs = gc.add_locations(calls)
    model = model_run(outs, calls)
    assert model[9]["best_slot"] == 2 and model[9]["candidate"]                 # place 2 is in the index although it was added without scoring
    assert_equals_model(outs, model)
    for p in (2, 5):
        assert not outs[p].scores.any() and outs[p].n_scored == 0 and outs[p].best_slot == -1 and outs[p].number_of_words > 0
    gc.close()


# ---- 3. batch = singles ----------------------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_singles_byte_for_byte(ctx):
    calls = locs()
    runs = []
    for size in (12, 4, 1):
        gc = checker(ctx)
        load_scenario(gc)
        got = []
        for i in range(0, P, size):
            gc.add_locations(calls[i:i + size])
            got += [raw_bytes(gc, k) for k in range(size)]
        runs.append(got)
        gc.close()
    assert runs[0] == runs[1], "three calls of four differ from one call of twelve"
    assert runs[0] == runs[2], "twelve single calls differ from one call of twelve"
    if "scenario_bytes" in _cache:
        assert runs[0] == _cache["scenario_bytes"]                              # a repetition on another handle


def test_seventy_places_cross_a_wave_boundary(ctx):
    n = 70
    V = vocabulary("fixture1024")
    places = M.make_places(V, seed=10, n_places=n, lo=20, hi=40, revisit=None)
    calls = locs(range(n))
    runs = []
    for size in (n, 1):
        gc = checker(ctx, max_desc=40, max_places=n, max_checks=n)
        load_scenario(gc, places)
        got, outs = [], []
        for i in range(0, n, size):
            outs += gc.add_locations(calls[i:i + size])
            got += [raw_bytes(gc, k) for k in range(size)]
        runs.append(got)
        gc.close()
        if size == n:
            model = model_run(outs, calls, n)
            assert sum(m["n_scored"] for m in model) > n and any(s >= 64 for m in model for s in m["stats"])      # terms on both sides of slot 64
            assert_equals_model(outs, model, n)
    assert runs[0] == runs[1]


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_as_it_was(ctx):
    from scavislam_amd.capi import SvsError

    def status(fn, code):
        with pytest.raises(SvsError) as e:
            fn()
        assert str(e.value).startswith(f"status {code}:"), str(e.value)

    gc = checker(ctx, max_checks=P)
    pl = scenario()
    for p in range(P - 1):                                                       # slot 11 stays empty for now
        gc.set_place(p, pl[p]["desc"], pl[p]["uvu"])
    status(lambda: gc.add_locations([0]), 1)                                     # no vocabulary
    V = vocabulary("fixture1024")
    status(lambda: gc.set_vocabulary(np.zeros((0, 64), np.float32)), 1)          # n_words < 1
    status(lambda: ctx.check(ctx.lib.svs_loop_set_vocabulary(gc.h, (1 << 20) + 1, V.ctypes.data)), 4)      # above SVS_LOOP_MAX_WORDS (refused before h_words is read)
    gc.set_vocabulary(V)
    calls = locs()
    first = gc.add_locations(calls[:1])
    status(lambda: gc.add_locations([calls[1], dict(slot=11)]), 1)               # an empty slot, behind a valid location
    status(lambda: gc.add_locations([calls[1], dict(slot=0)]), 1)                # a slot that is already a location
    status(lambda: gc.add_locations([dict(slot=12)]), 1)                         # a slot outside the store
    status(lambda: gc.add_locations([calls[1], dict(slot=2, exclude=[P])]), 1)   # an exclude slot outside [0, max_places)
    status(lambda: gc.add_locations([calls[1], dict(slot=2, exclude=[-1])]), 1)
    status(lambda: gc.add_locations([calls[1], calls[2], calls[1]]), 1)          # one slot twice in a call
    gc.set_place(11, pl[11]["desc"], pl[11]["uvu"])
    status(lambda: gc.add_locations(calls[1:] + [dict(slot=1)] * 2), 4)          # n > max_checks
    outs = list(first) + list(gc.add_locations(calls[1:]))
    model = model_run(outs, calls)
    assert model[9]["best_slot"] == 2 and model[9]["candidate"]
    assert_equals_model(outs, model)                                             # nothing of the refused calls reached the index
    gc.close()


# ---- 5. the C++ adaptor ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [True, False])
def test_cpp_adaptor_detects_the_loop_only_with_shared_geometry(ctx, tmp_path, geometry):
    exe = tmp_path / "place_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "place_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    V = vocabulary("fixture1024")
    places = scenario() if geometry else M.make_places(V, geometry=False)
    cam = L.CAM
    with open(tmp_path / "place.bin", "wb") as f:
        f.write(np.array([64, len(V), P, 330], np.int32).tobytes())
        f.write(np.array([cam["f"], cam["cx"], cam["cy"], cam["b"]], np.float64).tobytes())
        f.write(V.tobytes())
        for pl in places:
            f.write(np.array([len(pl["desc"])], np.int32).tobytes())
            f.write(pl["desc"].tobytes())
            f.write(pl["uvu"].tobytes())
    lines = [l.split() for l in subprocess.check_output([str(exe), str(tmp_path / "place.bin")]).decode().splitlines() if l.startswith("LOC ")]
    assert len(lines) == P
    # the same places through the Python mirror
    gc = checker(ctx)
    load_scenario(gc, places)
    outs = gc.add_locations(locs())
    for p, (tok, o) in enumerate(zip(lines, outs)):
        assert [int(t) for t in tok[1:6]] == [p, int(p == 9 and geometry), o.number_of_words, o.n_scored, o.best_slot], tok
        assert np.float32(float(tok[6])) == o.best_score and int(tok[7]) == int(o.candidate) == int(p == 9)
    t9 = lines[9]
    print("place 9:", " ".join(t9))
    assert (int(t9[8]), int(t9[9])) == (109, 102)                                # the DetectedLoop names the keyframes either way
    assert int(t9[10]) > 30 if geometry else int(t9[10]) < 10                    # inliers of the geometric check
    gc.close()
