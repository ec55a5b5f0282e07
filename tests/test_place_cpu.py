"""The place index without a GPU: the two restatements of tests/place_model.py against each other, the preconditions the GPU tests lean on, the fixture
against the reference's own dictionary, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import place_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PNG = "/root/reference/data/surfwords10000.png"
NEW_SYMBOLS = ("svs_loop_set_vocabulary", "svs_loop_add_locations", "svs_loop_index_stage_times")
P = 12


@pytest.fixture(scope="module")
def scenario():
    V = M.fixture_words()
    places = M.make_places(V)
    lit, den = M.LiteralIndex(len(V)), M.DenseIndex(len(V), P)
    rows = []
    for p, pl in enumerate(places):
        w, D, B = M.words(pl["desc"], V)
        rows.append(dict(word=w, bands=M.bands_empty(D, B), lit=lit.add_location(p, w, True, M.excludes(p)), den=den.add_location(p, w, True, M.excludes(p))))
    return rows


def test_literal_and_dense_models_agree_bit_for_bit(scenario):
    for p, r in enumerate(scenario):
        a, b = r["lit"], r["den"]
        assert np.array_equal(M.scores_row(a["stats"], P).view(np.uint32), b["scores"].view(np.uint32)), p
        for key in ("number_of_words", "n_scored", "best_slot", "candidate"):
            assert a[key] == b[key], (p, key)
        assert np.float32(a["best_score"]).view(np.uint32) == np.float32(b["best_score"]).view(np.uint32)


def test_scenario_has_the_shape_the_gpu_tests_rely_on(scenario):
    n = sum(len(r["word"]) for r in scenario)
    assigned = sum(int((r["word"] >= 0).sum()) for r in scenario)
    assert 0.75 < assigned / n < 0.85
    for p, r in enumerate(scenario):
        w = r["word"][r["word"] >= 0]
        assert 200 <= len(r["word"]) <= 330 and len(w) - len(set(w.tolist())) >= 5, p      # repeated words inside one place
        assert r["bands"] == (True, True), p                                                # no descriptor near a tie or near the radius
    a = scenario[9]["lit"]
    assert a["best_slot"] == 2 and a["candidate"] and abs(float(a["best_score"]) - 3.0954) < 5e-3
    others = [float(v) for p, r in enumerate(scenario) for o, v in r["lit"]["stats"].items() if (p, o) != (9, 2)]
    assert max(others) < 1.5 and not any(r["lit"]["candidate"] for p, r in enumerate(scenario) if p != 9)


def test_scores_depend_on_the_order_of_the_float_sum(scenario):
    """at least one score differs from the f64 sum of its own terms rounded once: a parallel or pairwise sum on the device would not pass the GPU test"""
    differ = total = 0
    for r in scenario:
        for o, t in r["lit"]["terms"].items():
            total += 1
            differ += int(np.float32(np.sum(np.asarray(t, np.float64))) != r["lit"]["stats"][o])
    print("scores that differ from the f64 sum rounded once:", differ, "of", total)
    assert differ >= 1


def test_repeated_word_meets_a_df_that_counts_its_own_keyframe():
    """the two properties of the reference the header spells out, on a hand-made index"""
    for Index in (lambda: M.LiteralIndex(4), lambda: M.DenseIndex(4, 4)):
        ix = Index()
        ix.add_location(0, [1, 1, 2], True)
        ix.add_location(1, [1, 3], True)
        r = ix.add_location(2, [1, 1], True)
        # first occurrence: n_loc = 2 (place 2 not counted), df = 2; second: df = 3 (place 2 inserted the word in between)
        t0 = [np.float32(np.float32(2) / np.float32(3)) * np.float32(np.float32(2) / np.float32(2)), np.float32(np.float32(2) / np.float32(3)) * np.float32(np.float32(2) / np.float32(3))]
        t1 = [np.float32(np.float32(1) / np.float32(2)) * np.float32(np.float32(2) / np.float32(2)), np.float32(np.float32(1) / np.float32(2)) * np.float32(np.float32(2) / np.float32(3))]
        got = r["stats"] if "stats" in r else {o: v for o, v in enumerate(r["scores"]) if v > 0}
        assert got[0] == np.float32(t0[0] + t0[1]) and got[1] == np.float32(t1[0] + t1[1])
        assert r["best_slot"] == 0 and r["n_scored"] == 2 and r["number_of_words"] == 2


def test_fixture_is_the_head_of_the_reference_dictionary():
    if not os.path.exists(REF_PNG):
        pytest.skip("the reference tree is absent")
    from PIL import Image
    im = np.ascontiguousarray(np.array(Image.open(REF_PNG)))
    assert im.shape == (9983, 256) and im.dtype == np.uint8
    V = M.fixture_words()
    assert V.dtype == np.float32 and V.shape == (1024, 64)
    assert np.array_equal(im[:1024].reshape(1024, 256).view(np.float32).view(np.uint32), V.view(np.uint32))


def test_header_and_binding_declare_the_index_entry_points():
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import LoopLocation, LoopLocationResult
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
    assert "svs_loop_location_result" in header and "} svs_loop_location;" in header
    assert int(re.search(r"#define\s+SVS_API_VERSION\s+(\d+)", header).group(1)) == capi.API_VERSION == 9
    assert int(re.search(r"#define\s+SVS_LOOP_MAX_WORDS\s+(\d+)", header).group(1)) >= 65536
    assert C.sizeof(LoopLocation) == 32 and C.sizeof(LoopLocationResult) == 20      # the C layouts on LP64
