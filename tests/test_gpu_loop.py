"""The loop-closure geometric check on the device (svs_loop_*: descriptor matching + SE3 RANSAC, PlaceRecognizer::geometricCheck) against the NumPy
restatement tests/loop_model.py.  The stages are judged separately: the model's RANSAC runs on the device's own trainIdx.

Bounds.  Matches: B_i = (K + 4) 2^-23 (|q_i|^2 + max_j |t_j|^2) bounds the error of a K-term f32 chain in either formulation (one rounding per product and
sum; the expansion form's terms are bounded by (|q| + |t|)^2).  RANSAC: EPS = 1e-6 px -- two legitimate f64 fits (SVD, Horn) differ by at most 5e-11 px in the
projections of matches within 50 px on these scenes (measured on the CPU, tests/test_loop_cpu.py asserts 1e-6); the margin covers a Jacobi variant and another
order of operations in T x.  Every scene asserts as a PRECONDITION, on the model, that no residual lies within EPS of the threshold and that every match gap
exceeds 2 B: the bands are empty, so counts, flags and indices must be EQUAL and no case is left out."""
import os
import subprocess

import numpy as np
import pytest

import loop_model as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6
THR = 2.5
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
SCENES = [(s, 200, 240, 64) for s in range(1, 7)] + [(11, 67, 131, 64), (12, 67, 131, 64), (13, 300, 150, 64), (14, 40, 300, 128)]
_cache = {}


def scene(seed, N, M, K, frac=0.6):
    key = (seed, N, M, K, frac)
    if key not in _cache:
        sc = L.make_scene(seed, N, M, K, inlier_frac=frac)
        sc["D"] = L.sqdist(sc["q_desc"], sc["t_desc"])
        sc["B"] = L.match_bound(sc["q_desc"], sc["t_desc"])
        for a in sc.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = sc
    return _cache[key]


@pytest.fixture(scope="module")
def ctx():
    from scavislam_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def checker(ctx, K=64, max_desc=320, max_places=4, max_hyp=256, max_checks=8):
    from scavislam_amd.loop import GeometricChecker
    return GeometricChecker(ctx, L.CAM, desc_dim=K, max_desc=max_desc, max_places=max_places, max_hyp=max_hyp, max_checks=max_checks)


def load(gc, sc, q_slot=1, t_slot=0):
    gc.set_place(t_slot, sc["t_desc"], sc["t_uvu"])
    gc.set_place(q_slot, sc["q_desc"], sc["q_uvu"])


def assert_matches(out, sc):
    D, B = sc["D"], sc["B"]
    n = len(D)
    srt = np.sort(D, axis=1)
    if D.shape[1] > 1:
        assert ((srt[:, 1] - srt[:, 0]) > 2 * B).all(), "precondition: a match gap inside 2 B (change the seed)"
    assert out.n_matches == n and out.train_idx.shape == (n,)
    assert (out.train_idx >= 0).all() and (out.train_idx < D.shape[1]).all()
    got = D[np.arange(n), out.train_idx]
    assert (got <= srt[:, 0] + 2 * B).all()
    d2 = out.distance.astype(np.float64) ** 2
    assert (np.abs(d2 - got) <= B + 2.0 ** -22 * got).all(), np.abs(d2 - got).max()      # + the square root's own rounding, squared
    assert np.array_equal(out.train_idx, np.argmin(D, axis=1))


def assert_ransac(out, sc, samples, thr=THR, positive=None):
    cam = sc["cam"]
    m = L.ransac(cam, sc["q_uvu"], sc["t_xyz"], out.train_idx, samples, thr)
    if m["valid"].any():
        assert np.nanmin(np.abs(m["res"] - thr)) > EPS, "precondition: a residual within EPS of the threshold (change the seed)"
    assert np.nanmin(np.abs(m["res_final"] - thr)) > EPS
    if positive is True:
        assert m["n_inliers"] > 30
    if positive is False:
        assert m["n_inliers"] < 10
    print("model: inliers", m["n_inliers"], "best", m["best"], "invalid", m["n_invalid"], "| device:", out.n_inliers, out.best_hyp, out.n_invalid_hyp)
    assert np.array_equal(out.hyp_inliers, m["hyp_inliers"])
    assert out.n_invalid_hyp == m["n_invalid"]
    assert np.array_equal(out.samples, np.where(m["valid"][:, None], np.asarray(samples), -1))
    assert out.best_hyp == m["best"]                     # counts are exact, so first-maximum picks the same index even where the maximum is shared
    assert out.n_inliers == m["n_inliers"] and np.array_equal(out.inlier, m["inlier"])
    T = out.T_query_from_train
    assert np.abs(T[:, :3].T @ T[:, :3] - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-12
    x = sc["t_xyz"][out.train_idx]
    near = m["res_final"].max(1) < 50.0
    if near.any():
        pd, pm = L.map_uvu(cam, x @ T[:, :3].T + T[:, 3]), L.map_uvu(cam, x @ m["T"][:, :3].T + m["T"][:, 3])
        assert np.abs(pd - pm)[near].max() < EPS, np.abs(pd - pm)[near].max()
    if m["best"] < 0:
        assert np.array_equal(T, I34)
    return m


def explicit_triples(rng, H, n, train_idx):
    """random valid triples on the device's train indices, with three rule breakers planted"""
    smp = np.empty((H, 3), np.int32)
    for h in range(H):
        while True:
            r = rng.choice(n, 3, replace=False)
            if len(set(train_idx[r].tolist())) == 3:
                break
        smp[h] = r
    if H >= 8:
        smp[3] = (smp[3][0], smp[3][0], smp[3][2])            # a repeated match
        smp[5] = (smp[5][0], n, smp[5][2])                     # outside the matches
        same = [i for i in range(n) if i != smp[6][0] and train_idx[i] == train_idx[smp[6][0]]]
        if same:
            smp[6][1] = same[0]                                # two matches of one train descriptor
    return smp


@pytest.mark.parametrize("seed,N,M,K", SCENES)
def test_scene_against_model(ctx, seed, N, M, K):
    sc = scene(seed, N, M, K)
    gc = checker(ctx, K)
    load(gc, sc)
    seeded = gc.check(1, 0, n_hyp=100, seed=seed)
    assert_matches(seeded, sc)
    positive = True if N >= 67 else None                       # 40 queries hold 24 planted correspondences: that scene cannot pass 30
    assert_ransac(seeded, sc, L.draw_triples(seed, 100, N, seeded.train_idx), positive=positive)
    smp = explicit_triples(np.random.default_rng(100 + seed), 100, N, seeded.train_idx)
    ex = gc.check(1, 0, samples=smp)
    assert np.array_equal(ex.train_idx, seeded.train_idx) and np.array_equal(ex.distance.view(np.uint32), seeded.distance.view(np.uint32))
    m = assert_ransac(ex, sc, smp, positive=positive)
    assert m["n_invalid"] >= 2
    gc.close()


@pytest.mark.parametrize("H", [1, 256])
def test_hypothesis_counts(ctx, H):
    sc = scene(2, 200, 240, 64)
    gc = checker(ctx)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=H, seed=77)
    assert_ransac(out, sc, L.draw_triples(77, H, 200, out.train_idx))
    smp = explicit_triples(np.random.default_rng(H), H, 200, out.train_idx)
    assert_ransac(gc.check(1, 0, samples=smp), sc, smp)
    gc.close()


def test_no_true_correspondences(ctx):
    sc = scene(31, 200, 240, 64, frac=0.0)
    gc = checker(ctx)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=100, seed=31)
    assert_matches(out, sc)
    assert_ransac(out, sc, L.draw_triples(31, 100, 200, out.train_idx), positive=False)
    assert out.n_inliers < 10
    gc.close()


def test_full_handle_no_full_tile(ctx):
    """N = M = max_desc = 96: no tile is full, and the last row of a place's store is used"""
    sc = scene(21, 96, 96, 64)
    gc = checker(ctx, max_desc=96, max_places=2)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=100, seed=21)
    assert_matches(out, sc)
    assert (out.train_idx == 95).any() or (np.argmin(sc["D"], 1) != 95).all()
    assert_ransac(out, sc, L.draw_triples(21, 100, 96, out.train_idx))
    gc.close()


def test_exact_tie_takes_the_lower_index(ctx):
    sc = scene(1, 200, 240, 64)
    t = sc["t_desc"].copy()
    t[171] = t[38]                                           # in another tile of 32, and in another wave's rows
    t[239] = t[5]
    q = sc["q_desc"].copy()
    q[0], q[199] = t[171], t[239]
    gc = checker(ctx)
    gc.set_place(0, t, sc["t_uvu"])
    gc.set_place(1, q, sc["q_uvu"])
    out = gc.check(1, 0, n_hyp=1, seed=0)
    assert out.train_idx[0] == 38 and out.train_idx[199] == 5
    assert out.distance[0] <= np.sqrt(L.match_bound(q, t)[0]) and out.distance[199] <= np.sqrt(L.match_bound(q, t)[199])
    gc.close()


def test_small_places(ctx):
    gc = checker(ctx)
    # (3, 3, 64): three matches, one possible set of indices
    sc = scene(41, 3, 3, 64, frac=1.0)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=100, seed=3)
    assert_matches(out, sc)
    assert_ransac(out, sc, L.draw_triples(3, 100, 3, out.train_idx))
    # (2, 5, 64): nothing
    sc = scene(42, 2, 5, 64)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=100, seed=3)
    assert_matches(out, sc)
    assert (out.n_matches, out.n_inliers, out.best_hyp, out.n_invalid_hyp) == (2, 0, -1, 100)
    assert np.array_equal(out.T_query_from_train, I34) and not out.inlier.any() and (out.samples == -1).all() and not out.hyp_inliers.any()
    # M = 1: three queries share the one train index -- 100 invalid hypotheses (the reference would never return), the identity
    sc = scene(43, 3, 1, 64)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=100, seed=3)
    assert np.array_equal(out.train_idx, [0, 0, 0])
    assert (out.n_matches, out.best_hyp, out.n_invalid_hyp) == (3, -1, 100) and (out.samples == -1).all()
    assert np.array_equal(out.T_query_from_train, I34)
    assert_ransac(out, sc, L.draw_triples(3, 100, 3, out.train_idx))
    gc.close()


def test_final_pass_with_the_identity(ctx):
    """no hypothesis has an inlier: T stays the identity and the final pass is still made with it (ransac.cpp:126-135) -- match 0 is an inlier under the
    identity only"""
    cam = L.CAM
    rng = np.random.default_rng(5)
    desc = (rng.normal(size=(4, 64)) / 8).astype(np.float32)
    t_xyz = np.array([[0.3, -0.2, 2.0], [-0.5, 0.4, 3.0], [0.8, 0.6, 4.0], [-0.9, -0.7, 5.0]])
    q_xyz = np.array([[0.3, -0.2, 2.0], [1.5, 1.2, 2.5], [-2.4, 0.9, 5.5], [1.0, -2.1, 3.5]])      # no rigid motion takes three train points near these
    t_uvu, q_uvu = L.map_uvu(cam, t_xyz), L.map_uvu(cam, q_xyz)
    sc = dict(cam=cam, q_uvu=q_uvu, t_xyz=L.unmap_uvu(cam, t_uvu))
    smp = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3], [3, 1, 0]], np.int32)
    m = L.ransac(cam, q_uvu, sc["t_xyz"], np.arange(4), smp)
    assert m["best"] == -1 and not m["hyp_inliers"].any() and m["inlier"].tolist() == [True, False, False, False]      # on the model first
    gc = checker(ctx)
    gc.set_place(0, desc, t_uvu)
    gc.set_place(1, desc, q_uvu)
    out = gc.check(1, 0, samples=smp)
    assert np.array_equal(out.train_idx, np.arange(4))
    assert_ransac(out, sc, smp)
    assert out.best_hyp == -1 and out.n_inliers == 1 and out.inlier.tolist() == [True, False, False, False] and np.array_equal(out.T_query_from_train, I34)
    # a place with its own xyz_vec instead of unmap_uvu(uvu): the hand-over of a caller that has it
    gc.set_place(0, desc, t_uvu, xyz=t_xyz + np.array([0.0, 0.0, 0.5]))
    out = gc.check(1, 0, samples=smp)
    assert_ransac(out, dict(cam=cam, q_uvu=q_uvu, t_xyz=t_xyz + np.array([0.0, 0.0, 0.5])), smp)
    gc.close()


def test_errors_come_before_any_launch_and_leave_the_handle_usable(ctx):
    from scavislam_amd.capi import SvsError
    sc = scene(11, 67, 131, 64)
    gc = checker(ctx, max_desc=131, max_places=3, max_hyp=100, max_checks=2)
    load(gc, sc)

    def status(fn, code):
        with pytest.raises(SvsError, match=f"status {code}"):
            fn()
    status(lambda: gc.check(3, 0), 1)                                        # bad slots
    status(lambda: gc.check(1, -1), 1)
    status(lambda: gc.check(2, 0), 1)                                        # an empty slot
    status(lambda: gc.check(1, 0, n_hyp=101), 4)                             # n_hyp > max_hyp
    status(lambda: gc.check(1, 0, n_hyp=0), 1)
    status(lambda: gc.check_batch([(1, 0)] * 3), 4)                          # n_checks > max_checks
    big = scene(1, 200, 240, 64)
    status(lambda: gc.set_place(2, big["q_desc"], big["q_uvu"]), 4)          # n > max_desc
    status(lambda: gc.set_place(3, sc["q_desc"], sc["q_uvu"]), 1)
    bad = sc["q_uvu"].copy()
    bad[5, 2] = bad[5, 0]                                                    # disparity 0 and no xyz
    status(lambda: gc.set_place(2, sc["q_desc"], bad), 1)
    status(lambda: gc.check(2, 0), 1)                                        # ... and the slot stayed empty
    gc.set_place(2, sc["q_desc"], bad, xyz=L.unmap_uvu(sc["cam"], sc["q_uvu"]))      # allowed with xyz given
    out = gc.check(1, 0, n_hyp=100, seed=11)                                 # the next valid call succeeds
    assert_matches(out, sc)
    assert_ransac(out, sc, L.draw_triples(11, 100, 67, out.train_idx))
    gc.close()


RAW = ("train_idx", "distance", "inlier", "samples", "hyp_inliers")


def _bytes_of(gc, c):
    from scavislam_amd.ctypes_types import LoopResult
    import ctypes as C
    sz = C.sizeof(LoopResult)
    return [gc.raw["results"][c * sz:(c + 1) * sz]] + [gc.raw[k][c].tobytes() for k in RAW]


def test_batch_equals_singles_byte_for_byte(ctx):
    a, b = scene(11, 67, 131, 64), scene(13, 300, 150, 64)
    gc = checker(ctx, max_checks=5)
    gc.set_place(0, a["t_desc"], a["t_uvu"])
    gc.set_place(1, a["q_desc"], a["q_uvu"])
    gc.set_place(2, b["t_desc"], b["t_uvu"])
    gc.set_place(3, b["q_desc"], b["q_uvu"])
    smp = explicit_triples(np.random.default_rng(9), 40, 67, np.argmin(a["D"], 1))
    five = [dict(query=1, train=0, n_hyp=100, seed=11), dict(query=3, train=2, n_hyp=256, seed=2), dict(query=1, train=2, n_hyp=17, seed=3),
            dict(query=1, train=0, samples=smp), dict(query=2, train=3, n_hyp=100, seed=5, pixel_thr=4.0)]
    outs = gc.check_batch(five)
    batch = [_bytes_of(gc, c) for c in range(5)]
    # the batch is no degenerate one: its two positive checks are the model's, which is asked for more than 30 inliers first (100 draws do not reach 30 on
    # every seed at 67 queries -- the model has 24 at seed 1 -- so the seeds are ones at which the MODEL does)
    assert_ransac(outs[0], a, L.draw_triples(11, 100, 67, outs[0].train_idx), positive=True)
    assert_ransac(outs[1], b, L.draw_triples(2, 256, 300, outs[1].train_idx), positive=True)
    gc.check_batch(five)
    assert [_bytes_of(gc, c) for c in range(5)] == batch                     # a repetition
    for c in range(5):
        gc.check_batch([five[c]])
        assert _bytes_of(gc, 0) == batch[c], f"check {c} alone differs from the batch"
    other = [dict(query=3, train=0, n_hyp=50, seed=8), dict(query=0, train=1, n_hyp=3, seed=9), five[2], dict(query=2, train=2, n_hyp=9, seed=1),
             dict(query=3, train=3, n_hyp=100, seed=4)]
    gc.check_batch(other)
    assert _bytes_of(gc, 2) == batch[2], "a check's bytes changed with its neighbours"
    gc.close()


def test_cpp_adaptor_reports_what_python_reports(ctx, tmp_path):
    exe = tmp_path / "loop_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "loop_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    sc = scene(12, 67, 131, 64)
    cam = sc["cam"]
    seed = 1234
    with open(tmp_path / "loop.bin", "wb") as f:
        f.write(np.array([64, 67, 131], np.int32).tobytes())
        f.write(np.array([cam["f"], cam["cx"], cam["cy"], cam["b"]], np.float64).tobytes())
        f.write(np.array([seed], np.uint64).tobytes())
        for k in ("q_desc", "q_uvu", "t_desc", "t_uvu"):
            f.write(sc[k].tobytes())
    lines = subprocess.check_output([str(exe), str(tmp_path / "loop.bin")]).decode().splitlines()
    tok = [l for l in lines if l.startswith("LOOP ")][0].split()
    T = np.array([float(v) for v in [l for l in lines if l.startswith("T ")][0].split()[1:]]).reshape(3, 4)
    gc = checker(ctx, max_hyp=100)
    load(gc, sc)
    out = gc.check(1, 0, n_hyp=100, seed=seed)
    assert [int(v) for v in tok[1:]] == [int(out.n_inliers > 30), 42, 17, out.n_matches, out.n_inliers, out.best_hyp, out.n_invalid_hyp]
    assert out.n_inliers > 30 and np.array_equal(T, out.T_query_from_train)
    gc.close()
