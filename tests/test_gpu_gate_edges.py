"""svs_process_matched_points (StereoFrontend::processMatchedPoints' gate) at its edges, against oracle.process_matched_points: every flag, position and counter
as BITS, the track-length sum to 1e-12 (parallel summation order).

  * list lengths around the 256 lanes of the sweep and their prefetch of record i + 256, all three strides longer than the list, poison in the gaps;
  * observations exactly on the lines of the 2 x 2 and 3 x 3 grids and one double to either side;
  * residuals exactly on the three thresholds (refused: the inequalities are strict) and one double inside (accepted);
  * the device's exact quotients (devutil.h: div_rn_guarded) on the hostile operands of tests/test_quotient_cpu.py -- with an identity pose and a unit camera
    curkey_uv_pyr IS the quotient of two of the caller's doubles."""
import ctypes as C

import numpy as np
import pytest

import quotient_pools as QP
from motion_cases import synthetic_results

pytestmark = pytest.mark.gpu

GUARD = 0xA5
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def _cam(c):
    from scavislam_amd.ctypes_types import Cam
    return Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"])


def _gate(gpu_ctx, res, pts, n_new, camc, T, mre, pads=(5, 9, 3)):
    """res, pts [B][n]; T [B][3][4].  Strides n + pads (results, points, gated); the gaps hold records that would count if they were read; returns
    (gated [B][n], stats [B]) after checking that the gaps of the gated buffer and the guard slot behind the statistics kept their fill"""
    import torch
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, GATED_POINT_DTYPE, MATCH_RESULT_DTYPE, POINT_STATS_DTYPE
    ctx, stream = gpu_ctx
    B, n = res.shape
    rbuf = np.zeros((B, n + pads[0]), MATCH_RESULT_DTYPE)
    rbuf["obs"] = np.nan                                   # an OK record in the gap: read, it would count in num_obs
    rbuf["xyz_actkey"] = (0.0, 0.0, 4.0)
    rbuf[:, :n] = res
    pbuf = np.zeros((B, n + pads[1]), CANDIDATE_DTYPE)
    pbuf["anchor_level"] = 9
    pbuf[:, :n] = pts
    gs, ss = GATED_POINT_DTYPE.itemsize, POINT_STATS_DTYPE.itemsize
    with torch.cuda.stream(stream):
        d_res = torch.as_tensor(rbuf.view(np.uint8).reshape(-1)).cuda()
        d_pts = torch.as_tensor(pbuf.view(np.uint8).reshape(-1)).cuda()
        d_T = torch.as_tensor(np.ascontiguousarray(T, np.float64).reshape(-1)).cuda()
        d_g = torch.full((B * (n + pads[2]) * gs,), GUARD, dtype=torch.uint8, device="cuda")
        d_s = torch.full(((B + 1) * ss,), GUARD, dtype=torch.uint8, device="cuda")
    ctx.call("svs_process_matched_points", d_res.data_ptr(), d_pts.data_ptr(), n, n + pads[0], n + pads[1], int(n_new), C.byref(camc), d_T.data_ptr(), float(mre),
             d_g.data_ptr(), n + pads[2], d_s.data_ptr(), B)
    ctx.sync()
    g = d_g.cpu().numpy().reshape(B, (n + pads[2]) * gs)
    s = d_s.cpu().numpy()
    assert (g[:, n * gs:] == GUARD).all() and (s[B * ss:] == GUARD).all(), "the gate wrote outside its lists"
    return np.ascontiguousarray(g[:, :n * gs]).view(GATED_POINT_DTYPE).reshape(B, n), s[:B * ss].view(POINT_STATS_DTYPE)


def _assert_bits(gated, stats, g_ref, s_ref, what):
    assert gated.tobytes() == g_ref.tobytes(), (what, "first differing record", int(np.flatnonzero(gated.view(np.uint8).reshape(len(gated), -1) != g_ref.view(np.uint8).reshape(len(gated), -1))[0] // 40))
    for k in ("num_points_grid2x2", "num_points_grid3x3", "num_matched_points", "num_track_points", "num_obs"):
        assert np.array_equal(stats[k], s_ref[k]), (what, k, stats[k], s_ref[k])
    np.testing.assert_allclose(stats["sum_track_length"], s_ref["sum_track_length"], rtol=1e-12, err_msg=str(what))


def _pts(rng, shape, level=None):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    pts = np.zeros(shape, CANDIDATE_DTYPE)
    pts["anchor_level"] = rng.integers(0, 3, shape) if level is None else level
    return pts


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513, 1025])
def test_gate_list_lengths_and_strides(gpu_ctx, n):
    import oracle as O
    from scavislam_amd import synth
    rng = np.random.default_rng([31, n])
    cam = synth.CAM_DEFAULT
    camc = _cam(cam)
    B = 3
    T = np.stack([synth.pose(synth.so3_exp(rng.normal(0, 0.01, 3)), rng.normal(0, 0.04, 3)) for _ in range(B)])
    res = np.stack([synthetic_results(rng, cam, T[b], n, outliers=0.25, n_fail=n // 5) for b in range(B)])
    res["obs"] += rng.choice([0.0, 1.9, 2.1, 3.9, 4.1, 5.9, 6.1, 7.9, 8.1], size=res["obs"].shape) * rng.choice([-1, 1], size=res["obs"].shape)
    pts = _pts(rng, (B, n))
    n_acc = 0
    for n_new in sorted({0, 1, n - 1, n, n + 5}):
        gated, stats = _gate(gpu_ctx, res, pts, n_new, camc, T, 2.0)
        for b in range(B):
            g_ref, s_ref = O.process_matched_points(res[b], pts[b], n_new, camc, T[b], 2.0)
            assert g_ref["is_new"].sum() == g_ref["accepted"][:n_new].sum()
            n_acc += int(s_ref["num_track_points"])
            _assert_bits(gated[b], stats[b], g_ref, s_ref, (n, n_new, b))
    assert n_acc > 0 or n <= 2


def _grid_lines(w):
    third = np.float32(1. / 3.)
    return [int(w * 0.5), int(np.float32(w) * third), int(np.float32(2 * w) * third)]


@pytest.mark.parametrize("w,h", [(640, 480), (512, 384), (322, 242), (160, 128)])
def test_gate_grid_lines(gpu_ctx, w, h):
    """observations exactly on half_w, third_w, twothird_w and their h counterparts, and on the doubles next to them; the point is un-projected from the observation,
    so every record passes and only its cell is in question"""
    import oracle as O
    from scavislam_amd import synth
    rng = np.random.default_rng([32, w])
    cam = dict(f=0.9 * w, cx=w / 2.0, cy=h / 2.0, b=0.075, w=w, h=h)
    camc = _cam(cam)
    T = synth.pose(synth.so3_exp(np.array([0.01, -0.02, 0.005])), np.array([0.03, -0.01, 0.08]))
    uv, triples = [], []                      # triples: index of the first of three records (just below the line, on it, just above) that share the other coordinate
    for axis, (size, other) in enumerate(((w, h), (h, w))):
        for L in _grid_lines(size):
            for _ in range(6):
                o = rng.uniform(1, other - 1)
                triples.append(len(uv))
                for val in (np.nextafter(float(L), -np.inf), float(L), np.nextafter(float(L), np.inf)):
                    uv.append((val, o) if axis == 0 else (o, val))
    uv = np.array(uv + [(rng.uniform(0, w), rng.uniform(0, h)) for _ in range(150)])
    n = len(uv)
    z = rng.uniform(3, 12, n)
    p_cur = np.stack([(uv[:, 0] - cam["cx"]) / cam["f"] * z, (uv[:, 1] - cam["cy"]) / cam["f"] * z, z], 1)
    Ti = synth.pose_inv(T)
    from scavislam_amd.ctypes_types import MATCH_RESULT_DTYPE
    res = np.zeros(n, MATCH_RESULT_DTYPE)
    res["xyz_actkey"] = p_cur @ Ti[:, :3].T + Ti[:, 3]
    res["obs"] = np.stack([uv[:, 0], uv[:, 1], uv[:, 0] - cam["f"] * cam["b"] / z], 1)
    pts = _pts(rng, n)
    g_ref, s_ref = O.process_matched_points(res, pts, n // 2, camc, T, 2.0)
    # preconditions: everything passes, every cell is populated, and the oracle puts the record below a line and the one on it into different cells
    assert s_ref["num_track_points"] == n and (s_ref["num_points_grid2x2"] > 0).all() and (s_ref["num_points_grid3x3"] > 0).all()
    for t in triples:
        cells = [O.process_matched_points(res[k:k + 1], pts[k:k + 1], 0, camc, T, 2.0)[1] for k in (t, t + 1, t + 2)]
        cells = [np.concatenate([c["num_points_grid2x2"], c["num_points_grid3x3"]]).tolist() for c in cells]
        assert cells[0] != cells[1] and cells[1] == cells[2], (t, uv[t:t + 3])
    gated, stats = _gate(gpu_ctx, np.stack([res, res[::-1]]), np.stack([pts, pts[::-1]]), n // 2, camc, np.stack([T, T]), 2.0)
    _assert_bits(gated[0], stats[0], g_ref, s_ref, (w, h))
    g_rev, s_rev = O.process_matched_points(res[::-1], pts[::-1], n // 2, camc, T, 2.0)
    _assert_bits(gated[1], stats[1], g_rev, s_rev, (w, h, "reversed"))


@pytest.mark.parametrize("mre", [2.0, 0.75, 5.0])
def test_gate_thresholds_on_the_line(gpu_ctx, mre):
    """A camera of exactly representable numbers (f 256, cx 320, cy 240, b 0.25), T = identity, z a power of two and x, y multiples of 1/256: the prediction is exact, and
    the point is placed so that the component under test predicts 0 -- the residual is then the observation itself, bit for bit.  Residuals of +-mre 2^level (u, v) and
    +-3 mre (u_right) are refused, one double toward zero from each is accepted; the other two components have a zero residual."""
    import oracle as O
    from scavislam_amd.ctypes_types import MATCH_RESULT_DTYPE
    cam = dict(f=256.0, cx=320.0, cy=240.0, b=0.25, w=640, h=480)
    camc = _cam(cam)
    rng = np.random.default_rng(33)
    rec, levels, want = [], [], []
    for comp in range(3):
        for level in range(3):
            for z in (1.0, 2.0, 4.0):
                for sign in (1.0, -1.0):
                    bound = 3.0 * mre if comp == 2 else mre * (1 << level)
                    for inside in (False, True):
                        x, y = rng.integers(-256, 257, 2) / 256.0 * z
                        if comp == 0:
                            x = -1.25 * z
                        elif comp == 1:
                            y = -0.9375 * z
                        else:
                            x = 0.25 - 1.25 * z
                        pred = np.array([x / z * 256.0 + 320.0, y / z * 256.0 + 240.0, (x - 0.25) / z * 256.0 + 320.0])
                        assert pred[comp] == 0.0
                        obs = pred.copy()
                        obs[comp] = np.nextafter(sign * bound, 0.0) if inside else sign * bound
                        rec.append((obs, (x, y, z)))
                        levels.append(level)
                        want.append(1 if inside else 0)
    n = len(rec)
    res = np.zeros(n, MATCH_RESULT_DTYPE)
    res["obs"] = [r[0] for r in rec]
    res["xyz_actkey"] = [r[1] for r in rec]
    pts = _pts(rng, n, level=np.array(levels))
    g_ref, s_ref = O.process_matched_points(res, pts, n // 3, camc, I34, mre)
    assert g_ref["accepted"].tolist() == want                       # precondition: on the line refused, its neighbour accepted, for every combination
    gated, stats = _gate(gpu_ctx, res[None], pts[None], n // 3, camc, I34[None], mre)
    _assert_bits(gated[0], stats[0], g_ref, s_ref, mre)


def quotient_records(b, seed=34):
    """(records, n0, n1, d, index ranges): T = identity and a unit camera make curkey_uv_pyr = (n0 / d, n1 / d); obs is NumPy's own quotient, so that a right quotient
    gives a zero residual and the record is accepted wherever the three quotients are finite"""
    from scavislam_amd.ctypes_types import MATCH_RESULT_DTYPE
    rng = np.random.default_rng(seed)
    ones = QP.all_ones([0, 3, QP.WINDOW_LO, QP.WINDOW_HI])
    tame = QP._with_exponents(QP._hostile_mantissas(), [0, 1, -1])          # hostile mantissas, exponents that keep every quotient finite
    near = QP._with_exponents(QP._hostile_mantissas(), [0, 1, -1, QP.WINDOW_LO, QP.WINDOW_LO + 1, QP.WINDOW_HI - 1, QP.WINDOW_HI])
    pool = np.concatenate([QP.window_edge_values(), QP.SPECIAL, QP.subnormals(rng, 100)])
    finite_pool = pool[np.isfinite(pool)]
    # Against an all-ones denominator the short path (the reciprocal one double below RN(1 / b)) is wrong for the numerators that are powers of two and for no other
    # (a / b is then 1 / b shifted: the same near-midpoint; exact rational evaluation of q + e r over all of `tame` and 20 000 random mantissas): each such
    # denominator meets +-1, +-2, +-1/2 in either numerator, and 26 more of `tame`
    pow2 = np.array([1.0, 2.0, 0.5, -1.0, -2.0, -0.5])
    first = lambda: np.concatenate([np.concatenate([pow2, rng.choice(tame, 26)]) for _ in ones])
    d = np.concatenate([np.repeat(ones, 32), rng.choice(near, 1200), rng.choice(finite_pool, 2640)])
    n0 = np.concatenate([first(), rng.choice(near, 1200), rng.choice(pool, 2640)])
    n1 = np.concatenate([first()[::-1], rng.choice(near, 1200), rng.choice(pool, 2640)])
    res = np.zeros(len(d), MATCH_RESULT_DTYPE)
    res["xyz_actkey"] = np.stack([n0, n1, d], 1)
    with np.errstate(all="ignore"):
        res["obs"] = np.stack([n0 / d, n1 / d, (n0 - b) / d], 1)
    return res, n0, n1, d, ones


@pytest.mark.parametrize("b", [0.0, 0.25])
def test_gate_quotients_are_the_division(gpu_ctx, b):
    import oracle as O
    res, n0, n1, d, ones = quotient_records(b)
    n = len(res)
    camc = _cam(dict(f=1.0, cx=0.0, cy=0.0, b=b, w=640, h=480))
    rng = np.random.default_rng(35)
    pts = _pts(rng, n, level=0)
    g_ref, s_ref = O.process_matched_points(res, pts, n // 2, camc, I34, 2.0)
    acc = g_ref["accepted"] == 1
    with np.errstate(all="ignore"):
        q = np.stack([n0 / d, n1 / d], 1)
        finite = np.isfinite(res["obs"]).all(axis=1)
    # preconditions, on the oracle: the accepted records carry NumPy's quotients, and enough of every kind are there
    assert g_ref["curkey_uv_pyr"][acc].tobytes() == (q[acc] + 0.0).tobytes()                     # (q * 1 + 0: a quotient of -0 arrives as +0)
    assert acc.sum() >= 1000 and np.array_equal(acc, finite)
    assert acc[:32 * len(ones)].all() and np.array_equal(d[:32 * len(ones)], np.repeat(ones, 32)), "every all-ones denominator among the accepted"
    pow2 = lambda x: np.frexp(x)[0] == np.copysign(0.5, x)
    assert all((acc & (d == v) & pow2(n0)).sum() >= 6 and (acc & (d == v) & pow2(n1)).sum() >= 6 for v in ones), "... with the numerators the short path gets wrong"
    outside = ~(QP.in_window(n0) & QP.in_window(n1) & QP.in_window(d))
    assert (acc & outside).sum() >= 100 and (~acc).sum() >= 100, ((acc & outside).sum(), (~acc).sum())
    half = n // 2
    gated, stats = _gate(gpu_ctx, np.stack([res[:half], res[half:]]), np.stack([pts[:half], pts[half:]]), half // 2, camc, np.stack([I34, I34]), 2.0)
    for k, sl in enumerate((slice(0, half), slice(half, n))):
        g_k, s_k = O.process_matched_points(res[sl], pts[sl], half // 2, camc, I34, 2.0)
        _assert_bits(gated[k], stats[k], g_k, s_k, (b, k))
