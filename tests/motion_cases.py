"""Cases, yardstick and bars shared by the edge tests of the motion-only refinement (tests/test_motion_edges_cpu.py: the oracle alone, under permutations of its
list and against the NumPy model; tests/test_gpu_motion_edges.py: the three device routes of svs_motion_only against the oracle).

The yardstick: two exact-arithmetic equals of the LM loop -- the same list in another order, or the same sums added in a kernel's order --
agree in chi2 to rounding, but their accept test rho = chi2 - new_chi2 > 0 can go either way on a trial with rho ~ 0, and the final poses then differ by about that
trial's step.  oracle.motion_only_trace reports every trial; the EXPOSURE e of a case is the largest step among its trials with |rho| <= 1e-11 chi2 (about 100 x the
relative noise of an f64 sum of up to 12 288 terms), 0 if there is none.  The pose bar of a case is 1e-9 + 2 e; chi2 is held to 1e-9 relative everywhere.

Every case is a list of matcher records, a start pose and the members of a PoseOptParams.  Cases come in GROUPS of equal list length and parameters: one group is one
batched device call.  The numbers are the smallest at which the fused kernel changes path: a wave (64), a workgroup (256), its register file (6 x 256 = 1536), a
compaction round (8 x 256 = 2048), the last list whose index list fits LDS (12 288)."""
import functools
from typing import NamedTuple

import numpy as np

REFERENCE_PRM = (1, 15, 2.0, -1.0, 1e-5)      # PoseOptParams.reference(): robust, 15 iterations, kernel 2, mu from tau = 1e-5
PLAIN_PRM = (0, 15, 2.0, -1.0, 1e-5)
COUNTS = (1, 2, 3, 6, 7, 20, 63, 64, 65, 255, 256, 257, 1535, 1536, 1537, 2049)
HOSTILE_FROM = 63                             # from this count up: two points behind the camera, two at 1000 x their distance
PLAIN_COUNTS = (3, 64, 257, 1537)             # without the hostile points: with no Huber weight they dominate and e reaches 1e-6
LAYOUT_LENGTHS = (2047, 2048, 2049, 4097)
LAYOUTS = ("last_only", "first_only", "round_rejected", "alternating", "wave_rejected", "random_statuses")
STARTS = ("far", "near", "true")
LOOP_COUNT = 300
SEED = 5


class Case(NamedTuple):
    name: str
    res: np.ndarray       # MATCH_RESULT_DTYPE [n]
    T0: np.ndarray        # 3 x 4
    prm: tuple            # PoseOptParams members (min_obs left at 0)
    tags: dict


class Group(NamedTuple):
    name: str
    cases: tuple


def cam():
    from scavislam_amd import synth
    return synth.CAM_DEFAULT


def cam_struct(c=None):
    from scavislam_amd.ctypes_types import Cam
    c = c or cam()
    return Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"])


def params(prm, min_obs=0):
    from scavislam_amd.ctypes_types import PoseOptParams
    return PoseOptParams(*prm, min_obs)


def synthetic_results(rng, cam, T_true, n, outliers=0.1, n_fail=30):
    """matcher-like result records: points in the active keyframe frame, stereo observations in the current frame."""
    from scavislam_amd.ctypes_types import MATCH_RESULT_DTYPE
    res = np.zeros(n, MATCH_RESULT_DTYPE)
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 15, n)], 1)
    p = xyz @ T_true[:, :3].T + T_true[:, 3]
    u = p[:, 0] / p[:, 2] * cam["f"] + cam["cx"]
    v = p[:, 1] / p[:, 2] * cam["f"] + cam["cy"]
    ur = (p[:, 0] - cam["b"]) / p[:, 2] * cam["f"] + cam["cx"]
    obs = np.stack([u, v, ur], 1) + rng.normal(0, 0.4, (n, 3))
    bad = rng.random(n) < outliers
    obs[bad] += rng.uniform(-25, 25, (bad.sum(), 3))
    res["obs"], res["xyz_actkey"] = obs, xyz
    res["status"][rng.choice(n, n_fail, replace=False)] = rng.integers(1, 7, n_fail)      # matcher rejections are skipped
    return res


def _project(cam, T, xyz):
    p = xyz @ T[:, :3].T + T[:, 3]
    return np.stack([p[:, 0] / p[:, 2] * cam["f"] + cam["cx"], p[:, 1] / p[:, 2] * cam["f"] + cam["cy"], (p[:, 0] - cam["b"]) / p[:, 2] * cam["f"] + cam["cx"]], 1)


def _add_hostile_points(rng, cam, T_true, res):
    """records 5 and 17: the point behind the camera (z of -2 ... -10), its observation left as it was -- a gross outlier whose Jacobian has the other sign;
    records 11 and 40: the point at 1000 x its distance, observed where it projects: an inlier with next to no pull on the translation"""
    xyz = res["xyz_actkey"]
    xyz[[5, 17], 2] = -rng.uniform(2, 10, 2)
    xyz[[11, 40]] *= 1000.0
    res["obs"][[11, 40]] = _project(cam, T_true, xyz[[11, 40]]) + rng.normal(0, 0.4, (2, 3))


def _truth(rng):
    from scavislam_amd import synth
    return synth.pose(synth.so3_exp(rng.normal(0, 0.01, 3)), rng.normal(0, 0.04, 3))


def _start(rng, T_true, start):
    """identity = far; a few mrad / mm off; the true pose itself"""
    from scavislam_amd import synth
    if start == "far":
        return synth.pose(np.eye(3), np.zeros(3))
    if start == "near":
        return synth.pose_mul(synth.pose(synth.so3_exp(rng.normal(0, 0.002, 3)), rng.normal(0, 0.005, 3)), T_true)
    return T_true.copy()


def _count_case(kind, n, si, prm, hostile, seed):
    rng = np.random.default_rng([SEED, seed, n, si, prm[0]])
    T_true = _truth(rng)
    res = synthetic_results(rng, cam(), T_true, n, outliers=0.1 if prm[0] else 0.0, n_fail=0)
    if hostile:
        _add_hostile_points(rng, cam(), T_true, res)
    return Case(f"{kind}-{n}-{STARTS[si]}", res, _start(rng, T_true, STARTS[si]), prm, dict(kind=kind, count=n, start=STARTS[si]))


def apply_layout(rng, res, layout):
    """rejected records (status != 0) laid out against the compaction's rounds of 8 x 256 status words and its per-wave ballots"""
    n = len(res)
    st = res["status"]
    st[:] = 0
    if layout == "last_only":
        st[:n - 1] = 3
    elif layout == "first_only":
        st[1:] = 4
    elif layout == "round_rejected":      # the whole first round rejected and 70 OK behind it -- where the list has no 70 records behind 2048: its last 70 (2049: its last one)
        first_ok = 2048 if n >= 2048 + 70 else (2048 if n > 2048 else n - 70)
        st[:] = 2
        st[first_ok:first_ok + 70] = 0
    elif layout == "alternating":
        st[1::2] = 1
    elif layout == "wave_rejected":       # one whole wave of 64 consecutive records, aligned to the waves of the second chunk
        st[256 + 64:256 + 128] = 5
    elif layout == "random_statuses":
        k = rng.choice(n, n // 3, replace=False)
        st[k] = rng.integers(1, 7, len(k))
    else:
        raise KeyError(layout)
    return res


def _layout_case(n, layout, seed):
    rng = np.random.default_rng([SEED, seed, n, LAYOUTS.index(layout)])
    T_true = _truth(rng)
    res = apply_layout(rng, synthetic_results(rng, cam(), T_true, n, n_fail=0), layout)
    return Case(f"layout-{n}-{layout}", res, _start(rng, T_true, "near"), REFERENCE_PRM, dict(kind="layout", layout=layout, length=n, count=int((res["status"] == 0).sum())))


def _long_case(n, n_ok, seed):
    rng = np.random.default_rng([SEED, seed, n])
    T_true = _truth(rng)
    res = synthetic_results(rng, cam(), T_true, n, n_fail=0)
    if n_ok < n:
        res["status"] = 6
        res["status"][np.sort(rng.choice(n, n_ok, replace=False))] = 0
    return Case(f"long-{n}", res, _start(rng, T_true, "near"), REFERENCE_PRM, dict(kind="long", length=n, count=n_ok))


# (the trailing seed of a case: changed until the conditions of tests/test_motion_edges_cpu.py::test_conditions hold)
@functools.lru_cache(maxsize=None)
def groups():
    out = []
    for n in COUNTS:
        out.append(Group(f"count-{n}", tuple(_count_case("count", n, si, REFERENCE_PRM, n >= HOSTILE_FROM, 0) for si in range(3))))
    for n in PLAIN_COUNTS:
        out.append(Group(f"plain-{n}", tuple(_count_case("plain", n, si, PLAIN_PRM, False, 1 if n == 3 else 0) for si in range(3))))      # (3, seed 0: all three e > 1e-9)
    for n in LAYOUT_LENGTHS:
        out.append(Group(f"layout-{n}", tuple(_layout_case(n, lay, 0) for lay in LAYOUTS)))
    out.append(Group("long-12288", (_long_case(12288, 12288, 1),)))      # (seed 0: e = 1.2e-10) the last list the fused kernel takes: 48 KB of dynamic LDS
    out.append(Group("long-12289", (_long_case(12289, 300, 0),)))        # the automatic fallback to the record-walking kernel
    for name, prm in (("iter0", (1, 0, 2.0, -1.0, 1e-5)), ("iter1", (1, 1, 2.0, -1.0, 1e-5)), ("mu", (1, 15, 2.0, 1e-3, 1e-5))):
        out.append(Group(f"loop-{name}", tuple(_count_case(f"loop-{name}", LOOP_COUNT, si, prm, True, 0) for si in range(3))))
    return tuple(out)


def group(name):
    return next(g for g in groups() if g.name == name)


def group_names():
    return [g.name for g in groups()]


def all_cases():
    return [c for g in groups() for c in g.cases]


def case(name):
    return next(c for c in all_cases() if c.name == name)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------------------
def stats_tuple(st):
    return (st.initial_chi2, st.chi2, st.max_err, st.num_obs, st.status)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's result of a case in its given order, computed once: dict(T, stats = (initial_chi2, chi2, max_err, num_obs, status), trials, e)"""
    import oracle as O
    c = case(name)
    T, st, trials = O.motion_only_trace(c.res, cam_struct(), c.T0, params(c.prm))
    T.setflags(write=False)
    trials.setflags(write=False)
    return dict(T=T, stats=stats_tuple(st), trials=trials, e=O.motion_only_exposure(trials))


def bars(e):
    """pose: absolute; chi2: relative, initial and final; max_err: relative -- sharp where the case is decided, a sanity bound elsewhere (a flipped step moves it by
    about f / z e)"""
    return dict(pose=1e-9 + 2 * e, chi2=1e-9, max_err=1e-9 if e <= 1e-10 else 1e-4)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def measure(T, stats, ref):
    """differences of a result (pose 3 x 4, stats tuple) from a reference() record"""
    return dict(pose=float(np.abs(np.asarray(T).reshape(3, 4) - ref["T"]).max()), chi2=max(_rel(stats[0], ref["stats"][0]), _rel(stats[1], ref["stats"][1])),
                max_err=_rel(stats[2], ref["stats"][2]))


def check(T, stats, ref, what):
    """a result against the bars of the reference; returns the measured differences"""
    m, bar = measure(T, stats, ref), bars(ref["e"])
    assert tuple(stats[3:]) == tuple(ref["stats"][3:]), (what, "num_obs / status", stats[3:], ref["stats"][3:])
    for k in ("pose", "chi2", "max_err"):
        assert m[k] <= bar[k], (what, k, m[k], bar[k], "e", ref["e"])
    return m


# ---- the mixed batch of tests/test_gpu_motion_edges.py: its lists, so that the CPU test can hold the oracle's side of it ----------------------------------
MIXED_OK = (0, 5, 19, 20, 300, 1537)
MIXED_LENGTH = 1600
MIXED_MIN_OBS = 20


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """streams of 0, 5, 19, 20, 300 and 1537 OK records scattered over 1600, and a seventh whose OK record 100 has a NaN observation; one start pose each (near)"""
    lists, starts = [], []
    for k, n_ok in enumerate(MIXED_OK + (300,)):
        rng = np.random.default_rng([SEED, 77, k])
        T_true = _truth(rng)
        res = synthetic_results(rng, cam(), T_true, MIXED_LENGTH, n_fail=0)
        res["status"] = rng.integers(1, 7, MIXED_LENGTH)
        ok = np.sort(rng.choice(MIXED_LENGTH, n_ok, replace=False))
        res["status"][ok] = 0
        if k == len(MIXED_OK):
            res["obs"][ok[100], 1] = np.nan
        lists.append(res)
        starts.append(_start(rng, T_true, "near"))
    return np.stack(lists), np.stack(starts)
