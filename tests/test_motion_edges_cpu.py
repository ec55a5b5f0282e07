"""The yardstick of the motion-only edge tests, held to itself: the oracle alone against the bars of tests/motion_cases.py (no GPU).

  * oracle.motion_only_trace is oracle.motion_only (same bits) and its records replay to the final pose;
  * the oracle on a list in its given order, reversed and in six seeded shuffles -- exact-arithmetic equals -- stays within the bars of the given order: pose
    1e-9 + 2 e, chi2 1e-9 relative, max_err 1e-9 relative where e <= 1e-10.  A bar that the reference misses against itself could be asked of no kernel;
  * the cases are worth their names: most are decided (e small), and every count, layout and long list has a decided case, so that the sharp 1e-9 pose bar is met
    at every edge;
  * tests/np_model.motion_only, which shares no code with the oracle, agrees with it within the same bars on the short lists.

Measured maxima: profiles/motion_edges.md."""
import functools

import numpy as np
import pytest

import motion_cases as MC

N_SHUFFLES = 6


@functools.lru_cache(maxsize=None)
def _orders(name):
    """results of the oracle on the permuted lists of a case: [(T, stats tuple)]"""
    import oracle as O
    c = MC.case(name)
    n = len(c.res)
    perms = [np.arange(n)[::-1]] + [np.random.default_rng([11, k, n]).permutation(n) for k in range(N_SHUFFLES)]
    out = []
    for p in perms:
        T, st = O.motion_only(c.res[p], MC.cam_struct(), c.T0, MC.params(c.prm))
        out.append((T, MC.stats_tuple(st)))
    return out


@pytest.mark.parametrize("gname", MC.group_names())
def test_trace_is_the_oracle_and_replays(gname):
    import oracle as O
    import np_model as M
    for c in MC.group(gname).cases:
        ref = MC.reference(c.name)
        T, st = O.motion_only(c.res, MC.cam_struct(), c.T0, MC.params(c.prm))
        assert T.tobytes() == ref["T"].tobytes() and MC.stats_tuple(st) == ref["stats"], c.name
        tr = ref["trials"]
        assert ref["stats"][4] == 0 and ref["stats"][3] == c.tags["count"] == int((c.res["status"] == 0).sum())
        assert len(tr) >= min(c.prm[1], 1) and tr["accepted"].sum() <= c.prm[1]
        assert np.array_equal(tr["rho"], tr["chi2"] - tr["new_chi2"]) and np.array_equal(tr["accepted"] != 0, tr["rho"] > 0)
        assert np.array_equal(tr["step"], np.abs(tr["delta"]).max(axis=1))
        # the accepted steps, composed by the NumPy model's own exp and product, end at the final pose: <= 15 products of entries <= ~15, a few ulp each
        Tr = np.asarray(c.T0, np.float64)
        chi2 = ref["stats"][0]
        for t in tr:
            assert t["chi2"] == chi2, c.name
            if t["accepted"]:
                Tr, chi2 = M.pose_mul(M.se3_exp(t["delta"]), Tr), t["new_chi2"]
        assert chi2 == ref["stats"][1]
        np.testing.assert_allclose(Tr, ref["T"], rtol=0, atol=1e-12, err_msg=c.name)


@pytest.mark.parametrize("gname", MC.group_names())
def test_oracle_under_permutations_keeps_its_bars(gname):
    for c in MC.group(gname).cases:
        ref = MC.reference(c.name)
        for k, (T, stats) in enumerate(_orders(c.name)):
            MC.check(T, stats, ref, (c.name, "order", k))


def test_conditions():
    """the cases are decided where the issue of a sharp bar needs them to be"""
    cases = MC.all_cases()
    e = {c.name: MC.reference(c.name)["e"] for c in cases}
    robust = [c for c in cases if c.prm[0] == 1]
    loose = [c.name for c in robust if e[c.name] > 1e-9]
    assert len(loose) <= 0.15 * len(robust), (len(loose), len(robust), loose)
    for n in MC.COUNTS:
        assert any(e[c.name] <= 1e-10 for c in cases if c.tags["kind"] == "count" and c.tags["count"] == n), ("count", n)
    for lay in MC.LAYOUTS:
        assert any(e[c.name] <= 1e-10 for c in cases if c.tags.get("layout") == lay), ("layout", lay)
    for n in (12288, 12289):
        assert e[f"long-{n}"] <= 1e-10, ("long", n, e[f"long-{n}"])
    for n in MC.PLAIN_COUNTS:
        assert any(e[c.name] <= 1e-9 for c in cases if c.tags["kind"] == "plain" and c.tags["count"] == n), ("plain", n)
    # the layouts are what they are called
    for n in MC.LAYOUT_LENGTHS:
        g = {c.tags["layout"]: c.res["status"] for c in MC.group(f"layout-{n}").cases}
        assert (g["last_only"] == 0).nonzero()[0].tolist() == [n - 1] and (g["first_only"] == 0).nonzero()[0].tolist() == [0]
        ok = (g["round_rejected"] == 0).nonzero()[0]
        assert (ok[0], len(ok)) == {2047: (1977, 70), 2048: (1978, 70), 2049: (2048, 1), 4097: (2048, 70)}[n]
        assert (g["alternating"][0::2] == 0).all() and (g["alternating"][1::2] != 0).all()
        assert (g["wave_rejected"] != 0).sum() == 64 and (g["wave_rejected"][320:384] != 0).all()
        assert set(np.unique(g["random_statuses"])) == set(range(7))
    # the hostile points are there
    for c in cases:
        if c.tags["kind"] == "count" and c.tags["count"] >= MC.HOSTILE_FROM:
            z = c.res["xyz_actkey"][:, 2]
            assert (z < -1.9).sum() == 2 and (z > 2000).sum() == 2, c.name


@pytest.mark.parametrize("gname", [g.name for g in MC.groups() if all(c.tags["kind"] in ("count", "plain") and c.tags["count"] <= 257 for c in g.cases)])
def test_numpy_model_agrees_with_the_oracle(gname):
    import np_model as M
    cam = MC.cam()
    for c in MC.group(gname).cases:
        ref = MC.reference(c.name)
        ok = c.res["status"] == 0
        T, init, chi2 = M.motion_only(c.res["xyz_actkey"][ok], c.res["obs"][ok], (cam["f"], cam["cx"], cam["cy"], cam["b"]), np.asarray(c.T0, np.float64),
                                      robust=bool(c.prm[0]), b=c.prm[2], num_iter=c.prm[1], tau=c.prm[4])
        # the model reports no max_err, no count and no status: those members are the reference's own
        MC.check(T, (init, chi2) + ref["stats"][2:], ref, (c.name, "np_model"))


def test_mixed_batch_in_the_oracle():
    """the oracle's side of the GPU test's mixed batch: an empty list is status 1, a NaN observation status 2 with the input pose, the rest refine"""
    import oracle as O
    lists, starts = MC.mixed_batch()
    want = [1, 0, 0, 0, 0, 0, 2]
    for k, (res, T0) in enumerate(zip(lists, starts)):
        T, st = O.motion_only(res, MC.cam_struct(), T0, MC.params(MC.REFERENCE_PRM))
        assert st.status == want[k] and st.num_obs == (MC.MIXED_OK + (300,))[k]
        if want[k]:
            assert T.tobytes() == np.asarray(T0, np.float64).tobytes()
        else:
            assert st.chi2 < st.initial_chi2
