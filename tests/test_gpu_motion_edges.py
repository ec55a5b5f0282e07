"""svs_motion_only at the edges of its two kernels, against the oracle and the oracle's own yardstick (tests/motion_cases.py).

Every group of cases is ONE batched call per route -- the fused kernel with and without its speculative chi2-only sweeps ("mo_spec" 1 / 0) and the record-walking
kernel ("mo_legacy") -- with streams that carry different lists and start poses, a batch stride 37 records longer than the list, status-OK records with NaN
observations in the gaps (a kernel that reads one ends in status 2) and two guard slots behind the poses and the statistics.  The bars are those the oracle keeps
against itself under permutations of its list (tests/test_motion_edges_cpu.py): pose 1e-9 + 2 e with the case's exposure e from oracle.motion_only_trace, chi2 1e-9
relative, num_obs and status equal.  Measured differences: profiles/motion_edges.md (every test prints its figures before it asserts)."""
import ctypes as C

import numpy as np
import pytest

import motion_cases as MC

pytestmark = pytest.mark.gpu

ROUTES = (("spec1", dict(mo_spec=1, mo_legacy=0)), ("spec0", dict(mo_spec=0, mo_legacy=0)), ("legacy", dict(mo_spec=1, mo_legacy=1)))
PAD = 37
GUARD = 0xA5


def _device_run(gpu_ctx, lists, starts, prm, route):
    """lists [B][n] records, starts [B][3][4]; returns (poses [B][3][4], [stats tuple], raw bytes of poses and statistics with their guard slots)"""
    import torch
    from scavislam_amd.ctypes_types import MATCH_RESULT_DTYPE, PoseOptStats
    ctx, stream = gpu_ctx
    B, n = lists.shape
    buf = np.zeros((B, n + PAD), MATCH_RESULT_DTYPE)
    buf["obs"] = np.nan                                    # the gaps: OK records that no kernel may read
    buf["xyz_actkey"] = (0.5, -0.25, 5.0)
    buf[:, :n] = lists
    sz = C.sizeof(PoseOptStats)
    T = np.full((B + 2) * 96, GUARD, np.uint8)
    T[:B * 96] = np.ascontiguousarray(starts, np.float64).reshape(-1).view(np.uint8)
    with torch.cuda.stream(stream):
        d_res = torch.as_tensor(buf.view(np.uint8).reshape(-1)).cuda()
        d_T = torch.as_tensor(T).cuda()
        d_st = torch.full(((B + 2) * sz,), GUARD, dtype=torch.uint8, device="cuda")
    camc = MC.cam_struct()
    for k, v in route.items():
        ctx.set_option(k, v)
    try:
        ctx.call("svs_motion_only", d_res.data_ptr(), n, n + PAD, C.byref(camc), C.byref(prm), d_T.data_ptr(), d_st.data_ptr(), B)
        ctx.sync()
    finally:
        ctx.set_option("mo_spec", 1)
        ctx.set_option("mo_legacy", 0)
    rawT, rawS = d_T.cpu().numpy(), d_st.cpu().numpy()
    assert (rawT[B * 96:] == GUARD).all() and (rawS[B * sz:] == GUARD).all(), "guard slots behind the batch were written"
    stats = [MC.stats_tuple(PoseOptStats.from_buffer_copy(rawS[i * sz:(i + 1) * sz].tobytes())) for i in range(B)]
    return rawT[:B * 96].view(np.float64).reshape(B, 3, 4).copy(), stats, rawT.tobytes() + rawS.tobytes()


def _all_routes(gpu_ctx, lists, starts, prm):
    return {name: _device_run(gpu_ctx, lists, starts, prm, opts) for name, opts in ROUTES}


@pytest.mark.parametrize("gname", MC.group_names())
def test_every_route_within_the_oracles_bars(gpu_ctx, gname):
    """counts around a wave, a workgroup, the register file and a compaction round; layouts of rejected records; the longest list of the fused kernel and the
    automatic fallback behind it; loop limits"""
    g = MC.group(gname)
    lists = np.stack([c.res for c in g.cases])
    starts = np.stack([c.T0 for c in g.cases])
    out = _all_routes(gpu_ctx, lists, starts, MC.params(g.cases[0].prm))
    refs = [MC.reference(c.name) for c in g.cases]
    for route, (T, stats, raw) in out.items():
        for b, (c, ref) in enumerate(zip(g.cases, refs)):
            m = MC.measure(T[b], stats[b], ref)
            print(f"MOEDGE {route} {c.name} e {ref['e']:.3e} pose {m['pose']:.3e} bar {MC.bars(ref['e'])['pose']:.3e} chi2 {m['chi2']:.3e} max_err {m['max_err']:.3e}")
    assert out["spec1"][2] == out["spec0"][2], "speculative trials changed the bits"
    if len(lists[0]) * 4 > 48 * 1024:
        assert out["spec1"][2] == out["legacy"][2], "a list beyond 48 KB of indices is the record-walking kernel's whatever mo_legacy says"
    for route, (T, stats, raw) in out.items():
        for b, (c, ref) in enumerate(zip(g.cases, refs)):
            MC.check(T[b], stats[b], ref, (route, c.name))


def test_mixed_batch_statuses(gpu_ctx):
    """streams of 0, 5, 19, 20, 300 and 1537 OK records and one with a NaN observation, min_obs = 20: statuses 1, 3, 3, 0, 0, 0, 2.  Status 1, 2 and 3 leave the pose
    bits; status 3 reports the list as it stands (num_obs, initial_chi2 == chi2: the header's contract -- the oracle has no min_obs, so the expectation is its run
    with num_iter = 0); the NaN stream leaves its neighbours' bytes what they are without it."""
    import oracle as O
    lists, starts = MC.mixed_batch()
    prm = MC.params(MC.REFERENCE_PRM, MC.MIXED_MIN_OBS)
    want = [1, 3, 3, 0, 0, 0, 2]
    n_ok = list(MC.MIXED_OK) + [300]
    clean = lists.copy()
    clean["obs"][6] = np.where(np.isnan(clean["obs"][6]), 100.0, clean["obs"][6])
    out, out_clean = _all_routes(gpu_ctx, lists, starts, prm), _all_routes(gpu_ctx, clean, starts, prm)
    assert out["spec1"][2] == out["spec0"][2]
    camc = MC.cam_struct()
    for route, (T, stats, raw) in out.items():
        Tc, stats_c, _ = out_clean[route]
        assert [s[4] for s in stats] == want and [s[3] for s in stats] == n_ok, (route, stats)
        assert T[:6].tobytes() == Tc[:6].tobytes() and stats[:6] == stats_c[:6] and stats_c[6][4] == 0, (route, "the NaN stream disturbed its neighbours")
        for b in range(7):
            if want[b] != 0:
                assert T[b].tobytes() == np.asarray(starts[b], np.float64).tobytes(), (route, b, "pose bits touched")
            if want[b] == 1:
                assert stats[b][:3] == (0.0, 0.0, 0.0), (route, stats[b])
            elif want[b] == 3:
                _, s0 = O.motion_only(lists[b], camc, starts[b], MC.params((1, 0, 2.0, -1.0, 1e-5)))
                assert stats[b][0] == stats[b][1], (route, b)
                np.testing.assert_allclose(stats[b][:3], [s0.initial_chi2, s0.chi2, s0.max_err], rtol=1e-9)
            elif want[b] == 2:
                _, s2 = O.motion_only(lists[b], camc, starts[b], MC.params(MC.REFERENCE_PRM))
                assert s2.status == 2 and np.isnan(stats[b][0]) and np.isnan(stats[b][1])
            else:
                Tr, sr, trials = O.motion_only_trace(lists[b], camc, starts[b], MC.params(MC.REFERENCE_PRM))
                ref = dict(T=Tr, stats=MC.stats_tuple(sr), e=O.motion_only_exposure(trials))
                m = MC.measure(T[b], stats[b], ref)
                print(f"MOEDGE {route} mixed-{n_ok[b]} e {ref['e']:.3e} pose {m['pose']:.3e} bar {MC.bars(ref['e'])['pose']:.3e} chi2 {m['chi2']:.3e} max_err {m['max_err']:.3e}")
                MC.check(T[b], stats[b], ref, (route, "mixed", b))


@pytest.mark.parametrize("gname", ["count-20", "count-257"])
def test_min_obs_boundary(gpu_ctx, gname):
    """min_obs equal to the count refines (the bytes of the run without a minimum); the count + 1 does not"""
    g = MC.group(gname)
    count = g.cases[0].tags["count"]
    lists, starts = np.stack([c.res for c in g.cases]), np.stack([c.T0 for c in g.cases])
    for name, opts in ROUTES:
        free = _device_run(gpu_ctx, lists, starts, MC.params(MC.REFERENCE_PRM, 0), opts)
        at = _device_run(gpu_ctx, lists, starts, MC.params(MC.REFERENCE_PRM, count), opts)
        above = _device_run(gpu_ctx, lists, starts, MC.params(MC.REFERENCE_PRM, count + 1), opts)
        assert at[2] == free[2] and all(s[4] == 0 for s in at[1]), name
        assert all(s[4] == 3 and s[3] == count and s[0] == s[1] for s in above[1]), (name, above[1])
        assert above[0].tobytes() == np.ascontiguousarray(starts, np.float64).tobytes(), name
        for b in range(len(lists)):
            assert above[1][b][0] == free[1][b][0], (name, b, "initial_chi2 of the untouched list")
