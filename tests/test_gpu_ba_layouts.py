"""Every layout of the BA Schur kernel and the LM trial step behind the solve, against the CPU oracle.

ba_landmark_kernel<MODE, NW, WC> runs with NW = 4..8 waves per workgroup and, at four waves, the big (one workgroup per CU, 22-pose LDS
window) or the small LDS pool (two per CU, 16 poses); svs_ba_schur_layout reports the layout the next launches take, and every case here
asserts the one it means to test.  Each case checks
  * the reduced camera system at lambda = 50 and 0.7 against O.ba_reduced_system, and
  * svs_ba_trial -- the MODE 1 launches (constraints' trial chi2, back-substitution x_l = D^-1 (b_l - W^T x_p), trial chi2, the landmark
    share of the LM scale) behind the trial poses exp(x_p) T -- at x_p = the solution of the oracle's system, against O.ba_trial.
Two families: (1) a window of hard landmark shapes (tests/ba_shapes.py) with "nw" forced to every layout, crossed with the self-edge
modes, fused / stand-alone constraints, "group", and robust off / Huber 0.3, 1, 3; (2) synth.ba_window sized from the CU count so that
pick_nw itself lands in every band, three of them also through a whole optimize() against O.ba_optimize.
"""
import numpy as np
import pytest

import ba_shapes

pytestmark = pytest.mark.gpu

# Bars, each with the maximum measured over all cases of this module on MI355X (f64 throughout; the GPU sums in another order than the
# oracle).  The reduced system also keeps the bar of test_reduced_system_matches_oracle, 1e-10 max|H_ref| (measured 1.7e-13).
C_H = 1e-11       # |dH_ij| <= C_H sqrt(H_ii H_jj) of the oracle's matrix (+ lambda I): measured 2.6e-13
R_POSE = 1e-14    # trial poses, relative to the largest entry of each pose: measured 4.0e-15
R_LM = 1e-10      # trial landmarks, relative to the landmark's |x_l| (floor: 1e-6 of the largest |x_l|): measured 1.4e-11
R_CHI = 1e-11     # trial chi2 and the landmark share of the scale, relative: measured 5.5e-14 and 1.6e-14

RAN = {}          # kernel variant -> cases that launched it (the coverage table printed by the last test)
MEASURED = {}


def _cam(c):
    from scavislam_amd.ctypes_types import Cam
    return Cam(c["f"], c["cx"], c["cy"], c["b"], c["w"], c["h"])


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


def _record(opt, name, nw, big):
    RAN.setdefault(f"ba_landmark_kernel<0, {nw}, {2 if big else 1}>", []).append(name)
    RAN.setdefault(f"ba_landmark_kernel<1, {nw}>", []).append(name)
    if opt.info()["wide_landmarks"] > 0:
        RAN.setdefault("ba_wide_landmark_kernel<0>", []).append(name)
        RAN.setdefault("ba_wide_landmark_kernel<1>", []).append(name)


def _check_system_and_trial(opt, prob, cons, cam, prm, lams=(50.0, 0.7)):
    """reduced system and trial at every lambda against the oracle; returns nothing, asserts the bars"""
    import oracle as O
    args = (prob["poses"], prob["psi"], prob["edges"], cons, cam, prm)
    chi2_ref = O.ba_chi2(*args)
    for lam in lams:
        H, b, chi2 = opt.reduced_system(lam)
        H_ref, b_ref = O.ba_reduced_system(*args, lam)
        dH = np.abs(H - H_ref)
        assert np.allclose(H, H.T)
        np.testing.assert_allclose(H, H_ref, rtol=0, atol=1e-10 * np.abs(H_ref).max())
        d = np.sqrt(np.abs(np.diag(H_ref)))
        sf = dH / np.outer(d, d)
        _note("H scale-free", sf.max())
        _note("H / max|H|", dH.max() / np.abs(H_ref).max())
        assert sf.max() <= C_H, f"scale-free bar: {sf.max():.3g} at {np.unravel_index(sf.argmax(), sf.shape)}"
        np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-10 * np.abs(b_ref).max())
        np.testing.assert_allclose(chi2, chi2_ref, rtol=1e-12)
        # the trial from the oracle's own solution of that system
        xp = np.linalg.solve(H_ref, b_ref)
        poses_t, psi_t, chi_t, scl = opt.trial(lam, xp)
        poses_r, psi_r, chi_r, scl_r = O.ba_trial(*args, lam, xp)
        ep = (np.abs(poses_t - poses_r).max(1) / np.abs(poses_r).max(1)).max()
        _note("trial poses", ep)
        assert ep <= R_POSE, ep
        xl_r = psi_r - prob["psi"]
        nx = np.abs(xl_r).max(1)
        el = (np.abs(psi_t - psi_r).max(1) / np.maximum(nx, 1e-6 * nx.max())).max()
        _note("trial landmarks", el)
        assert el <= R_LM, el
        n_obs = np.bincount(prob["edges"]["point"], minlength=len(prob["psi"]))
        assert np.array_equal(psi_t[n_obs == 0], prob["psi"][n_obs == 0])           # landmarks without edges keep their value
        _note("trial chi2", abs(chi_t - chi_r) / abs(chi_r))
        _note("scale_l", abs(scl - scl_r) / abs(scl_r))
        np.testing.assert_allclose(chi_t, chi_r, rtol=R_CHI)
        np.testing.assert_allclose(scl, scl_r, rtol=R_CHI)
    # the trial leaves the current state alone
    poses, psi = opt.restoreDataFromG2o()
    assert np.array_equal(poses, prob["poses"]) and np.array_equal(psi, prob["psi"])


# ---- (1) hard shapes, every layout forced --------------------------------------------------------------------------------------------
LAYOUTS = [(4, True), (4, False), (5, True), (6, True), (7, True), (8, True)]
ROBUST = [None, 0.3, 1.0, 3.0]          # None: robust off
N_CONS = [0, 1, 24]


def _cases():
    out = []
    for li, (nw, big) in enumerate(LAYOUTS):
        for k, delta in enumerate(ROBUST):
            # a covering design: over its four cases every layout meets both self-edge modes, fused and stand-alone constraints (with
            # constraints present in each), "group" on and off, every robust setting and 0 / 1 / many constraints
            out.append(pytest.param(nw, big, delta, k & 1, (k >> 1) & 1, (k ^ (k >> 1)) & 1, N_CONS[(k + li) % 3],
                                    id=f"nw{nw}{'' if big else '-small'}-{'huber' + str(delta) if delta else 'plain'}-self{k & 1}"
                                       f"-{'unfused' if (k >> 1) & 1 else 'fused'}-{'group' if (k ^ (k >> 1)) & 1 else 'nogroup'}-c{N_CONS[(k + li) % 3]}"))
    return out


_HARD = {}


def _hard(big_window):
    key = big_window
    if key not in _HARD:
        # the small pool needs more than 4 x CUs wave chunks: the hard shapes plus a bulk of ordinary landmarks
        _HARD[key] = ba_shapes.hard_window(P=130, seed=7, n_bulk=60 * _n_cu() if big_window else 400, wide=True)
    return _HARD[key]


@pytest.mark.parametrize("nw,big,delta,self_mode,unfused,group,n_cons", _cases())
def test_hard_shapes_every_layout(gpu_ctx, nw, big, delta, self_mode, unfused, group, n_cons):
    """Tracks of 1..64 observations and wide ones (65, 128, P), anchors first / middle / last, pose spans around both LDS windows,
    landmarks with only a self edge or no edge, residuals on both sides of the Huber delta: the reduced system and the trial against
    the oracle under a forced layout."""
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams
    ctx, stream = gpu_ctx
    prob = _hard(not big)
    cons = ba_shapes.constraints(prob, n_cons, seed=n_cons)
    cam = _cam(prob["cam"])
    prm = BaParams.reference_defaults()
    prm.self_edge_mode = self_mode
    prm.use_robust = 0 if delta is None else 1
    if delta is not None:
        prm.huber_delta = delta
    opt = SlamGraphOptimizer(ctx, stream)
    opt.set_option("nw", nw)
    opt.set_option("no_fused_cons", unfused)
    opt.set_option("group", 3 if group else 0)
    opt.set_option("host_marshal", 1)                 # the host layout (the one "group" applies to) at every size
    opt.copyDataToG2o(prob["poses"], prob["psi"], prob["edges"], cons, cam, prm)
    assert opt.schur_layout() == (nw, big), (opt.schur_layout(), opt.info())
    assert opt.info()["wide_landmarks"] == 9
    _check_system_and_trial(opt, prob, cons, cam, prm)
    _record(opt, f"hard nw{nw}{'' if big else '-small'}", nw, big)
    opt.close()


# ---- (2) natural bands of pick_nw ----------------------------------------------------------------------------------------------------
BANDS = [(4, True, 3.0), (5, True, 4.5), (6, True, 5.5), (7, True, 6.5), (8, True, 7.5), (4, False, 8.6)]      # target chunks / CU


@pytest.fixture(scope="module")
def band_window():
    """one synth.ba_window big enough for the widest band; each band takes a prefix of its landmarks (they are independent), sized from
    the chunks per landmark of the whole window"""
    import torch  # noqa: F401
    from scavislam_amd import capi, synth
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams
    n_cu = _n_cu()
    prob = synth.ba_window(50, int(8.8 * n_cu * 12), seed=2012)
    ctx, stream = capi.torch_context(0)
    opt = SlamGraphOptimizer(ctx, stream)
    opt.copyDataToG2o(prob["poses"], prob["psi"], prob["edges"], prob["cons"], _cam(prob["cam"]), BaParams.reference_defaults())
    per_lm = opt.info()["wave_chunks"] / len(prob["psi"])
    opt.close()
    ctx.close()
    return prob, per_lm, n_cu


def _prefix(prob, L):
    e = prob["edges"]
    return dict(prob, psi=prob["psi"][:L], edges=e[e["point"] < L])


@pytest.mark.parametrize("nw,big,target", BANDS, ids=[f"nw{b[0]}{'' if b[1] else '-small'}" for b in BANDS])
def test_natural_band(gpu_ctx, band_window, nw, big, target):
    """A plain window whose size puts pick_nw in the band (no option): reduced system and trial against the oracle; in the 5, 6 and 8
    bands (the never-compared ones) also optimize() against O.ba_optimize with the bars of test_optimize_matches_oracle -- after the
    trial, which must have left the state alone."""
    import oracle as O
    from scavislam_amd.backend import SlamGraphOptimizer
    from scavislam_amd.ctypes_types import BaParams
    ctx, stream = gpu_ctx
    full, per_lm, n_cu = band_window
    prob = _prefix(full, int(target * n_cu / per_lm))
    cam = _cam(prob["cam"])
    prm = BaParams.reference_defaults()
    opt = SlamGraphOptimizer(ctx, stream)
    opt.copyDataToG2o(prob["poses"], prob["psi"], prob["edges"], prob["cons"], cam, prm)
    assert opt.schur_layout() == (nw, big), (opt.schur_layout(), opt.info(), len(prob["edges"]))
    _check_system_and_trial(opt, prob, prob["cons"], cam, prm)
    _record(opt, f"band nw{nw}{'' if big else '-small'}", nw, big)
    if nw in (5, 6, 8):
        st = opt.optimize()
        poses, psi = opt.restoreDataFromG2o()
        poses_ref, psi_ref, st_ref = O.ba_optimize(prob["poses"], prob["psi"], prob["edges"], prob["cons"], cam, prm)
        assert (st.iterations, st.trials, st.accepted, st.terminated) == (st_ref.iterations, st_ref.trials, st_ref.accepted, st_ref.terminated)
        np.testing.assert_allclose(st.chi2_init, st_ref.chi2_init, rtol=1e-12)
        np.testing.assert_allclose(st.chi2_final, st_ref.chi2_final, rtol=1e-9)
        np.testing.assert_allclose(st.lambda_final, st_ref.lambda_final, rtol=1e-6)
        assert st_ref.accepted >= 1 and st_ref.chi2_final < st_ref.chi2_init
        for new, ref, start in ((poses, poses_ref, prob["poses"]), (psi, psi_ref, prob["psi"])):
            assert np.abs(new - ref).max() / np.abs(ref - start).max() < 1e-6
    opt.close()


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
KERNELS = [f"ba_landmark_kernel<0, {nw}, {2 if big else 1}>" for nw, big in LAYOUTS] + [f"ba_landmark_kernel<1, {nw}>" for nw in range(4, 9)] + \
          ["ba_wide_landmark_kernel<0>", "ba_wide_landmark_kernel<1>"]


def test_every_schur_kernel_variant_ran():
    """The eleven landmark-kernel variants (six MODE 0, five MODE 1) and the wide-landmark kernel in both modes were each launched and
    checked by the cases above (run the whole module)."""
    print("\nSchur kernel coverage of this module:")
    for k in KERNELS:
        print(f"  {k:32s} {len(RAN.get(k, [])):3d} cases  ({', '.join(sorted(set(RAN.get(k, []))))})")
    print("measured maxima:", ", ".join(f"{k} {v:.3g}" for k, v in MEASURED.items()))
    missing = [k for k in KERNELS if not RAN.get(k)]
    assert not missing, f"never launched: {missing}"
