"""The yardstick of tests/test_gpu_stereo_ndisp.py at the disparity counts no other test uses: oracle/stereo.c against the independent cost-volume model of
tests/np_model.py on the banded noise pair (tests/stereo_ndisp_cases.py), stage by stage, for 16, 48, 64 and 160 disparities -- and the counts that show the
input has work for every stage and winners beyond disparity 32.  Runs without a GPU."""
import numpy as np
import pytest

import np_model as M
import stereo_ndisp_cases as NC


@pytest.mark.parametrize("ndisp", [16, 48, 64, 160])
def test_oracle_matches_numpy_model_on_the_banded_pair(ndisp):
    """(N + 71) x 101, reference parameters: prefilter, raw block matching with its cost plane, left-right check, speckle filter and the float result are equal;
    the model's counts are those of NC.MODEL_COUNTS (valid / removed by the left-right check / kept / removed by the speckle filter / kept values >= 32 px):
    16: 6802 / 10 / 6672 / 120 / 0;  48: 6618 / 59 / 6425 / 134 / 1756;  64: 6390 / 39 / 6177 / 174 / 2848;  160: 6222 / 30 / 5949 / 243 / 4322."""
    import oracle as O
    l, r = NC.banded_pair(ndisp)
    assert l.shape == (101, ndisp + 71)
    prm = NC.params(ndisp)
    lp, rp = O.stereo_prefilter(l, prm.prefilter_cap), O.stereo_prefilter(r, prm.prefilter_cap)
    assert np.array_equal(lp, M.stereo_prefilter(l, prm.prefilter_cap)) and np.array_equal(rp, M.stereo_prefilter(r, prm.prefilter_cap))
    d16, cost = O.stereo_bm_core(lp, rp, prm)
    m16, mcost = M.stereo_bm_core(M.stereo_prefilter(l, 31), M.stereo_prefilter(r, 31), ndisp=ndisp)
    assert np.array_equal(d16, m16) and np.array_equal(cost, mcost)
    val = O.stereo_validate(d16, cost, prm)
    mval = M.stereo_validate(m16, mcost, ndisp=ndisp)
    assert np.array_equal(val, mval)
    fin = O.stereo_filter_speckles(val, -16, prm.speckle_window, prm.speckle_range)
    mfin = M.stereo_filter_speckles(mval, prm.speckle_window, prm.speckle_range)
    assert np.array_equal(fin, mfin)
    assert np.array_equal(O.stereo_bm(l, r, prm), M.stereo_bm(l, r, prm))
    assert np.array_equal(O.stereo_bm(l, r, prm), fin.astype(np.float32) / 16)
    assert NC.work((m16, mval, mfin), ndisp) == NC.MODEL_COUNTS[ndisp]
    assert NC.assert_has_work(NC.oracle_stages(ndisp), ndisp) == NC.MODEL_COUNTS[ndisp]
    assert (d16[:, :ndisp - 1] == -16).all() and (d16.max() >> 4) <= ndisp - 1
