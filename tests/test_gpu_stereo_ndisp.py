"""Block matching over 16, 32, ..., 160 disparities (ui.num_disp16 = 1..10): stereo_bm_wide_kernel / stereo_bm_edge_kernel<64> of csrc/stereo_search.inc against the
oracle restatement of cv::StereoBM, bit for bit (np.array_equal everywhere: an integer pipeline).  tests/test_gpu_stereo_paths.py walks the dispatch at 32
disparities; here the disparity count varies.  Input: the banded noise pair of tests/stereo_ndisp_cases.py, whose winners cover the whole search range
(tests/test_stereo_ndisp_cpu.py pins the oracle to the NumPy model on it), and noise against its own roll.

The library hands out the float disparity only.  The stages are therefore compared through three parameter sets per case: without left-right check and speckle
filter the result IS the raw 16-bit plane (/ 16); with the left-right check alone it is the plane after validateDisparity, which depends on the COST plane of
the search (a strictly smaller cost wins a column); with both it is the final plane.  Which search ran is asserted through "stereo_wide_search_calls".

The wide search gives a wave WIDE_TILE = 64 output columns and WIDE_STRIP = 48 output rows, and the edge kernel a workgroup 64 rows of the three leftmost
searched columns; 16 disparities are one group of the runtime loop and a quarter of the edge kernel's lanes, 160 are ten groups and three lane chunks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_cases as SC
import stereo_ndisp_cases as NC
import test_gpu_stereo_paths as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE, STRIP = 64, 48      # csrc/stereo.hip: WIDE_TILE, WIDE_STRIP (the constants the host shares with csrc/stereo_search.inc)
WIDE = "stereo_wide_search_calls"
RAW = dict(disp12_max_diff=-1, speckle_window=0)      # the raw plane of the search
LR = dict(speckle_window=0)                           # ... after the left-right check (cost plane)


def _run(gpu_ctx, pairs, prm, **layout):
    """-> (results, steps of the path counters incl. the wide search's)"""
    ctx, _ = gpu_ctx
    before = ctx.get_stat(WIDE)
    got, d = P._run(gpu_ctx, pairs, prm, **layout)
    d[WIDE] = ctx.get_stat(WIDE) - before
    return got, d


def _f32(plane16):
    return plane16.astype(np.float32) / 16


def _assert_stages(gpu_ctx, ndisp, l, r, stages, window, what="", **kw):
    """the GPU's raw plane, the plane after the left-right check and the final plane (speckle window `window`) equal the oracle's `stages`"""
    for name, over, ref in (("raw", RAW, stages[0]), ("left-right", LR, stages[1]), ("final", dict(speckle_window=window), stages[2])):
        prm = NC.params(ndisp, **dict(kw, **over))
        got, d = _run(gpu_ctx, [(l, r)], prm)
        assert d[WIDE] == 1
        g = got[0]
        assert g.dtype == np.float32 and np.array_equal(g, _f32(ref)), \
            f"{what} {ndisp} disparities, {name} plane: {(g != _f32(ref)).sum()} px differ from the oracle, first at {np.argwhere(g != _f32(ref))[:4].tolist()}"


# ---- a. counts and the full pipeline ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndisp", [16, 48, 64, 112, 160])
def test_full_pipeline_on_the_banded_pair(gpu_ctx, ndisp):
    """(N + 71) x 101 at the reference parameters: 72 searched columns (three of the edge kernel, 64 + 5 of the wave kernel: two tiles), three strips of rows.
    Oracle alone (valid / removed by the left-right check / kept / removed by the speckle filter / kept values >= 32 px):
    16: 6802 / 10 / 6672 / 120 / 0;  48: 6618 / 59 / 6425 / 134 / 1756;  64: 6390 / 39 / 6177 / 174 / 2848;  160: 6222 / 30 / 5949 / 243 / 4322
    (tests/test_stereo_ndisp_cpu.py asserts these); 112 is held to the same floors: >= 5000 / >= 5 / - / >= 100 / >= 1000."""
    import oracle as O
    l, r = NC.banded_pair(ndisp)
    stages = NC.oracle_stages(ndisp)
    c = NC.assert_has_work(stages, ndisp)
    if ndisp in NC.MODEL_COUNTS:
        assert c == NC.MODEL_COUNTS[ndisp]
    prm = NC.params(ndisp)
    _assert_stages(gpu_ctx, ndisp, l, r, stages, prm.speckle_window)
    got, d = _run(gpu_ctx, [(l, r)], prm)
    assert d[WIDE] == 1 and np.array_equal(got[0], O.stereo_bm(l, r, prm))
    assert got[0].max() < ndisp and (got[0][:, :ndisp - 1] == -1).all()


# ---- b. the parameters at 64 disparities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(uniqueness_ratio=0), dict(uniqueness_ratio=60), dict(texture_threshold=0), dict(texture_threshold=400),
                                dict(disp12_max_diff=-1), dict(disp12_max_diff=0), dict(disp12_max_diff=4), dict(speckle_window=0, speckle_range=8),
                                dict(speckle_window=3000, speckle_range=512), dict(prefilter_cap=41), dict(prefilter_cap=42), dict(prefilter_cap=63)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_parameters_at_64_disparities(gpu_ctx, kw):
    """one parameter away from the reference set at a time on the banded pair (135 x 101): raw, left-right and final plane each.  Caps 41 / 42 are where the
    32-disparity kernel changes its key width (the wide search has one width: 32 bits); 63 gives the largest sums, 49 * 126 = 6174.  On noise texture_threshold
    400 removes nothing and speckle_window 3000 little (oracle: 84 px) -- the expected planes are the oracle's whatever they hold; uniqueness_ratio 60 leaves 4985
    raw pixels of 6390, 0 makes all 7272 valid."""
    ndisp = 64
    l, r = NC.banded_pair(ndisp)
    NC.assert_has_work(NC.oracle_stages(ndisp), ndisp)      # the input at the reference parameters
    prm = NC.params(ndisp, **kw)
    stages = SC.stages(l, r, prm)
    if "texture_threshold" not in kw or kw["texture_threshold"] == 0:
        assert (stages[0] != -16).sum() >= 4000, (stages[0] != -16).sum()
    over = {k: v for k, v in kw.items() if k not in ("disp12_max_diff", "speckle_window")}
    # the raw plane and (where the check is on) the left-right plane under these parameters, then the set itself
    cases = [("raw", dict(over, **RAW), stages[0])]
    if prm.disp12_max_diff >= 0:
        cases.append(("left-right", dict(over, disp12_max_diff=prm.disp12_max_diff, speckle_window=0), stages[1]))
    cases.append(("final", kw, stages[2]))
    for name, k, ref in cases:
        got, d = _run(gpu_ctx, [(l, r)], NC.params(ndisp, **k))
        assert d[WIDE] == 1
        assert np.array_equal(got[0], _f32(ref)), f"{kw}, {name} plane: {(got[0] != _f32(ref)).sum()} px differ, first at {np.argwhere(got[0] != _f32(ref))[:4].tolist()}"


# ---- c. widths and heights -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndisp", [16, 160])
@pytest.mark.parametrize("dw", [6, 2 + TILE, 3 + TILE, 85])
def test_widths(gpu_ctx, ndisp, dw):
    """w = N + 6, the narrowest frame (three edge columns and four of the wave kernel); N + 2 + TILE, exactly one tile of the wave kernel; N + 3 + TILE, a tile
    and one column; N + 85 = 5 mod 16, odd and no multiple of 4 (a tile and 19 columns; single-pixel loads in the left-right check and the finish kernel).
    20 rows.  A frame this small is smaller than the reference's speckle window, which would remove everything: the final plane runs with window 10."""
    w, h = ndisp + dw, 20
    assert w % 4 != 0 or dw != 85
    l, r = NC.banded_pair(ndisp, w, h, seed=dw)
    stages = NC.oracle_stages(ndisp, w, h, seed=dw, speckle_window=10)
    assert (stages[0] != -16).sum() >= 0.4 * (dw - 5) * h and (stages[2] != -16).sum() >= 0.2 * (dw - 5) * h, NC.work(stages, ndisp)
    _assert_stages(gpu_ctx, ndisp, l, r, stages, 10, f"{w} x {h},")


@pytest.mark.parametrize("ndisp", [16, 160])
@pytest.mark.parametrize("h", [2, 5, STRIP, STRIP + 1])
def test_heights(gpu_ctx, ndisp, h):
    """2 rows, the shortest frame; 5, odd (the prefilter's flat last row); STRIP rows, one strip of the wave kernel exactly, and STRIP + 1.  N + 23 wide (odd).
    Speckle window 10 (see test_widths); at 2 and 5 rows the window rows clamp on both sides of every pixel."""
    w = ndisp + 23
    l, r = NC.banded_pair(ndisp, w, h, seed=h)
    stages = NC.oracle_stages(ndisp, w, h, seed=h, speckle_window=10)
    assert (stages[0] != -16).sum() >= 0.4 * 18 * h, NC.work(stages, ndisp)
    _assert_stages(gpu_ctx, ndisp, l, r, stages, 10, f"{w} x {h},")


# ---- d. winners at both ends of the range and in the middle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndisp", [16, 160])
def test_winner_at_both_ends_and_in_the_middle(gpu_ctx, ndisp):
    """noise against its own roll by 0, N / 2 and N - 1 pixels, uniqueness and texture tests off, (N + 71) x 101: at the ends the parabola mirrors its missing
    neighbour (s[-1] = s[1], s[N] = s[N-2]).  Oracle alone: every one of the 7272 searched pixels of the raw plane is valid and at least 7000 lie within half a
    pixel of the shift (the rest: the first searched columns, whose right window runs into the image border); at shifts 0 and N - 1 every valid pixel of the
    FINAL plane is the shift exactly, at least 7000 of them (7272 / 7173 at N = 16, 7254 / 7160 at N = 160)."""
    w, h = NC.size_for(ndisp)
    for shift in (0, ndisp // 2, ndisp - 1):
        l, r = SC.noise_roll_pair(w, h, shift, seed=ndisp + shift)
        kw = dict(uniqueness_ratio=0, texture_threshold=0)
        stages = SC.stages(l, r, NC.params(ndisp, **kw))
        raw, fin = stages[0][:, ndisp - 1:], stages[2]
        assert (raw != -16).sum() == 7272 and (np.abs(raw.astype(np.int32) - 16 * shift) <= 8).sum() >= 7000
        if shift in (0, ndisp - 1):
            assert (fin[fin != -16] == 16 * shift).all() and (fin != -16).sum() >= 7000
        _assert_stages(gpu_ctx, ndisp, l, r, stages, 100, f"shift {shift},", **kw)


# ---- e. definition D1: right-image columns past w - 1 read column w - 1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndisp", [16, 160])
def test_rightmost_column_reads_clamped_columns(gpu_ctx, ndisp):
    """the last searched column X = w - 1: its left window reads columns w .. w + 2 clamped, and at disparity index N - 1 (disparity 0) so does the right window.
    On the raw plane and on the plane after the left-right check (cost), column w - 1 and the two before it agree with the oracle, which has valid pixels there."""
    l, r = NC.banded_pair(ndisp)
    stages = NC.oracle_stages(ndisp)
    assert (stages[0][:, -1] != -16).sum() >= 20 and (stages[1][:, -1] != -16).sum() >= 20, (stages[0][:, -1] != -16).sum()
    for over, ref in ((RAW, stages[0]), (LR, stages[1])):
        got, d = _run(gpu_ctx, [(l, r)], NC.params(ndisp, **over))
        assert d[WIDE] == 1 and np.array_equal(got[0][:, -3:], _f32(ref)[:, -3:])


# ---- f. batches ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndisp,layout", [(48, {}), (160, {}), (48, dict(strides=(48 + 71 + 1, 48 + 71 + 7, 48 + 71 + 5), offsets=(1, 2), slack=(3, 9, 6), dguard=33))],
                         ids=["48", "160", "48-padded-unaligned"])
def test_batch_equals_frames_alone(gpu_ctx, ndisp, layout):
    """three different frames (banded pairs of seeds 0, 1, 2) in one call and the same frames one per call: bit-identical, and equal to the oracle.  The third
    case: row strides w + 1 / w + 7 / w + 5, pointers 1 and 2 bytes past a 16-byte boundary and slack between the slots (the 4-pixel prefilter kernel, asserted)."""
    pairs = [NC.banded_pair(ndisp, seed=s) for s in range(3)]
    prm = NC.params(ndisp)
    for s in range(3):
        NC.assert_has_work(NC.oracle_stages(ndisp, seed=s), ndisp)
    together, d = _run(gpu_ctx, pairs, prm, **layout)
    assert d[WIDE] == 1 and (not layout or (d["stereo_prefilter4_calls"] == 1 and d["stereo_prefilter16_calls"] == 0))
    for s, pair in enumerate(pairs):
        alone, d = _run(gpu_ctx, [pair], prm, **layout)
        assert d[WIDE] == 1
        assert np.array_equal(alone[0], together[s]), f"frame {s}: {(alone[0] != together[s]).sum()} px differ between the batch and the frame alone"
        assert np.array_equal(together[s], _f32(NC.oracle_stages(ndisp, seed=s)[2]))


# ---- g. 32 disparities through both searches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rendered-640x480", "banded"])
def test_wide_search_equals_register_ring_search_at_32(gpu_ctx, monkeypatch, which):
    """SVS_STEREO_WIDE=1 at create sends 32 disparities through the wide search: the same result as the register-ring kernels, on a rendered 640 x 480 pair
    (+-6 of noise) and on the banded pair (103 x 101), final and raw plane; the counter steps by one with the switch and not at all without it."""
    import oracle as O
    l, r = SC.rendered_pair(640, 480, 6, seed=1) if which.startswith("rendered") else NC.banded_pair(32)
    for over in ({}, RAW):
        prm = NC.params(32, **over)
        ref = O.stereo_bm(l, r, prm)
        assert (ref >= 0).mean() > 0.3
        ring, d = _run(gpu_ctx, [(l, r)], prm)
        assert d[WIDE] == 0
        with monkeypatch.context() as m:
            m.setenv("SVS_STEREO_WIDE", "1")
            wide, d = _run(gpu_ctx, [(l, r)], prm)
        assert d[WIDE] == 1
        assert np.array_equal(wide[0], ring[0]) and np.array_equal(wide[0], ref)
    got, d = _run(gpu_ctx, [NC.banded_pair(64)], NC.params(64))
    assert d[WIDE] == 1


# ---- h. what create refuses ------------------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_other_counts_and_narrow_frames(gpu_ctx):
    """0, 8, 40, 176 and -16 disparities, and 64 disparities at 69 pixels of width: SVS_ERR_UNSUPPORTED, nothing allocated, the accepted set (and for an accepted
    count the bound) in the message.  64 at 70 works and equals the oracle."""
    ctx, _ = gpu_ctx
    live = ctx.get_stat("live_device_bytes")
    for ndisp, w in ((0, 320), (8, 320), (40, 320), (176, 320), (-16, 320), (64, 69)):
        prm = NC.params(ndisp)
        h_ = C.c_void_p()
        rc = ctx.lib.svs_stereo_create(ctx.h, w, 20, 1, C.byref(prm), C.byref(h_))
        assert rc == P.SVS_ERR_UNSUPPORTED and not h_.value, (ndisp, w, rc)
        msg = ctx.lib.svs_last_error(ctx.h).decode()
        assert "16, 32, ..., 160" in msg and (ndisp != 64 or "70" in msg), msg
        assert ctx.get_stat("live_device_bytes") == live
    l, r = NC.banded_pair(64, 70, 20)
    stages = NC.oracle_stages(64, 70, 20, speckle_window=10)
    assert (stages[0] != -16).sum() >= 40
    _assert_stages(gpu_ctx, 64, l, r, stages, 10, "70 x 20,")


# ---- i. the layers above ---------------------------------------------------------------------------------------------------------------------------------------
def test_frontend_with_64_disparities(gpu_ctx):
    """a use_block_matching front end created with num_disp16 = 4 (FrontendParams.reference) at 160 x 128, the smallest size the front-end tests use (the front end
    wants multiples of 16): the disparity that svs_frontend_device_view hands out after processFirstFrame and after processFrame is the oracle's for that pair."""
    import oracle as O
    from scavislam_amd import capi
    from scavislam_amd.frontend import StereoFrontend
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE
    ctx, _ = gpu_ctx
    w, h, ndisp = 160, 128, 64
    cam = dict(f=0.9 * w, cx=w / 2.0, cy=h / 2.0, b=0.1, w=w, h=h)
    prm = capi.FrontendParams.reference(use_block_matching=True, num_disp16=4)
    assert prm.stereo.num_disparities == ndisp
    assert capi.FrontendParams.reference(use_block_matching=True).stereo.num_disparities == 32
    pairs = [NC.banded_pair(ndisp, w, h, seed=s) for s in (0, 1)]
    before = ctx.get_stat(WIDE)
    fe = StereoFrontend(ctx, cam, max_points=64, max_keyframes=2, params=prm)

    def disparity():
        p, stride = C.c_void_p(), (C.c_int32 * 3)()
        ctx.check(ctx.lib.svs_frontend_device_view(fe.h, 0, None, stride, C.byref(p), None, None))
        out = np.zeros((h, stride[0]), np.float32)
        ctx.call("svs_memcpy_d2h", out.ctypes.data, p, out.nbytes)
        return out[:, :w]

    I = np.eye(3, 4)
    try:
        fe.processFirstFrame(pairs[0][0], right=pairs[0][1])
        ref = O.stereo_bm(pairs[0][0], pairs[0][1], prm.stereo)
        assert (ref >= 32).sum() >= 1000 and np.array_equal(disparity(), ref)
        fe.keepKeyframe(0, I)
        fe.setCandidates(np.zeros(0, CANDIDATE_DTYPE), 0)
        fe.processFrame(pairs[1][0], I, I, right=pairs[1][1])
        ref = O.stereo_bm(pairs[1][0], pairs[1][1], prm.stereo)
        assert (ref >= 32).sum() >= 1000 and np.array_equal(disparity(), ref)
    finally:
        fe.close()
    assert ctx.get_stat(WIDE) - before == 2


def test_python_wrapper_takes_num_disp16(gpu_ctx):
    """StereoMatcher(ctx, frame, num_disp16=3) searches 48 disparities; without the argument 32, as before"""
    import oracle as O
    from scavislam_amd.frontend import FramePyramid, StereoMatcher
    from scavislam_amd import synth
    ctx, stream = gpu_ctx
    w, h = 128, 96
    l, r = NC.banded_pair(48, w, h)
    assert (O.stereo_bm(l, r, NC.params(48)) >= 32).sum() >= 500
    fr = FramePyramid(ctx, stream, dict(synth.CAM_DEFAULT, w=w, h=h, cx=w / 2.0, cy=h / 2.0), batch=1, with_float=False)
    fr.upload(np.array(l)[None])
    for k, ndisp in ((3, 48), (None, 32)):
        sm = StereoMatcher(ctx, fr) if k is None else StereoMatcher(ctx, fr, num_disp16=k)
        assert sm.params.num_disparities == ndisp
        sm.upload_right(np.array(r)[None])
        sm.calcDisparityCpu()
        assert np.array_equal(sm.disparity_host(0), O.stereo_bm(l, r, NC.params(ndisp)))
        sm.close()


def test_cpp_adaptor_with_64_disparities(tmp_path):
    """tests/cpp/stereo_ndisp_smoke.cpp: StereoBM(c, w, h, 4) of include/scavislam_hip.hpp on the banded pair (160 x 128) gives the plane the oracle wrote, with
    values beyond 32 in it; num_disp16 = 11 and a frame of 69 pixels are refused"""
    import oracle as O
    exe = tmp_path / "stereo_ndisp_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stereo_ndisp_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    w, h, ndisp = 160, 128, 64
    l, r = NC.banded_pair(ndisp, w, h)
    ref = O.stereo_bm(l, r, NC.params(ndisp))
    assert (ref >= 32).sum() >= 1000
    with open(tmp_path / "left.bin", "wb") as f:
        f.write(np.array([w, h], np.int32).tobytes())
        f.write(l.tobytes())
    (tmp_path / "right.bin").write_bytes(r.tobytes())
    (tmp_path / "want.bin").write_bytes(ref.tobytes())
    out = subprocess.check_output([str(exe), str(tmp_path / "left.bin"), str(tmp_path / "right.bin"), str(tmp_path / "want.bin"), "4"],
                                  stderr=subprocess.DEVNULL).decode().splitlines()
    tok = [ln for ln in out if ln.startswith("NDISP ")][0].split()
    assert [int(t) for t in tok[1:]] == [ndisp, 0, int((ref >= 0).sum()), int((ref >= 32).sum())], out
    assert [ln for ln in out if ln.startswith("REFUSED ")][0].split()[1:] == ["1", "1"], out
