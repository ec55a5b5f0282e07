"""The FAST score kernel's per-cell floor (fast.hip, context option "fast_floor"): the kernel pre-tests, scores, lists and histograms only from
max(t_lo, thr - 2 * max(trials - 1, 0)) up, thr being the cell's stored threshold of its stream in device memory when the kernel runs.  Nothing the detection
returns may change: corner lists (order included), per-cell counts, emit thresholds, threshold state and the matcher's corner bitmap must be the oracle's, and the
same with the option on and off.

322 x 242 frames (levels 322 x 242, 161 x 121, 81 x 61: cells of 107 x 80, 53 x 40 and 40 x 30 pixels, none a multiple of the 64 x 32 tile, six and two tiles
per cell on levels 0 and 1), three streams with different images and different starting thresholds: all cells 10 (the floor is clamped at t_lo), all 40 (fast_max:
the highest floor a cell can have), a ramp 10 .. 40 over the cells of a level (a floor per cell)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 322, 242
N_STREAMS = 3
N_FRAMES = 6
N_PTS = (40, 16, 8)            # 64 candidate points per stream


def _trials(i):
    return 5 if i == 0 else 6      # the first frame of a sequence uses 5 (stereo_frontend.cpp:131-136)


def _start_thr(s, nc):
    return [np.full(nc, 10), np.full(nc, 40), np.linspace(10, 40, nc).astype(int)][s].astype(np.int32)


_D = {}


def _data():
    """the streams' two frames (A, B), their pyramids, and the oracle's six-frame sequence A B A B A B from the three starting thresholds: computed once"""
    if _D:
        return _D
    import oracle as O
    from scavislam_amd import synth
    cam = dict(f=570.342 * W / 640, cx=0.5 * W, cy=0.5 * H, b=0.075, w=W, h=H)
    sc = synth.Scene(2011)
    traj = synth.trajectory(8)
    poses = [(traj[2 * s + 1], traj[2 * s + 2]) for s in range(N_STREAMS)]
    frames = [[sc.render(cam, T, seed=10 * s + k) for k, T in enumerate(poses[s])] for s in range(N_STREAMS)]       # [s][A / B] = (image, disparity)
    pyrs = [[O.build_pyramid(f[0]) for f in frames[s]] for s in range(N_STREAMS)]
    seq = []          # [frame][stream][level] = (xy, cell counts, emit thresholds, threshold state behind the frame)
    grids = [[O.fastgrid_for_level(pyrs[s][0][l].shape[1], pyrs[s][0][l].shape[0], l) for l in range(3)] for s in range(N_STREAMS)]
    for s in range(N_STREAMS):
        for l in range(3):
            nc = grids[s][l].gx * grids[s][l].gy
            grids[s][l].thr[:nc] = list(_start_thr(s, nc))
    floors = []       # every cell's floor in front of every frame: what the test covers
    for i in range(N_FRAMES):
        per_stream = []
        for s in range(N_STREAMS):
            per_level = []
            for l in range(3):
                g = grids[s][l]
                nc = g.gx * g.gy
                floors += [max(10, t - 2 * (_trials(i) - 1)) for t in g.thr[:nc]]
                xy, cc, et = O.fastgrid_detect_adaptively(g, pyrs[s][i & 1][l], _trials(i))
                per_level.append((xy, cc, et, np.array(g.thr[:nc], np.int32)))
            per_stream.append(per_level)
        seq.append(per_stream)
    _D.update(cam=cam, poses=poses, frames=frames, pyrs=pyrs, seq=seq, floors=np.array(floors))
    return _D


class _Pyramid:
    """The device frame data FastGrid and GuidedMatcher ask a FramePyramid for, with levels of cv::buildPyramid's sizes ((w + 1) / 2: 322 -> 161 -> 81; FramePyramid
    sizes its buffers w >> l and is for frames whose levels halve exactly) and the oracle's pyramids uploaded into them: this file is about the detector."""

    def __init__(self, ctx, stream, cam, batch):
        import torch
        from scavislam_amd.ctypes_types import level_cams
        self.ctx, self.stream, self.cam, self.batch = ctx, stream, cam, batch
        self.cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"], 3)
        self.w, self.h = [W], [H]
        for _ in range(2):
            self.w.append((self.w[-1] + 1) // 2)
            self.h.append((self.h[-1] + 1) // 2)
        self.stride = [(w + 63) // 64 * 64 for w in self.w]
        with torch.cuda.stream(stream):
            self.pyr = [torch.zeros((batch, self.h[l], self.stride[l]), dtype=torch.uint8, device="cuda") for l in range(3)]
            self.disp = torch.zeros((batch, self.h[0], self.stride[0]), dtype=torch.float32, device="cuda")

    def bstride(self, l):
        return self.h[l] * self.stride[l]

    def upload(self, pyrs, disps=None):
        """pyrs: per stream the three levels (numpy u8)"""
        import torch
        with torch.cuda.stream(self.stream):
            for l in range(3):
                lv = np.stack([p[l] for p in pyrs])
                assert lv.shape == (self.batch, self.h[l], self.w[l]), (l, lv.shape)
                self.pyr[l][:, :, :self.w[l]] = torch.as_tensor(lv).cuda()
            if disps is not None:
                self.disp[:, :, :W] = torch.as_tensor(np.stack(disps).astype(np.float32)).cuda()


def _frame(ctx, stream, cam, pyrs, disps=None):
    fr = _Pyramid(ctx, stream, cam, len(pyrs))
    fr.upload(pyrs, disps)
    return fr


def _busy_image():
    """small dark and bright squares all over: far too many strong corners on every level"""
    rng = np.random.default_rng(3)
    img = np.full((H, W), 20, np.uint8)
    for _ in range(6000):
        x, y, s = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(1, 6))
        img[y:y + s, x:x + s] = int(rng.integers(0, 2)) * 210 + 20
    return img


def _raw_bits(fg, slot, level):
    """the bytes of a stream's corner bitmap of one level, as the matcher reads them (svs_fast_device_view)"""
    d_bits, stride, bstride, colbits = C.c_void_p(), C.c_int32(), C.c_size_t(), C.c_int32()
    fg.ctx.check(fg.ctx.lib.svs_fast_device_view(fg.h, level, C.byref(d_bits), C.byref(stride), C.byref(bstride), C.byref(colbits), None, None))
    fg.ctx.sync()
    raw = np.zeros((fg.frame.h[level], stride.value), np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = hip.hipMemcpy(raw.ctypes.data, d_bits.value + slot * bstride.value, raw.nbytes, 2)      # hipMemcpyDeviceToHost
    assert rc == 0, rc
    return raw


def _with_floor(ctx, floor, fn):
    ctx.set_option("fast_floor", floor)
    try:
        return fn()
    finally:
        ctx.set_option("fast_floor", 1)


_RUN = {}


def _sequence(ctx, stream, floor):
    """the six frames on the device with "fast_floor" = floor: per frame the downloads of every stream and level and the bitmaps' bytes; behind the last frame
    (a frame B) one svs_match of 64 points per stream against the streams' frames A.  Run once per option value."""
    if floor in _RUN:
        return _RUN[floor]
    from scavislam_amd import synth
    from scavislam_amd.frontend import FastGrid, GuidedMatcher
    D = _data()

    def run():
        A = [D["frames"][s][0] for s in range(N_STREAMS)]
        B = [D["frames"][s][1] for s in range(N_STREAMS)]
        pA = [D["pyrs"][s][0] for s in range(N_STREAMS)]
        pB = [D["pyrs"][s][1] for s in range(N_STREAMS)]
        kf = _frame(ctx, stream, D["cam"], pA)
        fr = _frame(ctx, stream, D["cam"], pA, [f[1] for f in A])
        fg = FastGrid(ctx, fr)
        for s in range(N_STREAMS):
            for l in range(3):
                fg.set_thresholds(s, l, _start_thr(s, fg.grids[l].gx * fg.grids[l].gy))
        out = []
        for i in range(N_FRAMES):
            fr.upload(pB if i & 1 else pA, [f[1] for f in (B if i & 1 else A)])
            fg.detectAdaptively(trials=_trials(i))
            out.append(dict(got=[[fg.corners(s, l) for l in range(3)] for s in range(N_STREAMS)],
                            bits=[[_raw_bits(fg, s, l) for l in range(3)] for s in range(N_STREAMS)]))
        # the matcher reads the bitmap of the last detection: stream s matches 64 points anchored in its frame A (keyframe s) into its frame B
        pts = np.stack([synth.candidate_points(np.random.default_rng(7 + s), D["cam"], np.maximum(A[s][1], 0), D["poses"][s][0], N_PTS, kf_index=s)
                        for s in range(N_STREAMS)])
        T_rel = []
        for s in range(N_STREAMS):
            T = synth.pose_mul(D["poses"][s][1], synth.pose_inv(D["poses"][s][0]))
            T[:, 3] += np.array([0.004, -0.003, 0.002])
            T_rel.append(T.reshape(12))
        gm = GuidedMatcher(ctx, fr, fg)
        m = gm.match([(kf.pyr, s, D["poses"][s][0].reshape(12)) for s in range(N_STREAMS)], np.stack(T_rel),
                     np.stack([D["poses"][s][0].reshape(12) for s in range(N_STREAMS)]), pts)
        fg.close()
        return dict(frames=out, match=m.copy())

    _RUN[floor] = _with_floor(ctx, floor, run)
    return _RUN[floor]


def _same(got, ref, where):
    xy, cc, et, ts = got
    xy_ref, cc_ref, et_ref, ts_ref = ref
    assert np.array_equal(cc, cc_ref), (where, "cell counts", cc, cc_ref)
    assert np.array_equal(et, et_ref), (where, "emit thresholds", et, et_ref)
    assert np.array_equal(ts, ts_ref), (where, "threshold state", ts, ts_ref)
    assert np.array_equal(xy, xy_ref), (where, "corner list")


@pytest.mark.parametrize("floor", [1, 0])
def test_sequence_equals_the_oracle(gpu_ctx, floor):
    """six frames A B A B A B, trials 5 then 6: corner lists, counts, emit thresholds and threshold state of every stream, level and frame are the oracle's"""
    ctx, stream = gpu_ctx
    D = _data()
    # the starting thresholds do what they are there for: floors at t_lo, at fast_max - 2 * 4 = 32 (the first frame's five trials) and in between, per cell
    assert D["floors"].min() == 10 and D["floors"].max() == 32 and len(np.unique(D["floors"])) > 6, np.unique(D["floors"])
    run = _sequence(ctx, stream, floor)
    n = 0
    for i in range(N_FRAMES):
        for s in range(N_STREAMS):
            for l in range(3):
                _same(run["frames"][i]["got"][s][l], D["seq"][i][s][l], (floor, i, s, l))
                n += len(D["seq"][i][s][l][0])
    assert n > 2000, n
    print(f"fast_floor {floor}: {N_FRAMES} frames x {N_STREAMS} streams x 3 levels equal the oracle ({n} corners); floors {np.unique(D['floors'])}")


def test_sequence_floor_on_equals_floor_off(gpu_ctx):
    """both option values give each other's downloads, and the same bytes in the corner bitmaps the matcher reads"""
    ctx, stream = gpu_ctx
    on, off = _sequence(ctx, stream, 1), _sequence(ctx, stream, 0)
    n_set = 0
    for i in range(N_FRAMES):
        for s in range(N_STREAMS):
            for l in range(3):
                _same(on["frames"][i]["got"][s][l], off["frames"][i]["got"][s][l], (i, s, l))
                a, b = on["frames"][i]["bits"][s][l], off["frames"][i]["bits"][s][l]
                assert a.tobytes() == b.tobytes(), (i, s, l, "corner bitmap")
                assert int(np.unpackbits(a).sum()) == len(on["frames"][i]["got"][s][l][0]), (i, s, l, "bits set = corners")
                n_set += int(np.unpackbits(a).sum())
    assert n_set > 2000, n_set


def test_matcher_reads_the_same_bitmap(gpu_ctx):
    """one svs_match over 64 points per stream behind the sequence: identical records with the option on and off"""
    ctx, stream = gpu_ctx
    on, off = _sequence(ctx, stream, 1)["match"], _sequence(ctx, stream, 0)["match"]
    assert on.shape == (N_STREAMS, sum(N_PTS))
    assert on.tobytes() == off.tobytes()
    assert all((on[s]["status"] == 0).sum() >= 8 for s in range(N_STREAMS)), [(on[s]["status"] == 0).sum() for s in range(N_STREAMS)]


@pytest.mark.parametrize("floor", [1, 0])
@pytest.mark.parametrize("trials", [0, 1])
def test_single_trial_detections(gpu_ctx, trials, floor):
    """FastGrid::detect (trials 0) and a one-trial detectAdaptively: the floor is the stored threshold itself"""
    import oracle as O
    from scavislam_amd.frontend import FastGrid
    ctx, stream = gpu_ctx
    D = _data()

    def run():
        fr = _frame(ctx, stream, D["cam"], [D["pyrs"][s][0] for s in range(N_STREAMS)])
        fg = FastGrid(ctx, fr, corner_cap=1 << 16)      # (a static detection at 10 finds 8 900 corners on level 0)
        for s in range(N_STREAMS):
            for l in range(3):
                fg.set_thresholds(s, l, _start_thr(s, fg.grids[l].gx * fg.grids[l].gy))
        if trials == 0:
            fg.detect()
        else:
            fg.detectAdaptively(trials=trials)
        got = [[fg.corners(s, l) for l in range(3)] for s in range(N_STREAMS)]
        fg.close()
        return got

    got = _with_floor(ctx, floor, run)
    n = 0
    for s in range(N_STREAMS):
        for l in range(3):
            img = D["pyrs"][s][0][l]
            g = O.fastgrid_for_level(img.shape[1], img.shape[0], l)
            nc = g.gx * g.gy
            g.thr[:nc] = list(_start_thr(s, nc))
            xy, cc, et, ts = got[s][l]
            if trials == 0:
                xy_ref, cc_ref = O.fastgrid_detect(g, img)
                assert np.array_equal(ts, _start_thr(s, nc)), (s, l, "detect leaves the thresholds alone")
            else:
                xy_ref, cc_ref, et_ref = O.fastgrid_detect_adaptively(g, img, trials)
                assert np.array_equal(et, et_ref) and np.array_equal(ts, np.array(g.thr[:nc])), (s, l, et, et_ref, ts)
            assert np.array_equal(cc, cc_ref), (s, l, cc, cc_ref)
            assert np.array_equal(xy, xy_ref), (s, l)
            n += len(xy_ref)
    assert n > 500, n


@pytest.mark.parametrize("floor", [1, 0])
@pytest.mark.parametrize("trials", [0, 6])
def test_thresholds_moved_from_outside(gpu_ctx, trials, floor):
    """a frame of small high-contrast squares leaves every cell's threshold at fast_max = 40; svs_fast_set_thresholds then puts 10 there and the next detection (static, or six trials)
    must find what the oracle finds from 10: the floor comes from the thresholds in memory when the kernel runs, not from anything the last frame left behind"""
    import oracle as O
    from scavislam_amd.frontend import FastGrid
    ctx, stream = gpu_ctx
    D = _data()
    busy = _busy_image()

    def run():
        fr = _frame(ctx, stream, D["cam"], [O.build_pyramid(busy)])
        fg = FastGrid(ctx, fr, corner_cap=1 << 16)
        for l in range(3):
            fg.set_thresholds(0, l, np.full(fg.grids[l].gx * fg.grids[l].gy, 40, np.int32))
        fg.detectAdaptively(trials=6)
        high = [fg.corners(0, l)[3] for l in range(3)]
        for l in range(3):
            fg.set_thresholds(0, l, np.full(fg.grids[l].gx * fg.grids[l].gy, 10, np.int32))
        fr.upload([D["pyrs"][0][0]])
        if trials == 0:
            fg.detect()
        else:
            fg.detectAdaptively(trials=trials)
        got = [fg.corners(0, l) for l in range(3)]
        fg.close()
        return high, got

    high, got = _with_floor(ctx, floor, run)
    n_low = 0
    for l in range(3):
        assert np.all(high[l] == 40), (l, high[l])
        p = D["pyrs"][0][0][l]
        g = O.fastgrid_for_level(p.shape[1], p.shape[0], l)
        nc = g.gx * g.gy
        g.thr[:nc] = [10] * nc
        xy, cc, et, ts = got[l]
        if trials == 0:
            xy_ref, cc_ref = O.fastgrid_detect(g, p)
        else:
            xy_ref, cc_ref, et_ref = O.fastgrid_detect_adaptively(g, p, trials)
            assert np.array_equal(et, et_ref) and np.array_equal(ts, np.array(g.thr[:nc])), (l, et, et_ref, ts)
            n_low += int((et_ref < 30).sum())
        assert np.array_equal(cc, cc_ref), (l, cc, cc_ref)
        assert np.array_equal(xy, xy_ref), l
        if trials == 0:
            n_low += int((et < 30).sum()) * (len(xy_ref) > 0)      # (a static detection emits at the stored threshold: 10)
    assert n_low > 0, "the detection must ask for scores below the floor the frame before had (30)"
