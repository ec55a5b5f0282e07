"""The tail of the refinement kernel (motion.hip: motion_only_fused_kernel<true> -- processMatchedPoints' gate and the three dense clouds behind a stream's LM loop,
with their loads requested ahead and their quotients through one reciprocal) against the separate launches ("fe_fuse_tail" 0: svs_motion_only, gate_matched_kernel,
pointcloud_cpu_sem_levels_kernel): refined pose, point statistics, gated records and all three clouds of every stream must be the same bytes; the clouds of both
schedules, and those of the stand-alone per-level kernel, must be the oracle's at the refined pose.

128 streams (the smallest batch that takes the fused path on 256 CUs: 2 B >= n_cu) at 160 x 128, the smallest frame of tests/test_gpu_frame_sizes.py's grid:
  * level 2 has 10 x 8 = 80 samples, fewer than the workgroup's 256 lanes; level 1 has 320 (two trips, the second a quarter full); level 0 has 1 280 = five trips,
    no multiple of the prefetch depth (4) -- the ring of requested disparities runs past the end of every level;
  * the disparity images are device views with padded rows (16 floats, NaN) and extra rows between streams;
  * big_batch_common's streams: candidate lists of 0, 1, 3, 1 024 and odd lengths (no multiple of 256 among them but 0 and 1 024), a different number of new-point
    records per stream, flat streams (no corner, no match: the gate sees no accepted record), streams without any valid disparity;
  * on top, every fifth stream gets blobs of disparity 0 and -1 punched into its tracked frames."""
import numpy as np
import pytest

import big_batch_common as BB
from test_gpu_big_batch import _outputs
from test_gpu_frame_sizes import cam_of

pytestmark = pytest.mark.gpu

W, H = 160, 128
B = 128
N_FRAMES = 2
PREFETCH = 4          # motion.hip: CLOUD_PF


def _blobs(disp, seed):
    """rectangles of disparity 0 and -1 (and one row and one column of them across the whole frame)"""
    rng = np.random.default_rng(seed)
    d = disp.copy()
    for k in range(6):
        x, y = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8))
        d[y:y + int(rng.integers(3, 24)), x:x + int(rng.integers(3, 24))] = (0.0, -1.0)[k % 2]
    d[int(rng.integers(0, H)) // 4 * 4, :] = 0.0
    d[:, int(rng.integers(0, W)) // 4 * 4] = -1.0
    return d


_S = {}


def _streams():
    if "S" not in _S:
        cam, S = BB.make_streams(B, seed=53, cam=cam_of(W, H))
        for b, s in enumerate(S):
            if b % 5 == 2:
                s["frames"] = [(img, _blobs(disp, 100 * b + k)) for k, (img, disp) in enumerate(s["frames"])]
        _S.update(cam=cam, S=S)
    return _S["cam"], _S["S"]


def _padded(stream, arrays, dtype, extra, fill):
    """[B][h][w] as a view into a device buffer with rows `extra` elements longer and 3 extra rows per stream, padding `fill`"""
    import torch
    a = np.stack(arrays).astype(dtype, copy=False)
    with torch.cuda.stream(stream):
        buf = torch.full((len(arrays), H + 3, W + extra), fill, dtype=torch.uint8 if dtype == np.uint8 else torch.float32, device="cuda")
        buf[:, :H, :W] = torch.as_tensor(a).cuda()
    stream.synchronize()
    return buf[:, :H, :W]


def _run(ctx, stream, cam, S, fuse):
    """two keyframes, the first frame, N_FRAMES tracked frames through svs_frontend_process_frames; per tracked frame: every stream's outputs as bytes, the
    refined poses and the clouds as arrays"""
    from scavislam_amd import capi
    from scavislam_amd.frontend import StereoFrontend
    ctx.set_option("fe_fuse_tail", fuse)
    try:
        fe = StereoFrontend(ctx, cam, max_points=BB.MAX_POINTS, max_keyframes=3, params=capi.FrontendParams.reference(), n_streams=len(S))
        up = lambda frames: dict(left=_padded(stream, [f[0] for f in frames], np.uint8, 64, 255), disp=_padded(stream, [f[1] for f in frames], np.float32, 16, float("nan")))
        for j in range(2):
            fe.processFirstFrames(**up([s["kf"][j] for s in S]))
            fe.keepKeyframes(j, np.stack([s["T_kf"][j].reshape(12) for s in S]))
        fe.processFirstFrames(**up([s["first"] for s in S]))
        fe.recomputeCloud(np.stack([s["T_first"].reshape(12) for s in S]))
        fe.setCandidateListsAll([s["pts"] for s in S], [s["group_end"] for s in S])
        T_act = np.stack([s["T_act"].reshape(12) for s in S])
        out = []
        for k in range(N_FRAMES):
            fe.processFrames(np.stack([s["T_guess"][k].reshape(12) for s in S]), T_act, **up([s["frames"][k] for s in S]))
            T, ok = fe.poses()
            o = [_outputs(fe, b) for b in range(len(S))]
            res = [fe.results(b) for b in range(len(S))]
            clouds = [[fe.cloud_host(l, stream=b) for l in range(3)] for b in range(len(S))]
            out.append(dict(T=T.copy(), ok=ok.copy(), bytes=o, res=res, clouds=clouds))
        fe.close()
        return out
    finally:
        ctx.set_option("fe_fuse_tail", 1)


def test_fused_tail_equals_separate_launches_and_the_oracle(gpu_ctx):
    import oracle as O
    from scavislam_amd.ctypes_types import level_cams
    from scavislam_amd.frontend import DenseTracker, FramePyramid
    ctx, stream = gpu_ctx
    assert 2 * B >= BB.n_cu(), "the batch is too small for the fused path on this device"
    cam, S = _streams()
    n_px = [(W >> l) // 4 * ((H >> l) // 4) for l in range(3)]
    assert n_px[2] < 256 and any(-(-n // 256) % PREFETCH for n in n_px), n_px
    lens = [len(s["pts"]) for s in S]
    assert {0, 1, 3, BB.MAX_POINTS} <= set(lens) and sum(n % 256 != 0 for n in lens) > B // 2
    assert len({int(s["group_end"][0]) for s in S}) > B // 4, "the streams' numbers of new-point records"

    fused = _run(ctx, stream, cam, S, 1)
    apart = _run(ctx, stream, cam, S, 0)
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    n_gated = n_none = n_samples_off = 0
    for k in range(N_FRAMES):
        f, a = fused[k], apart[k]
        assert f["T"].tobytes() == a["T"].tobytes() and f["ok"].tobytes() == a["ok"].tobytes(), (k, "poses")
        for b in range(B):
            for kind in f["bytes"][b]:
                assert f["bytes"][b][kind] == a["bytes"][b][kind], (k, b, S[b]["spec"]["kind"], kind)
            res, m, g = f["res"][b]
            n_ok = int((m["status"] == 0).sum())
            assert res.point_stats.num_obs == n_ok, (k, b)
            n_gated += int(g["accepted"].sum())
            n_none += n_ok > 0 and int(g["accepted"].sum()) == 0 or n_ok == 0 and len(m) > 0
            # the clouds of both schedules: the oracle's at the refined pose, bit for bit
            disp = S[b]["frames"][k][1]
            for l in range(3):
                ref = O.pointcloud_cpu(disp, cams[l], l, f["T"][b])
                assert np.array_equal(f["clouds"][b][l].view(np.uint32), ref.view(np.uint32)), (k, b, "fused cloud against the oracle", l)
                n_samples_off += int((ref[..., 3] < 0).sum())
    assert n_gated > 100 and n_none > 0 and n_samples_off > 1000, (n_gated, n_none, n_samples_off)

    # the stand-alone per-level kernel (svs_pointcloud_cpu_sem) on a few of the streams, at the pose the front end refined
    pick = [b for b in range(B) if b % 5 == 2][:4] + [b for b in range(B) if S[b]["spec"]["kind"] == "no_depth"][:1] + [0, 1]
    k = N_FRAMES - 1
    fr = FramePyramid(ctx, stream, cam, batch=len(pick), with_float=False)
    fr.upload(np.stack([S[b]["frames"][k][0] for b in pick]), np.stack([S[b]["frames"][k][1] for b in pick]))
    dt = DenseTracker(ctx, fr)
    dt.computeDensePointCloudCpu(np.stack([fused[k]["T"][b].reshape(12) for b in pick]))
    ctx.sync()
    for j, b in enumerate(pick):
        for l in range(3):
            got = dt.ref_dense_points[l][j].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), fused[k]["clouds"][b][l].view(np.uint32)), (b, "stand-alone cloud kernel", l)
    print(f"{W} x {H}, {B} streams x {N_FRAMES} frames: fused tail = separate launches in every output; clouds = the oracle's ({n_samples_off} samples without "
          f"disparity); {n_gated} gated points, {n_none} stream-frames whose gate accepted nothing; list lengths {min(lens)} .. {max(lens)}")
