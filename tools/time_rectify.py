"""rectifier (svs_rectify_frames: BGR left + gray right through the first / second lens set) on B raw 640x480 pairs, alternated in one process with the
pyramid step (svs_pyr_down_u8) on the same frames: ms per batch and bytes/s on algorithmic bytes, device events over >= 0.2 s of work each.
usage: python tools/time_rectify.py [B] [mode] [name=value ...]
  mode "all" (default)   "kernels", then "frontend"
  mode "kernels"         the table above + depth to disparity
  mode "frontend"        a processFrames step of B streams with and without the rectifier in front
  mode "profile"         a few calls of each kernel only: run it under `rocprofv3 --kernel-trace --stats` or, in a run of its own, `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE`
                         (tools/rocpd_summary.py / tools/pmc_any.py read the databases)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scavislam_amd import capi, synth
from scavislam_amd.frontend import FrameGrabber, StereoFrontend

opts = [a for a in sys.argv[1:] if "=" in a]      # context options, e.g. xcd_swizzle=0
args = [a for a in sys.argv[1:] if "=" not in a]
B = int(args[0]) if len(args) > 0 else 512
MODE = args[1] if len(args) > 1 else "all"
LENS = {"first": ((-0.28, 0.07, 1e-3, -5e-4, 0.01), (0.004, -0.011, 0.007)), "second": ((-0.25, 0.05, -8e-4, 6e-4, 0.0), (-0.003, 0.009, -0.02))}
W, H = 640, 480
CAM = dict(f=530.0, cx=319.5, cy=239.5, b=0.075, w=W, h=H)

ctx, stream = capi.torch_context(0)
for a in opts:
    ctx.set_option(a.split("=")[0], int(a.split("=")[1]))
grab = FrameGrabber(ctx, CAM, max_batch=B)
grab.intializeRectifier(LENS["first"][1], LENS["first"][0], LENS["second"][1], LENS["second"][0])
with torch.cuda.stream(stream):
    raw_l = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")      # distinct frames: nothing for a cache to share between streams
    raw_r = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda")
    out_l, out_r = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda"), torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    lvl1 = torch.zeros((B, H // 2, W // 2), dtype=torch.uint8, device="cuda")
    depth = torch.randint(1, 32767, (B, H, W), dtype=torch.int16, device="cuda")
    disp = torch.zeros((B, H, W), dtype=torch.float32, device="cuda")
MAP_BYTES = 2 * W * H * 6                                    # both sides' maps as given (int16 x 2 + uint16), read once per launch whatever the batch
RECT_BYTES = B * (3 * W * H + W * H + 2 * W * H) + MAP_BYTES      # BGR left + gray right in, two gray images out
PYR_BYTES = B * (W * H + (W // 2) * (H // 2))
DEPTH_BYTES = B * W * H * 6


def rect():
    grab.rectifyFrame(raw_l, out_l, raw_r, out_r)


def pyr():
    ctx.call("svs_pyr_down_u8", out_l.data_ptr(), W, H, W, H * W, lvl1.data_ptr(), W // 2, (H // 2) * (W // 2), B)


def d2d():
    grab.depthToDisp(depth, disp)


def block_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


if MODE == "profile":
    for _ in range(5):
        rect(); pyr(); d2d()
    ctx.sync()
    print("profile: 5 calls of each")
    sys.exit(0)



def kernels():
    for fn in (rect, pyr, d2d):                              # warm-up: code objects, clocks
        block_ms(fn, 10)
    N = 20
    fns = dict(rectify=(rect, RECT_BYTES), pyr_down=(pyr, PYR_BYTES), depth_to_disp=(d2d, DEPTH_BYTES))
    one = {k: block_ms(f, N) for k, (f, _) in fns.items()}
    blocks = max(10, int(np.ceil(250.0 / min(one.values()))))    # every kernel gets >= 0.25 s of device time
    ms = {k: [] for k in fns}
    for _ in range(blocks):                                      # alternated: rectifier, pyramid step, depth, rectifier, ...
        for k, (f, _) in fns.items():
            ms[k].append(block_ms(f, N) / N)
    print(f"B = {B}, {W}x{H}, {blocks} alternated blocks of {N} calls")
    for k, (f, nbytes) in fns.items():
        v = np.array(ms[k])
        print("%-14s %.4f ms per %d (min %.4f, max %.4f; %.2f s timed)  %.1f MB algorithmic  %.3f TB/s" % (k, np.median(v), B, v.min(), v.max(), v.sum() * N / 1e3, nbytes / 1e6,
                                                                                                           nbytes / (np.median(v) * 1e-3) / 1e12))


if MODE in ("all", "kernels"):
    kernels()
if MODE == "kernels":
    sys.exit(0)
del raw_l, raw_r, out_l, out_r, lvl1, depth, disp
torch.cuda.empty_cache()

# ---- a processFrames step of B streams (frames resident in HBM, ping-pong A B A B like bench.py's headline, its own small set of scenes), plain against
# ---- "raw BGR + 16-bit depth through rectifyFrame + depthToDisp into the input view, then processFrames without frames"
sc = synth.Scene(2011)
traj = synth.trajectory(12)
cam = synth.CAM_DEFAULT
NP = 8
g2 = FrameGrabber(ctx, cam, max_batch=B)
g2.intializeRectifier(LENS["first"][1], LENS["first"][0])
fr = [[sc.render(cam, traj[4 + p + k], seed=100 * k + p) for k in range(2)] for p in range(NP)]
d16 = [[np.where(f[1] > 0.5, np.clip(np.rint(5000.0 * cam["f"] * cam["b"] / np.maximum(f[1], 0.5)), 1, 65535), 65535).astype(np.uint16) for f in pr] for pr in fr]
pair = [b % NP for b in range(B)]
with torch.cuda.stream(stream):
    rawL = [torch.as_tensor(np.stack([np.repeat(fr[p][k][0][:, :, None], 3, axis=2) for p in pair])).cuda() for k in range(2)]
    rawD = [torch.as_tensor(np.stack([d16[p][k] for p in pair]).view(np.int16)).cuda() for k in range(2)]
    rectL = [torch.zeros((B, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    rectD = [torch.zeros((B, H, W), dtype=torch.float32, device="cuda") for _ in range(2)]
for k in range(2):
    g2.rectifyFrame(rawL[k], rectL[k])
    g2.depthToDisp(rawD[k], rectD[k])
ctx.sync()
ready = torch.cuda.Event()                                   # svs_frames_dev::ready_event of the plain arm: its frames are complete from here on (bench.py does the same)
with torch.cuda.stream(stream):
    ready.record(stream)
T_act = np.stack([traj[4 + p].reshape(12) for p in pair])
I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
T_AB = [synth.pose_mul(traj[5 + p], synth.pose_inv(traj[4 + p])).reshape(12) for p in range(NP)]
T_pose = [np.tile(I34, (B, 1)), np.stack([T_AB[p] for p in pair])]
pts = [synth.candidate_points(np.random.default_rng(7 + p), cam, np.maximum(fr[p][0][1], 0), traj[4 + p], (1200, 600, 200)) for p in range(NP)]


def frontend():
    fe = StereoFrontend(ctx, cam, max_points=2000, max_keyframes=1, n_streams=B)
    fe.processFirstFrames(left=rectL[0], disp=rectD[0])
    fe.keepKeyframes(0, T_act)
    fe.setCandidateListsAll([pts[p] for p in pair], [[len(pts[p]) // 2, len(pts[p])] for p in pair])
    return fe


def steps(fe, n, k0, raw):
    for k in range(k0, k0 + n):
        f = k & 1
        if raw:
            (pl, sl, bl), _, (pd, sd, bd) = fe.inputView()
            g2.rectifyFrame(rawL[f], (pl, sl, bl))
            g2.depthToDisp(rawD[f], (pd, sd, bd))
            fe.processFrames(T_pose[1 - f], T_act)
        else:
            fe.processFrames(T_pose[1 - f], T_act, left=rectL[f], disp=rectD[f], ready_event=ready)


res = {}
fes = {False: frontend(), True: frontend()}
for raw in (False, True):
    steps(fes[raw], 3, 1, raw)
ctx.sync()
for rep in range(5):                                         # alternated arms, 10 steps a block
    for raw in (False, True):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            steps(fes[raw], 10, 4, raw)
            e1.record(stream)
        e1.synchronize()
        res.setdefault(raw, []).append(e0.elapsed_time(e1) / 10)
Ta, Tb = fes[False].poses()[0], fes[True].poses()[0]
print("processFrames step, %d streams: %.3f ms rectified frames by pointer; %.3f ms raw BGR + depth through rectifyFrame + depthToDisp first (blocks: %s | %s); poses identical: %s"
      % (B, np.median(res[False]), np.median(res[True]), " ".join("%.3f" % v for v in res[False]), " ".join("%.3f" % v for v in res[True]), bool(np.array_equal(Ta, Tb))))
for fe in fes.values():
    fe.close()
