"""Distinct streams for the big-batch tests (tests/test_gpu_big_batch.py).  A big batch (more streams than CUs) runs the flat tracker kernel, the balanced grid
order, the continuation launch for parked streams and the side-stream FAST: machinery that only a batch of that size uses.  Streams dealt round-robin from a
few inputs cannot show a result written to, or read from, the wrong slot.  Every stream made here differs from every other in what reaches a kernel: its place
in the 200-frame there-and-back sequence (frames are rendered once and shared), its motion guess, its candidate list (length and keyframe slots) -- plus a
few hostile but legal streams (flat image, no valid disparity, saturated image).  Everything is seeded: two calls give identical inputs."""
import numpy as np

N_OFFSETS = 16            # places in the sequence; a stream's frames are those at offset o .. o + N_TRACKED (+ its two keyframes in front)
N_TRACKED = 3             # tracked frames per stream
FIRST = 2                 # the first offset (two keyframes in front of it)
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
HOSTILE = ("flat", "no_depth", "saturated")
MAX_POINTS = 1024         # the front end's max_points in the tests
ACTKEY, NEIGHBOUR = 1, 0  # keyframe slots: the active keyframe (the frame in front of the first one) and its one neighbour


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_FRAMES = {}


def seq_frames(cam=None):
    """(image, disparity) of the frames of the default sequence the streams use, rendered once per process and camera; + the trajectory.  cam: another
    camera (dict f, cx, cy, b, w, h) on the same trajectory, frames rendered the way seq_common.frames renders them; None: the default camera"""
    key = "default" if cam is None else tuple(sorted(cam.items()))
    if key not in _FRAMES:
        import seq_common
        from scavislam_amd import synth
        n = FIRST + N_OFFSETS + N_TRACKED
        traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)[:n]
        if cam is None:
            f = list(seq_common.frames("default", n))
        else:
            sc = synth.Scene(2011)
            f = [sc.render(cam, traj[i], seed=i) for i in range(n)]
        _FRAMES[key] = (f, traj)
    return _FRAMES[key]


def hostile_frame(kind, img):
    """flat: +-1 grey level of texture around 128 (no FAST corner anywhere; a perfectly constant image would leave the tracker a singular system);
    saturated: the frame four times as bright, clipped (most pixels 255); no_depth: every disparity <= 0 (the tracker leaves the pose as it came in)"""
    if kind == "flat":
        return (127 + (img.astype(np.int32) * 3 // 256)).astype(np.uint8), None
    if kind == "saturated":
        return np.minimum(img.astype(np.int32) * 4, 255).astype(np.uint8), None
    return None, np.full(img.shape, -1.0, np.float32)


def motion_error(rng, size):
    """a small rotation + translation of magnitude `size` (0 .. 1) on top of the true relative pose"""
    from scavislam_amd import synth
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    dirn = rng.normal(size=3); dirn /= np.linalg.norm(dirn)
    return synth.pose(synth.so3_exp(axis * np.deg2rad(1.2) * size), dirn * 0.06 * size)


def stream_spec(b, seed=0):
    """the inputs of stream b (a pure function of (b, seed)): offset, motion error size per tracked frame, candidate counts per level, hostile kind"""
    rng = np.random.default_rng([seed, b])
    o = FIRST + int(rng.integers(0, N_OFFSETS))
    # log-spread sizes: most streams converge in a few trials, the large ones take more than ten on level 0 and park
    sizes = [float(10 ** rng.uniform(-3, 0)) for _ in range(N_TRACKED)]
    kind = HOSTILE[b % 29 // 9] if b % 29 in (4, 13, 22) else None
    counts = [tuple(int(x) for x in rng.integers(0, (201, 101, 41))) for _ in range(2)]      # candidates per level, one draw per keyframe
    n = sum(map(sum, counts))
    length = (0, 1, 3)[b // 23 % 3] if b % 23 == 5 else (MAX_POINTS if b % 41 == 7 else int(rng.integers(n // 2, n + 1)))      # the list: trimmed / padded to this
    return dict(o=o, sizes=sizes, kind=kind, counts=counts, length=length, seed=int(rng.integers(1 << 30)))


def make_streams(B, seed=0, specs=None, cam=None):
    """B pairwise distinct streams (or the given specs).  Per stream: the two keyframes' images / disparities / poses (slot 1 = the active keyframe), the first
    frame and its pose relative to the active keyframe, N_TRACKED frames to track (image, disparity) with their motion guess T_cur_from_actkey (and, for the
    first one, the same guess relative to the first frame: the bare tracker's start pose), T_actkey_from_w, the candidate list in matchAndTrack's order with its
    group ends (active keyframe's new points | the neighbour's | the neighbourhood) and each record's list (the reference's list_of).  cam: see seq_frames."""
    from scavislam_amd import synth
    F, traj = seq_frames(cam)
    cam = synth.CAM_DEFAULT if cam is None else cam
    own = specs is None
    specs = [stream_spec(b, seed) for b in range(B)] if own else specs
    out = []
    for b, sp in enumerate(specs):
        o, rng = sp["o"], np.random.default_rng(sp["seed"])
        kfs = [o - 2, o - 1]
        pts = np.concatenate([synth.candidate_points(rng, cam, np.maximum(F[k][1], 0), traj[k], sp["counts"][j], kf_index=j) for j, k in enumerate(kfs)])
        rng.shuffle(pts)
        n = sp["length"]
        pts = np.concatenate([pts] * (n // max(len(pts), 1) + 1))[:n] if len(pts) else pts[:0]
        pts["point_id"] = np.arange(len(pts))
        g = sorted(int(x) for x in rng.integers(0, n + 1, size=2))
        group_end = np.array([g[0], g[1], n], np.int32)
        list_of = np.concatenate([np.full(g[0], ACTKEY), np.full(g[1] - g[0], NEIGHBOUR), np.full(n - g[1], -1)]).astype(np.int32)
        T_act = traj[o - 1]
        frames, guesses = [], []
        for k in range(1, N_TRACKED + 1):
            img, disp = F[o + k]
            if sp["kind"] is not None:
                hi, hd = hostile_frame(sp["kind"], img)
                img = hi if hi is not None else img
                disp = hd if hd is not None else disp
            frames.append((img, disp))
            err = motion_error(rng, sp["sizes"][k - 1])
            guesses.append(synth.pose_mul(err, synth.pose_mul(traj[o + k], synth.pose_inv(T_act))))
            if k == 1:
                guess_from_first = synth.pose_mul(err, synth.pose_mul(traj[o + 1], synth.pose_inv(traj[o])))
        first = F[o]
        if sp["kind"] == "no_depth":
            first = (first[0], np.full_like(first[1], -1.0))
        out.append(dict(spec=sp, kf=[F[k] for k in kfs], T_kf=[traj[k] for k in kfs], first=first, T_first=synth.pose_mul(traj[o], synth.pose_inv(T_act)),
                        T_act=T_act, frames=frames, T_guess=guesses, T_guess_first=guess_from_first, pts=pts, group_end=group_end, list_of=list_of))
    if own and B >= 100:
        lens = [len(s["pts"]) for s in out]
        assert {0, 1, MAX_POINTS} <= set(lens) and sum(n % 2 for n in lens) >= B // 4, "candidate list lengths 0, 1, odd and max_points must all occur"
    return cam, out
