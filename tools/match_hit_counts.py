#!/usr/bin/env python3
"""How many corners the guided matcher's search windows hold on the benchmark's frames (no GPU: the oracle's FAST on the benchmark's renders).

match_kernel3 scores a point's hits 16 at a time: the first trip of its stage (5) takes hits 1..16, a later trip each further 16.  This prints, for a few of
bench.py's frame pairs, the share of candidate points whose (2R+1)^2 window holds more than 16 and more than 32 corners -- how much of the batch the later trips
see at all.  The frames, motions and candidate lists are bench.py's (same scene, seeds and quota per level); FAST runs as the front end runs it on a stream's
first two frames (5 trials on frame A, 6 on frame B, thresholds carried over), the window is centred on the projection at the true pose of frame B (the tracker's
pose lies within a fraction of a pixel of it).  A point counts if the benchmark's matcher would search it: predicted position finite, depth ratio below 3.

    python tools/match_hit_counts.py [--pairs 4] [--radius 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--points", type=int, default=2000)
    a = ap.parse_args()
    import oracle as O
    from scavislam_amd import synth
    from scavislam_amd.ctypes_types import level_cams
    cam = synth.CAM_DEFAULT
    cams = level_cams(cam["f"], cam["cx"], cam["cy"], cam["b"], cam["w"], cam["h"])
    scene, traj = synth.Scene(2011), synth.trajectory(8)
    mrng = np.random.default_rng(77)
    quota = (int(a.points * 0.6), int(a.points * 0.3), a.points - int(a.points * 0.6) - int(a.points * 0.3))
    tot = np.zeros(3, np.int64)
    hist_all = []
    for p in range(a.pairs):
        T_p = traj[4 + p % 4]
        step, yaw = mrng.uniform(0.02, 0.08), np.deg2rad(mrng.uniform(0.05, 0.5)) * mrng.choice([-1, 1])
        R_rel = synth.so3_exp(np.array([mrng.normal(0, 0.0005), yaw, mrng.normal(0, 0.0005)]))
        T_rel = synth.pose(R_rel, np.array([mrng.normal(0, 0.003), mrng.normal(0, 0.002), -step]))
        (img_a, disp_a), (img_b, _) = scene.render(cam, T_p, seed=100 + p), scene.render(cam, synth.pose_mul(T_rel, T_p), seed=200 + p)
        pa, pb = O.build_pyramid(img_a), O.build_pyramid(img_b)
        rng = np.random.default_rng(2011 + p)
        corners_a, corners_b = [], []
        for l in range(3):
            g = O.fastgrid_for_level(pa[l].shape[1], pa[l].shape[0], l)
            corners_a.append(O.fastgrid_detect_adaptively(g, pa[l], 5)[0].astype(np.int64))
            corners_b.append(O.fastgrid_detect_adaptively(g, pb[l], 6)[0].astype(np.int64))
        per_level = []
        for l in range(3):                                      # bench.py, candidates_from_corners
            xy = corners_a[l]
            d = disp_a[xy[:, 1] << l, xy[:, 0] << l]
            keep = np.nonzero(d > 0.5)[0]
            per_level.append((xy[keep], d[keep].astype(np.float64), rng.permutation(len(keep))))
        take = [min(quota[l], len(per_level[l][2])) for l in range(3)]
        take[0] = min(len(per_level[0][2]), take[0] + (a.points - sum(take)))
        counts = []
        for l, ((xy, d, perm), n) in enumerate(zip(per_level, take)):
            sel = perm[:n]
            s = float(1 << l)
            u0, v0 = xy[sel, 0] * s, xy[sel, 1] * s
            z = cam["f"] * cam["b"] / d[sel]
            X = np.stack([(u0 - cam["cx"]) / cam["f"] * z, (v0 - cam["cy"]) / cam["f"] * z, z], 1)
            Q = X @ T_rel[:, :3].T + T_rel[:, 3]
            ok = (Q[:, 2] > 0) & (z / Q[:, 2] < 3) & (Q[:, 2] / z < 3)
            ui = (cams[l].f * Q[:, 0] / Q[:, 2] + cams[l].cx).astype(np.int64)
            vi = (cams[l].f * Q[:, 1] / Q[:, 2] + cams[l].cy).astype(np.int64)
            wl, hl = pb[l].shape[1], pb[l].shape[0]
            img = np.zeros((hl, wl), np.int64)
            cb = corners_b[l]
            cb = cb[(cb[:, 0] >= 6) & (cb[:, 0] < wl - 6) & (cb[:, 1] >= 6) & (cb[:, 1] < hl - 6)]
            img[cb[:, 1], cb[:, 0]] = 1
            ii = np.pad(img.cumsum(0).cumsum(1), ((1, 0), (1, 0)))
            x0, x1 = np.clip(ui - a.radius, 0, wl), np.clip(ui + a.radius + 1, 0, wl)
            y0, y1 = np.clip(vi - a.radius, 0, hl), np.clip(vi + a.radius + 1, 0, hl)
            c = ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]
            counts.append(c[ok])
        c = np.concatenate(counts)
        hist_all.append(c)
        tot += (len(c), int((c > 16).sum()), int((c > 32).sum()))
        print("pair %d: %d searched points, corners per level on frame B %s; hits per window: median %d, 90 %% %d, max %d; more than 16: %.2f %%, more than 32: %.2f %%"
              % (p, len(c), [len(x) for x in corners_b], np.median(c), np.percentile(c, 90), c.max(), 100.0 * (c > 16).mean(), 100.0 * (c > 32).mean()))
    print("all: %d points, more than 16 hits: %.2f %%, more than 32: %.2f %%" % (tot[0], 100.0 * tot[1] / tot[0], 100.0 * tot[2] / tot[0]))


if __name__ == "__main__":
    main()
