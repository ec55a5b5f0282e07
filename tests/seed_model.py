"""NumPy restatement of new-point seeding: StereoFrontend::addNewPoints / addMorePoints / addMorePointsToOtherFrame (stereo_frontend.cpp:682-823) given a visiting
order, and the generated order of include/scavislam_hip.h.  The yardstick of scavislam_amd/csrc/seed.hip.

It follows the reference line by line and takes no shortcut: the point tree is an explicit list of (x, y) and the clearance test is cv::Rect_<double>::contains
as quadtree.h:713-754 applies it.  tests/test_seed_cpu.py holds it against the reference's compiled quadtree and against the points the reference itself seeded."""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def thirds(n):
    """float third = 1./3.; int third_width = cam.width()*third; int twothird_width = cam.width()*2*third;  (stereo_frontend.cpp:738-742): float products"""
    third = np.float32(1.0 / 3.0)
    return int(np.float32(n) * third), int(np.float32(np.float32(n * 2) * third))


def window_contains(x, y, R, px, py):
    """Rectangle win(x - R, y - R, 2 R + 1, 2 R + 1); win.contains(p): win.x <= p.x < win.x + win.width and the same in y (cv::Rect_::contains)"""
    wx, wy, ww = float(x - R), float(y - R), float(2 * R + 1)
    return wx <= px < wx + ww and wy <= py < wy + ww


def is_window_empty(points, x, y, R):
    return not any(window_contains(x, y, R, px, py) for px, py in points)


def level_size(W, H, l):
    return (W + (1 << l) - 1) >> l, (H + (1 << l) - 1) >> l


def generated_order(seed, level, cell_counts):
    """visiting order (list indices) of a level whose corner list holds cell_counts[c] corners of cell c, cells back to back"""
    seed = int(seed) & M64
    keys, start = [], 0
    for c, nc in enumerate(int(v) for v in cell_counts):
        a = sorted((splitmix64(seed ^ ((1 << 62) | (level << 32) | i)), i) for i in range(start, start + nc))
        for j, (_, i) in enumerate(a):
            keys.append((j, splitmix64(seed ^ ((2 << 62) | (level << 48) | (j << 16) | c)), c, i))
        start += nc
    return np.array([k[3] for k in sorted(keys)], np.int32).reshape(-1)


def unmap_uvu(cam, u0, u1, u2):
    """stereo_camera.cpp:46-52 with LinearCamera::unmap(uv) = (uv - c) / f"""
    sd = (u0 - u2) / cam["b"]
    z = cam["f"] / sd
    return ((u0 - cam["cx"]) / cam["f"]) * z, ((u1 - cam["cy"]) / cam["f"]) * z, z


def seed_points(corners, orders, disp, cam, tree_xy, tree_level, add_flags, n0, T=None, kf_index=0, first_point_id=0, clearance=2, num_max_points=300, n_levels=3):
    """corners[l]: (n, 2) ints of level l; orders[l]: indices into it; disp: (H, W) float32 (any row stride); cam: dict f, cx, cy, b, w, h (level 0);
    tree_xy (m, 2) doubles at their level, tree_level (m,); add_flags (9,) [i * 3 + j]; n0 (3,).
    Returns (records in the reference's list order: dict of arrays xyz_anchor, anchor_obs_pyr, anchor_level, kf_index, point_id; n_new (3,); trace) where
    trace[l] = list of (list index, reason) with reason in 'disp', 'border', 'flag', 'window', 'taken' for every corner visited"""
    W, H, R = int(cam["w"]), int(cam["h"]), int(clearance)
    T = np.hstack([np.eye(3), np.zeros((3, 1))]) if T is None else np.asarray(T, np.float64).reshape(3, 4)
    third_w, twothird_w = thirds(W)
    third_h, twothird_h = thirds(H)
    taken, n_new, trace = [], [0, 0, 0], [[], [], []]
    tree_xy = np.asarray(tree_xy, np.float64).reshape(-1, 2)
    tree_level = np.asarray(tree_level, np.int64).reshape(-1)
    for l in range(n_levels):
        LW, LH = level_size(W, H, l)
        # a tree point whose floor lies outside the level image is ignored (the reference asserts)
        tree = [(float(x), float(y)) for (x, y), tl in zip(tree_xy, tree_level) if tl == l and 0 <= np.floor(x) < LW and 0 <= np.floor(y) < LH]
        n, cap = int(n0[l]), int(num_max_points) >> l
        xy = np.asarray(corners[l]).reshape(-1, 2)
        for idx in (int(v) for v in orders[l]):
            if not 0 <= idx < len(xy):
                continue
            x, y = int(xy[idx, 0]), int(xy[idx, 1])
            ux, uy = x << l if x >= 0 else -((-x) << l), y << l if y >= 0 else -((-y) << l)
            inside = 1 <= ux < W - 1 and 1 <= uy < H - 1                      # isInFrame(uvi, 1); tested first: the disparity outside the image does not exist
            d = float(np.float64(disp[uy, ux]) * (1.0 / (1 << l))) if inside else 0.0      # interpolateDisparity
            if inside and not d > 0:
                trace[l].append((idx, "disp")); continue
            if not inside:
                trace[l].append((idx, "border")); continue
            i = 0 if ux < third_w else (1 if ux < twothird_w else 2)
            j = 0 if uy < third_h else (1 if uy < twothird_h else 2)
            if not add_flags[i * 3 + j]:
                trace[l].append((idx, "flag")); continue
            if not is_window_empty(tree, x, y, R):
                trace[l].append((idx, "window")); continue
            trace[l].append((idx, "taken"))
            uvu = (float(x), float(y), float(x) - d)
            f = float(1 << l)
            px, py, pz = unmap_uvu(cam, uvu[0] * f, uvu[1] * f, uvu[2] * f)
            xyz = [((T[r, 0] * px + T[r, 1] * py) + T[r, 2] * pz) + T[r, 3] for r in range(3)]
            tree.append((float(x), float(y)))
            taken.append((xyz, uvu, l))
            n_new[l] += 1
            n += 1
            if n > cap:
                break
    m = len(taken)
    rec = dict(xyz_anchor=np.zeros((m, 3)), anchor_obs_pyr=np.zeros((m, 3)), anchor_level=np.zeros(m, np.int32), kf_index=np.full(m, kf_index, np.int32),
               point_id=np.zeros(m, np.int32))
    for k, (xyz, uvu, l) in enumerate(taken):      # newpoint_map[kf].push_front: the list is the reverse of the order the corners were taken in
        p = m - 1 - k
        rec["xyz_anchor"][p] = xyz; rec["anchor_obs_pyr"][p] = uvu; rec["anchor_level"][p] = l; rec["point_id"][p] = first_point_id + k
    return rec, np.array(n_new, np.int32), trace


def flags_from_grid3x3(num_points_grid3x3, min_num_points=25):
    """addNewKeyframe, stereo_frontend.cpp:322-331"""
    return (np.asarray(num_points_grid3x3) <= min_num_points).astype(np.int32)
