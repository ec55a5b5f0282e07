"""Shared by the seeding tests: the inputs of StereoFrontend::addNewPoints / addMorePoints at the keyframes of the sequence fixtures
(tests/golden/ref_seq_*.npz: what the reference's own front end seeded there, `new_ids` / `new_val`), and hand-made problems for the kernel's edge cases."""
import os

import numpy as np

import seed_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
_fx, _frames, _cases = {}, {}, {}


def fixture(camname):
    if camname not in _fx:
        import seq_common
        fx = np.load(os.path.join(HERE, "golden", f"ref_seq_{camname}.npz"))
        _fx[camname] = (fx, seq_common.expand(fx))
    return _fx[camname]


def frame(camname, i):
    """(u8 image, f32 disparity) of frame i of the sequence, as seq_common.frames renders it"""
    if (camname, i) not in _frames:
        import seq_common
        from scavislam_amd import synth
        sc = synth.Scene(2011)
        traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)
        _frames[(camname, i)] = sc.render(seq_common.cam_of(camname), traj[i], seed=i)
    return _frames[(camname, i)]


def keyframes(camname):
    return [i for i, r in enumerate(fixture(camname)[1]) if r["dropped"]]


def order_from_reference(corners, ref_level, ref_obs):
    """visiting orders that make the greedy retrace the reference: per level the corners the reference took, in the order it took them (its list is push_front:
    reversed), then every other corner in list order.  Every corner the reference passed over failed a predicate, or was blocked by a SUBSET of the final tree,
    or was never reached behind the cap -- so the greedy must reproduce the reference's list from this order"""
    orders = []
    for l in range(3):
        xy = np.asarray(corners[l], np.int64)
        index = {(int(x), int(y)): k for k, (x, y) in enumerate(xy)}
        took = [index[(int(o[0]), int(o[1]))] for o in ref_obs[ref_level == l][::-1]]
        rest = [k for k in range(len(xy)) if k not in set(took)]
        orders.append(np.array(took + rest, np.int32))
    return orders


def keyframe_case(camname, i):
    """inputs and the reference's result at keyframe frame i; None if the rendered frame or the FAST thresholds do not reproduce the fixture's (guards)"""
    key = (camname, i)
    if key in _cases:
        return _cases[key]
    import oracle as O
    import seq_common
    fx, recs = fixture(camname)
    cam = seq_common.cam_of(camname)
    img, disp = frame(camname, i)
    r = recs[i]
    case = dict(cam=cam, img=img, disp=disp, frame=i, ok=True, why="")
    if seq_common.frame_crc(img, disp) != r["crc"]:
        case.update(ok=False, why="crc")
        _cases[key] = case
        return case
    pyr = O.build_pyramid(img)
    corners, cells, off, thr_now = [], [], 0, []
    for l in range(3):
        g = O.fastgrid_for_level(pyr[l].shape[1], pyr[l].shape[0], l)
        nc = g.gx * g.gy
        if i > 0:
            for c in range(nc):
                g.thr[c] = int(recs[i - 1]["fast_thr"][off + c])
        xy, cc, _ = O.fastgrid_detect_adaptively(g, pyr[l], 5 if i == 0 else 6)
        thr_now += [g.thr[c] for c in range(nc)]
        corners.append(xy); cells.append(cc[:nc].copy()); off += nc
    if not np.array_equal(np.array(thr_now), r["fast_thr"][:off]):
        case.update(ok=False, why="fast_thr")
        _cases[key] = case
        return case
    pts = r["pts"].astype(np.float64)
    tree_level = pts[:, 0].astype(np.int32) if i > 0 else np.zeros(0, np.int32)
    tree_xy = pts[:, 2:4] / 4.0 if i > 0 else np.zeros((0, 2))
    W, H = cam["w"], cam["h"]
    tw, ttw = M.thirds(W)
    th, tth = M.thirds(H)
    grid = np.zeros(9, np.int32)
    for (x, y), l in zip(tree_xy, tree_level):
        u, v = x * (1 << l), y * (1 << l)
        grid[(0 if u < tw else (1 if u < ttw else 2)) * 3 + (0 if v < th else (1 if v < tth else 2))] += 1
    ids, val = r["new_ids"], r["new_val"]
    case.update(corners=corners, cells=cells, tree_xy=tree_xy, tree_level=tree_level, n0=np.array([(tree_level == l).sum() for l in range(3)], np.int32),
                grid3x3=grid, flags=M.flags_from_grid3x3(grid) if i > 0 else np.ones(9, np.int32), ref_ids=ids, ref_val=val,
                first_point_id=int(ids[:, 0].min()) if len(ids) else 0, orders=order_from_reference(corners, ids[:, 1], val[:, 3:6]))
    _cases[key] = case
    return case


def assert_equals_reference(rec, case, what):
    """the bar seq_common.compare sets for these arrays: ids and levels identical, values within 1e-6"""
    ids, val = case["ref_ids"], case["ref_val"]
    assert len(rec["point_id"]) == len(ids), f"{what}: {len(rec['point_id'])} points, the reference seeded {len(ids)}"
    assert np.array_equal(rec["point_id"], ids[:, 0]) and np.array_equal(rec["anchor_level"], ids[:, 1]), f"{what}: ids / levels"
    got = np.hstack([rec["xyz_anchor"], rec["anchor_obs_pyr"]])
    assert np.abs(got - val).max() <= 1e-6, f"{what}: values differ by {np.abs(got - val).max()}"


# ---- hand-made problems for the kernel (small level-0 sizes; every edge the issue lists) ---------------------------------------------------------------------
def small_cam(W, H):
    return dict(f=0.6 * W, cx=W / 2.0 - 0.5, cy=H / 2.0 - 0.5, b=0.12, w=W, h=H)


def handmade_problem(W, H, seed, R, variant=0):
    """corners, cell counts (2 x 2 cells per level), disparity, tree points, flags, n0 and caller's orders of one problem.  variant 0 carries the planted edge
    cases; other variants only change the random content (batches of different problems)"""
    rng = np.random.default_rng(1000 * seed + variant)
    cam = small_cam(W, H)
    disp = rng.uniform(0.5, 6.0, (H, W)).astype(np.float32)
    tw, ttw = M.thirds(W)
    th, tth = M.thirds(H)
    corners, cells, tree_xy, tree_level = [], [], [], []
    planted, planted_edge = set(), set()
    for l in range(3):
        LW, LH = M.level_size(W, H, l)
        cw, ch = LW // 2, LH // 2
        n_target = (150, 40, 0)[l] if variant == 0 else (int(rng.integers(70, 160)), int(rng.integers(10, 50)), int(rng.integers(0, 12)))[l]
        per_cell = []
        for cj in range(2):
            for ci in range(2):
                want = n_target // 4 + (1 if (cj * 2 + ci) < n_target % 4 else 0)
                pix = set()
                if variant == 0 and l == 0 and ci == 0 and cj == 0:
                    # border (uvi 0 and W - 1 lies in another cell: added below), neighbours, dword boundary, the thirds
                    pix |= {(0, 5), (5, 0), (31, 9), (32, 9), (30, 11), (tw, 20), (tw - 1, 22), (10, th), (10, th - 1), (1, 1), (2, 2), (3, 1)}
                if variant == 0 and l == 0 and ci == 1 and cj == 0:
                    pix |= {(W - 1, 7), (W - 2, 3), (ttw, 15), (ttw - 1, 17), (63, 5), (64, 5), (65, 7)}
                if variant == 0 and l == 0 and ci == 1 and cj == 1:
                    pix |= {(W - 2, H - 2), (W - 3, H - 1), (W - 2, H - 3)}
                pix = {(x, y) for (x, y) in pix if ci * cw <= x < (ci + 1) * cw + (LW - 2 * cw if ci == 1 else 0) and cj * ch <= y < (cj + 1) * ch + (LH - 2 * ch if cj == 1 else 0)}
                if l == 0:
                    planted |= pix
                    if variant == 0:      # two corners per cell, clear of the others, whose window edges get a tree point each
                        for k in range(2):
                            e_ = (ci * cw + 8 + 14 * k, cj * ch + 14 + 4 * k)
                            pix.add(e_); planted.add(e_); planted_edge.add(e_)
                while len(pix) < want:
                    pix.add((int(rng.integers(ci * cw, (ci + 1) * cw)), int(rng.integers(cj * ch, (cj + 1) * ch))))
                per_cell.append(sorted(pix, key=lambda p: (p[1], p[0])))      # row-major inside the cell
        cells.append(np.array([len(p) for p in per_cell], np.int32))
        corners.append(np.array([p for cell in per_cell for p in cell], np.int16).reshape(-1, 2))
    # disparity 0, negative and NaN: under most corners of level 0, so that a cap of 12 is reached late (variant 0: under every corner that was not planted; variant 1,
    # with two flag cells only, never reaches it and walks all chunks; variant 2 reaches it inside a chunk)
    c0 = corners[0]
    keep = planted if variant == 0 else set()
    q = (0.0, 0.3, 0.25)[min(variant, 2)]
    for k, (x, y) in enumerate(c0.tolist()):
        if (x, y) not in keep and rng.uniform() >= q:
            disp[y, x] = (0.0, -1.5, np.nan)[k % 3]
    if variant == 0:
        # a tree point on and around all four edges of the windows of eight corners
        e = 2.0 ** -20
        edge = [k for k, (x, y) in enumerate(c0.tolist()) if (x, y) in planted_edge]
        for k, (dx, dy) in zip(edge, ((-R, 0), (-R - e, 0), (R + 1 - e, 0), (R + 1, 0), (0, -R), (0, -R - e), (0, R + 1 - e), (0, R + 1))):
            tree_xy.append((float(c0[k, 0]) + dx, float(c0[k, 1]) + dy)); tree_level.append(0)
        tree_xy += [(-3.0, 4.0), (1e9, 2.0), (float(W), 1.0), (5.5, float(H) + 0.25)]; tree_level += [0, 0, 0, 0]      # outside the level image: ignored
        tree_xy += [(7.25, 6.75), (3.0, 3.0)]; tree_level += [1, 5]
    for _ in range(int(rng.integers(5, 25))):
        l = int(rng.integers(0, 3))
        LW, LH = M.level_size(W, H, l)
        tree_xy.append((float(rng.uniform(0, LW)), float(rng.uniform(0, LH)))); tree_level.append(l)
    flags = np.ones(9, np.int32)
    flags[4 if variant == 0 else int(rng.integers(0, 9))] = 0      # a cleared flag cell
    if variant == 1:      # two cells only: few corners pass, so the walk goes through all chunks of the level without reaching the cap
        flags[:] = 0
        flags[[0, 5]] = 1
    n0 = np.array([0, 9, 0], np.int32) if variant == 0 else rng.integers(0, 8, 3).astype(np.int32)      # level 1 starts above its cap of 6: exactly one point
    if variant == 1:
        n0[0] = 0
    orders = [rng.permutation(len(c)).astype(np.int32) for c in corners]
    if variant == 0:      # neighbours adjacent in visiting order inside one chunk (positions 3, 4) and across a chunk boundary (63, 64)
        idx = {(int(x), int(y)): k for k, (x, y) in enumerate(corners[0])}
        o = [k for k in orders[0].tolist() if k not in (idx[(1, 1)], idx[(2, 2)], idx[(31, 9)], idx[(32, 9)])]
        o[3:3] = [idx[(1, 1)], idx[(2, 2)]]
        o[63:63] = [idx[(31, 9)], idx[(32, 9)]]
        orders[0] = np.array(o, np.int32)
    th_ = rng.uniform(-0.2, 0.2, 3)
    Rm = np.array([[1, -th_[2], th_[1]], [th_[2], 1, -th_[0]], [-th_[1], th_[0], 1.0]])
    T = np.hstack([np.linalg.qr(Rm)[0], rng.uniform(-1, 1, (3, 1))])      # a non-identity T_newkey_from_cur
    return dict(cam=cam, disp=disp, corners=corners, cells=cells, tree_xy=np.array(tree_xy, np.float64).reshape(-1, 2), tree_level=np.array(tree_level, np.int32),
                flags=flags, n0=n0, orders=orders, T=T, kf_index=3 + variant, first_point_id=1000 * (variant + 1), seed=0x9E3779B97F4A7C15 * (seed + 1) + variant)
