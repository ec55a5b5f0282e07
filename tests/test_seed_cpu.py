"""CPU tests of the new-point seeding yardstick (tests/seed_model.py): its clearance rule against the reference's own compiled quadtree, the whole procedure
against the points the reference's front end seeded at the keyframes of the sequence fixtures, the properties of the greedy and of the generated order, and the
binding of the new entry points."""
import os
import re

import numpy as np
import pytest

import seed_common as S
import seed_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_SYMBOLS = ["svs_seed_points", "svs_frontend_seed_keyframes", "svs_seed_params_default"]


def test_window_rule_equals_the_reference_quadtree():
    """>= 2 000 windows: points at least 1 apart (the reference's insert drops closer ones), fractional positions on and around all four window edges"""
    import oracle as O
    try:
        O.RefQuadTree.lib()
    except (FileNotFoundError, OSError):
        pytest.skip("oracle/_ref not built (needs the reference checkout)")
    rng = np.random.default_rng(5)
    n_windows, n_blocked = 0, 0
    e = 2.0 ** -20
    for trial in range(40):
        W, H = (160, 120) if trial % 2 else (80, 48)
        R = int(rng.integers(0, 4))
        centres = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(60)]
        pts = []
        for (x, y) in centres[:24]:      # on / just outside / just inside every edge of these windows
            k = len(pts) % 8
            dx, dy = ((-R, 0), (-R - e, 0), (R + 1 - e, 0), (R + 1, 0), (0, -R), (0, -R - e), (0, R + 1 - e), (0, R + 1))[k]
            pts.append((x + dx + (0.0 if k < 4 else float(rng.uniform(-R, R + 1 - e))), y + dy + (0.0 if k >= 4 else float(rng.uniform(-R, R + 1 - e)))))
        pts += [(float(rng.uniform(0, W)), float(rng.uniform(0, H))) for _ in range(40)]
        kept = []
        qt = O.RefQuadTree(W, H, 1.0)
        for (px, py) in pts:
            if not (0 <= px < W and 0 <= py < H) or any(np.hypot(px - qx, py - qy) < 1.5 for qx, qy in kept):
                continue
            kept.append((px, py))
            qt.insert(px, py, len(kept))
        for (x, y) in centres:
            ref = qt.is_window_empty(x - R, y - R, 2 * R + 1, 2 * R + 1)
            got = M.is_window_empty(kept, x, y, R)
            assert got == ref, (trial, x, y, R, [p for p in kept if abs(p[0] - x) < R + 2 and abs(p[1] - y) < R + 2])
            # ... and the occupancy-map form the device uses: exact on floor(p)
            assert got == (not any(x - R <= np.floor(px) <= x + R and y - R <= np.floor(py) <= y + R for px, py in kept))
            n_windows += 1
            n_blocked += not ref
    assert n_windows >= 2000 and 200 < n_blocked < n_windows - 200, (n_windows, n_blocked)


def test_whole_procedure_reproduces_what_the_reference_seeded():
    """both cameras, all 7 keyframes each: ids and levels identical, values 1e-6.  Frame 0 is mandatory; a later keyframe may be left out only if its FAST
    threshold guard fails, at most 2 of the 12"""
    left_out = []
    for cam in ("default", "newcollege"):
        kfs = S.keyframes(cam)
        assert len(kfs) == 7 and kfs[0] == 0
        for i in kfs:
            c = S.keyframe_case(cam, i)
            if not c["ok"]:
                assert i > 0 and c["why"] == "fast_thr", f"{cam} frame {i}: guard '{c['why']}' failed"
                left_out.append((cam, i))
                continue
            rec, n_new, _ = M.seed_points(c["corners"], c["orders"], c["disp"], c["cam"], c["tree_xy"], c["tree_level"], c["flags"], c["n0"],
                                          first_point_id=c["first_point_id"])
            S.assert_equals_reference(rec, c, f"{cam} frame {i}")
            if i == 0:
                assert n_new.tolist() == [301, 151, 76]      # all three caps hit
    assert len(left_out) <= 2, left_out


@pytest.mark.parametrize("W,H,R,nmp", [(80, 48, 2, 12), (96, 64, 0, 12), (80, 48, 1, 300), (96, 64, 3, 40)])
def test_greedy_properties(W, H, R, nmp):
    for variant in range(3):
        p = S.handmade_problem(W, H, 7, R, variant)
        rec, n_new, trace = M.seed_points(p["corners"], p["orders"], p["disp"], p["cam"], p["tree_xy"], p["tree_level"], p["flags"], p["n0"], T=p["T"],
                                          kf_index=p["kf_index"], first_point_id=p["first_point_id"], clearance=R, num_max_points=nmp)
        assert np.array_equal(rec["point_id"], p["first_point_id"] + np.arange(len(rec["point_id"]))[::-1])
        assert np.array_equal(rec["anchor_level"], np.sort(rec["anchor_level"])[::-1])      # level 2's last point first
        for l in range(3):
            cap = nmp >> l
            took = [idx for idx, why in trace[l] if why == "taken"]
            assert len(took) == n_new[l]
            capped = n_new[l] > 0 and p["n0"][l] + n_new[l] > cap
            # the count rule, including n0 > cap -> exactly one point
            assert n_new[l] <= max(cap - p["n0"][l], 0) + 1
            if p["n0"][l] > cap and any(why == "taken" for _, why in trace[l]):
                assert n_new[l] == 1
            if capped:
                assert trace[l][-1][1] == "taken"
            else:
                assert len(trace[l]) == len(p["orders"][l])      # every corner was visited
            xy = p["corners"][l].astype(np.int64)
            LW, LH = M.level_size(W, H, l)
            tree = [(x, y) for (x, y), tl in zip(p["tree_xy"], p["tree_level"]) if tl == l and 0 <= np.floor(x) < LW and 0 <= np.floor(y) < LH]
            for a, ia in enumerate(took):
                for ib in took[:a]:      # no two taken corners in each other's window
                    assert max(abs(xy[ia, 0] - xy[ib, 0]), abs(xy[ia, 1] - xy[ib, 1])) > R
                assert M.is_window_empty(tree, xy[ia, 0], xy[ia, 1], R)      # and none in a tree point's
            final = tree + [(float(xy[k, 0]), float(xy[k, 1])) for k in took]
            for idx, why in trace[l]:      # every visited corner that passed steps 1-3 and was not taken has a blocker
                if why == "window":
                    assert not M.is_window_empty(final, xy[idx, 0], xy[idx, 1], R)


@pytest.mark.parametrize("W", [80, 96, 512, 640])
def test_float_thirds(W):
    """float third = 1./3.; int third_width = W * third; int twothird_width = W * 2 * third: products in float, truncated"""
    import ctypes as C
    third = C.c_float(1.0 / 3.0).value
    a, b = M.thirds(W)
    assert a == int(C.c_float(C.c_float(W).value * third).value) and b == int(C.c_float(C.c_float(2 * W).value * third).value)
    assert (a, b) == {80: (26, 53), 96: (32, 64), 512: (170, 341), 640: (213, 426)}[W]


def test_generated_order():
    rng = np.random.default_rng(3)
    for seed, cells in [(1, [5, 0, 9, 3]), (0xDEADBEEFCAFEF00D, [40, 37, 41, 2, 0, 0, 13, 60, 1]), (7, [0, 0]), (9, [1]), (11, rng.integers(0, 30, 16).tolist())]:
        for level in range(3):
            o = M.generated_order(seed, level, cells)
            n = int(np.sum(cells))
            assert sorted(o.tolist()) == list(range(n))      # a permutation
            start = np.concatenate([[0], np.cumsum(cells)])
            cell_of = np.searchsorted(start, o, side="right") - 1
            for j in range(0, max(cells, default=0) + 1):      # every prefix ending on a round boundary holds min(n_c, j) corners of every cell
                m = int(sum(min(c, j) for c in cells))
                assert np.array_equal(np.bincount(cell_of[:m], minlength=len(cells)), np.minimum(cells, j))
            assert np.array_equal(o, M.generated_order(seed, level, cells))
        assert not np.array_equal(M.generated_order(seed, 0, cells), M.generated_order(seed, 1, cells)) or np.sum(cells) < 3
    assert not np.array_equal(M.generated_order(1, 0, [20, 20]), M.generated_order(2, 0, [20, 20]))
    assert M.splitmix64(0) == 0xE220A8397B1DCDAF


def test_generated_order_does_not_depend_on_the_batch_position():
    """the order is a function of (seed, level, cell counts): the same problem at another place in a batch, among other problems, gets the same order"""
    probs = [S.handmade_problem(80, 48, 7, 2, v) for v in range(3)]
    alone = [[M.generated_order(p["seed"], l, p["cells"][l]) for l in range(3)] for p in probs]
    for perm in ([2, 0, 1], [1, 2, 0]):
        batch = [probs[k] for k in perm]
        for pos, p in enumerate(batch):
            for l in range(3):
                assert np.array_equal(M.generated_order(p["seed"], l, p["cells"][l]), alone[perm[pos]][l])


def test_binding_names_the_seed_entry_points():
    from scavislam_amd import capi
    for n in SEED_SYMBOLS:
        assert n in capi.EXPORTS, n
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    for n in SEED_SYMBOLS:
        assert re.search(r"\b%s\(" % n, hdr), n
    lib = capi.load()
    for n in SEED_SYMBOLS:
        assert hasattr(lib, n)
    from scavislam_amd.ctypes_types import SeedParams
    p = SeedParams()
    lib.svs_seed_params_default(__import__("ctypes").byref(p))
    assert (p.clearance, p.num_max_points, p.min_num_points, p.n_levels) == (2, 300, 25, 3) and p.max_records() == 528


def test_pod_layouts_of_the_seed_structs(tmp_path):
    import ctypes as C
    import subprocess
    from scavislam_amd.ctypes_types import SEED_PROBLEM_DTYPE, SeedArgs, SeedParams, SeedRequest
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(svs_seed_params),sizeof(svs_seed_problem),sizeof(svs_seed_args),sizeof(svs_seed_request),"
                   "offsetof(svs_seed_problem,seed),offsetof(svs_seed_problem,n0),offsetof(svs_seed_problem,use_order),offsetof(svs_seed_problem,n_order),"
                   "offsetof(svs_seed_args,d_disp),offsetof(svs_seed_args,cam),offsetof(svs_seed_args,d_order),offsetof(svs_seed_args,batch),"
                   "offsetof(svs_seed_request,seed),offsetof(svs_seed_request,n_order));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    f = SEED_PROBLEM_DTYPE.fields
    assert got == [C.sizeof(SeedParams), SEED_PROBLEM_DTYPE.itemsize, C.sizeof(SeedArgs), C.sizeof(SeedRequest), f["seed"][1], f["n0"][1], f["use_order"][1],
                   f["n_order"][1], SeedArgs.d_disp.offset, SeedArgs.cam.offset, SeedArgs.d_order.offset, SeedArgs.batch.offset, SeedRequest.seed.offset,
                   SeedRequest.n_order.offset]
