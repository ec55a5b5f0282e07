"""CPU tests of the loop-closure geometric check's yardstick (tests/loop_model.py) and of its boundary: the model recovers a planted pose, its sample
generator keeps the rule of ransac.cpp:68-96 and gives up after 64 draws, its two fits agree, and the binding names the new entry points."""
import os
import re

import numpy as np

import loop_model as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_SYMBOLS = ["svs_loop_check_batch", "svs_loop_create", "svs_loop_destroy", "svs_loop_set_place", "svs_loop_set_timing", "svs_loop_stage_times"]


def test_model_recovers_a_planted_pose():
    sc = L.make_scene(1, 200, 240, 64)
    tidx, _ = L.match(sc["q_desc"], sc["t_desc"])
    planted = sc["truth"] >= 0
    assert np.array_equal(tidx[planted], sc["truth"][planted])
    m = L.ransac(sc["cam"], sc["q_uvu"], sc["t_xyz"], tidx, L.draw_triples(1, 100, len(tidx), tidx))
    assert m["best"] >= 0 and m["n_inliers"] > 30 and m["n_inliers"] == m["hyp_inliers"][m["best"]]
    assert m["inlier"][planted].sum() >= m["n_inliers"] - 2                  # the inliers are the planted correspondences
    dR = m["T"][:, :3] @ sc["T_true"][:, :3].T
    assert np.arccos(min(1.0, (np.trace(dR) - 1) / 2)) < 0.01 and np.abs(m["T"][:, 3] - sc["T_true"][:, 3]).max() < 0.05


def test_generator_keeps_the_rule_and_stops_at_64_draws(monkeypatch):
    sc = L.make_scene(13, 300, 150, 64)                                      # more queries than trains: shared train indices
    tidx, _ = L.match(sc["q_desc"], sc["t_desc"])
    assert len(set(tidx.tolist())) < len(tidx)
    smp = L.draw_triples(5, 256, len(tidx), tidx)
    assert (smp >= 0).all() and (smp < len(tidx)).all()
    for r in smp:
        assert len(set(r.tolist())) == 3 and len(set(tidx[r].tolist())) == 3
    assert len({tuple(r) for r in smp.tolist()}) > 250                       # hypotheses differ
    assert np.array_equal(smp, L.draw_triples(5, 256, len(tidx), tidx))
    # the known answer of the header's text: splitmix64(0) and one draw
    assert L.splitmix64(0) == 0xE220A8397B1DCDAF
    assert L.draw(0, 0, 0, 1 << 20) == 0xE220A8397B1DCDAF >> 44
    # three matches, one train index twice: no valid triple exists; the reference would loop forever
    calls = []
    real = L.draw
    monkeypatch.setattr(L, "draw", lambda *a: (calls.append(a[2]), real(*a))[1])
    assert L.draw_triple(9, 0, 3, np.array([4, 7, 4])) is None
    assert calls == list(range(64))
    assert L.draw_triple(9, 0, 2, np.array([0, 1])) is None


def test_svd_and_horn_fits_agree():
    sc = L.make_scene(2, 200, 240, 64)
    tidx, _ = L.match(sc["q_desc"], sc["t_desc"])
    x = sc["t_xyz"][tidx]
    worst = 0.0
    for r in L.draw_triples(3, 60, len(tidx), tidx):
        p0, p1 = L.unmap_uvu(sc["cam"], sc["q_uvu"][r]), sc["t_xyz"][tidx[r]]
        Ta, Tb = L.fit_svd(p0, p1), L.fit_horn(p0, p1)
        for T in (Ta, Tb):
            assert np.abs(T[:, :3].T @ T[:, :3] - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(T[:, :3]) - 1) < 1e-12
        near = L.residuals(sc["cam"], Ta, x, sc["q_uvu"]).max(1) < 50.0
        pa, pb = L.map_uvu(sc["cam"], x @ Ta[:, :3].T + Ta[:, 3]), L.map_uvu(sc["cam"], x @ Tb[:, :3].T + Tb[:, 3])
        worst = max(worst, np.abs(pa - pb)[near].max() if near.any() else 0.0)
    assert worst < 1e-6, worst


def test_unmap_then_map_is_the_identity_to_rounding():
    rng = np.random.default_rng(0)
    u = rng.uniform(0, 640, 50)
    uvu = np.stack([u, rng.uniform(0, 480, 50), u - rng.uniform(5, 60, 50)], 1)
    assert np.abs(L.map_uvu(L.CAM, L.unmap_uvu(L.CAM, uvu)) - uvu).max() < 1e-10


def test_binding_names_the_loop_entry_points():
    from scavislam_amd import capi
    for n in LOOP_SYMBOLS:
        assert n in capi.EXPORTS, n
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    lib = capi.load()
    for n in LOOP_SYMBOLS:
        assert hasattr(lib, n)


def test_pod_layouts_of_the_loop_structs(tmp_path):
    import ctypes as C
    import subprocess
    from scavislam_amd.ctypes_types import LoopCheck, LoopResult
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",sizeof(svs_loop_check),'
                   "sizeof(svs_loop_result),offsetof(svs_loop_check,pixel_thr),offsetof(svs_loop_check,h_samples),offsetof(svs_loop_result,T_query_from_train));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(LoopCheck), C.sizeof(LoopResult), LoopCheck.pixel_thr.offset, LoopCheck.h_samples.offset, LoopResult.T_query_from_train.offset]
