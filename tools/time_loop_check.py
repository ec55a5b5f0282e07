"""loop-closure geometric check (svs_loop_check_batch: descriptor matching + SE3 RANSAC): device time of ONE check and of a BATCH of 32, per stage from the
library's own events (svs_loop_set_timing), at (N, M) = (500, 500) and (2000, 2000), K = 64, H = 100; the same checks through the vectorised NumPy of
tests/loop_model.py on this host beside them (the only CPU figure there is: the reference's OpenCV / Eigen form is not buildable here and nobody has timed it).
usage: python tools/time_loop_check.py [out.md]
Prints a markdown table (and writes it when a path is given).  The one condition: 32 checks in one call take less device time than 32 single calls measured in
the same run."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import loop_model as L
from scavislam_amd import capi
from scavislam_amd.loop import GeometricChecker

K, H, NB, ROUNDS = 64, 100, 32, 7
CLOCK_GHZ, CUS = 2.4, 256                       # datasheet peak engine clock; f32-input MFMA: 64 FLOP per clock and SIMD
MFMA_PEAK = CUS * 4 * 64 * CLOCK_GHZ * 1e9

ctx = capi.Context(0)
rows = []
for (N, M) in ((500, 500), (2000, 2000)):
    gc = GeometricChecker(ctx, L.CAM, desc_dim=K, max_desc=max(N, M), max_places=2 * NB, max_hyp=H, max_checks=NB)
    scenes = [L.make_scene(1000 + i, N, M, K) for i in range(NB)]      # 32 different place pairs
    for i, sc in enumerate(scenes):
        gc.set_place(2 * i, sc["t_desc"], sc["t_uvu"])
        gc.set_place(2 * i + 1, sc["q_desc"], sc["q_uvu"])
    checks = [dict(query=2 * i + 1, train=2 * i, n_hyp=H, seed=i) for i in range(NB)]
    gc.set_timing(True)
    outs = gc.check_batch(checks)                                     # warm-up, and the results the CPU run is compared with
    single, batch = [], []
    for r in range(ROUNDS):                                           # alternated in one process
        s = np.zeros(2)
        for c in checks:
            gc.check_batch([c])
            s += gc.stage_times_ms()
        single.append(s)
        gc.check_batch(checks)
        batch.append(np.array(gc.stage_times_ms()))
    single, batch = np.median(single, 0), np.median(batch, 0)        # single: the SUM over the 32 single calls
    t0 = time.perf_counter()
    for i in range(2):
        sc = scenes[i]
        tidx, _ = L.match(sc["q_desc"], sc["t_desc"])
        m = L.ransac(sc["cam"], sc["q_uvu"], sc["t_xyz"], tidx, L.draw_triples(i, H, N, tidx))
        assert m["n_inliers"] == outs[i].n_inliers and np.array_equal(tidx, outs[i].train_idx), "device and model disagree"
    cpu_ms = (time.perf_counter() - t0) / 2 * 1e3
    flop = 2.0 * N * M * K
    rows.append((N, M, single / NB, batch, single.sum() / NB, batch.sum(), batch.sum() / single.sum(), cpu_ms, flop / (single[0] / NB * 1e-3) / MFMA_PEAK,
                 NB * flop / (batch[0] * 1e-3) / MFMA_PEAK, int(np.mean([o.n_inliers for o in outs]))))
    gc.close()
ctx.close()

out = ["| N x M | one check: match / RANSAC / both (ms) | batch of 32: match / RANSAC / both (ms) | batch / 32 singles | f32 MFMA rate, one check | f32 MFMA rate, batch | "
       "NumPy model, one check on the host (ms) | mean inliers |", "|---|---:|---:|---:|---:|---:|---:|---:|"]
for (N, M, s, b, s_all, b_all, ratio, cpu, f1, fb, inl) in rows:
    out.append(f"| {N} x {M} | {s[0]:.4f} / {s[1]:.4f} / {s_all:.4f} | {b[0]:.4f} / {b[1]:.4f} / {b_all:.4f} | {ratio:.3f} | {100 * f1:.2f} % | {100 * fb:.2f} % | {cpu:.1f} | {inl} |")
    assert ratio < 1.0, "a batch of 32 must take less device time than 32 single calls"
text = "\n".join(out)
print(text)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(text + "\n")
