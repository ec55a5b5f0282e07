"""place index (svs_loop_add_locations: visual words + TF-IDF scores): device time per stage from the library's own events (svs_loop_set_timing), K = 64,
a seeded vocabulary of 9 983 random unit rows, places of N = 500 and N = 2 000 descriptors built like the test scenario's (four of five inside the radius).
  (a) the words stage of ONE location against the same arithmetic through the existing entry point: the vocabulary loaded as a place, one svs_loop_check_batch,
      its distance stage (svs_loop_stage_times).  Condition: the new stage is not slower, at either N.
  (b) 32 locations in one call against 32 single calls (words + scoring).  Condition: the batch takes less device time.
Medians over 7 rounds, the forms alternating in one process; the index is emptied (svs_loop_set_vocabulary) in front of every form, outside the brackets.
usage: python tools/time_place_index.py [out.md]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import loop_model as L
import place_model as M
from scavislam_amd import capi
from scavislam_amd.loop import GeometricChecker

K, NW, NB, ROUNDS = 64, 9983, 32, 7
CLOCK_GHZ, CUS = 2.4, 256                       # datasheet peak engine clock; f32-input MFMA: 64 FLOP per clock and SIMD
MFMA_PEAK = CUS * 4 * 64 * CLOCK_GHZ * 1e9

rng = np.random.default_rng(1)
V = rng.normal(size=(NW, K))
V = (V / np.linalg.norm(V, axis=1, keepdims=True)).astype(np.float32)
ctx = capi.Context(0)
rows = []
for N in (500, 2000):
    places = [M.descriptors(rng, V, rng.integers(0, NW, N)) for _ in range(NB)]
    u = rng.uniform(60, 600, NW)
    uvu = np.stack([u, rng.uniform(0, 480, NW), u - 20.0], 1)
    # the yardstick: the vocabulary as train place NB of a store with max_desc >= 9 983
    gc = GeometricChecker(ctx, L.CAM, desc_dim=K, max_desc=NW, max_places=NB + 1, max_hyp=1, max_checks=NB)
    for p, d in enumerate(places):
        gc.set_place(p, d, uvu[:N])
    gc.set_place(NB, V, uvu)
    gc.set_timing(True)
    locs = [dict(slot=p, exclude=[p]) for p in range(NB)]
    gc.set_vocabulary(V)
    batch_out = gc.add_locations(locs)                                          # warm-up, and what the other forms are compared with
    ref = gc.check_batch([dict(query=0, train=NB, n_hyp=1, seed=0)])[0]
    assert np.array_equal(np.where(batch_out[0].word >= 0, ref.train_idx, -1), batch_out[0].word), "the two entry points disagree on the words"
    old, new1, single, batch = [], [], [], []
    for r in range(ROUNDS):
        gc.check_batch([dict(query=0, train=NB, n_hyp=1, seed=0)])
        old.append(gc.stage_times_ms()[0])
        gc.set_vocabulary(V)
        s = np.zeros(2)
        for k, c in enumerate(locs):
            o = gc.add_locations([c])[0]
            t = np.array(gc.index_stage_times_ms())
            s += t
            if k == 0:
                new1.append(t[0])
            assert np.array_equal(o.scores.view(np.uint32), batch_out[k].scores.view(np.uint32)) and np.array_equal(o.word, batch_out[k].word)
        single.append(s)
        gc.set_vocabulary(V)
        gc.add_locations(locs)
        batch.append(np.array(gc.index_stage_times_ms()))
    old, new1, single, batch = np.median(old), np.median(new1), np.median(single, 0), np.median(batch, 0)
    flop = 2.0 * N * NW * K
    rows.append((N, old, new1, new1 / old, flop / (old * 1e-3) / MFMA_PEAK, flop / (new1 * 1e-3) / MFMA_PEAK, single, batch, batch.sum() / single.sum(),
                 NB * flop / (batch[0] * 1e-3) / MFMA_PEAK, float(np.mean([o.number_of_words for o in batch_out])), float(np.mean([o.n_scored for o in batch_out]))))
    gc.close()
ctx.close()

out = ["| N x 9983 | distance stage of svs_loop_check_batch (ms) | words stage, one location (ms) | new / old | f32 MFMA rate old / new | 32 singles: words / scoring (ms) | "
       "batch of 32: words / scoring (ms) | batch / 32 singles | f32 MFMA rate, batch | mean words | mean places scored |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
for (N, old, new1, ratio, f_old, f_new, s, b, br, fb, nwd, nsc) in rows:
    out.append(f"| {N} | {old:.4f} | {new1:.4f} | {ratio:.3f} | {100 * f_old:.2f} % / {100 * f_new:.2f} % | {s[0]:.4f} / {s[1]:.4f} | {b[0]:.4f} / {b[1]:.4f} | {br:.3f} | "
               f"{100 * fb:.2f} % | {nwd:.0f} | {nsc:.1f} |")
text = "\n".join(out)
print(text)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(text + "\n")
for (N, old, new1, ratio, f_old, f_new, s, b, br, fb, nwd, nsc) in rows:
    assert ratio <= 1.0, f"N = {N}: the words stage must not be slower than the distance stage of svs_loop_check_batch on the same arithmetic"
    assert br < 1.0, f"N = {N}: a batch of 32 must take less device time than 32 single calls"
