"""svs_vocab_train at the reference's scale (create_dictionary.cpp: up to ~300 000 SURF descriptors into 10 000 words, 11 iterations): device time of the seeding,
the assignment launches and the update launches from the library's own events (svs_vocab_stage_times), and the wall time of the call; K = 64, 150 000 unit
rows drawn around 12 000 seeded unit rows as the tests draw theirs.  The NumPy restatement (tests/vocab_model.py) is timed at a stated smaller size.
No bar was fixed in advance: these are the first numbers of this code.
usage: python tools/time_vocab_train.py [out.md] [--small]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import vocab_model as V
from scavislam_amd import capi
from scavislam_amd.loop import train_vocabulary, vocabulary_stage_times_ms

small = "--small" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
K = 64
N, NW, NB = (20000, 1000, 1500) if small else (150000, 10000, 12000)
MN, MNW = 3000, 100                                   # the model's size

X = V.points(V.unit_rows(3, NB, K), N, 4)
ctx = capi.Context(0)
train_vocabulary(ctx, X[:4096], 64, iterations=2)      # warm-up: code objects, allocator
rows = []
for it in (0, 1, 11):
    t0 = time.perf_counter()
    out = train_vocabulary(ctx, X, NW, iterations=it, seed=1)
    wall = (time.perf_counter() - t0) * 1e3
    ms = vocabulary_stage_times_ms(ctx)
    rows.append((it, out, ms, wall))
    print(f"iterations {it}: wall {wall:.1f} ms, stages {ms}", flush=True)
Xm = X[:MN]
t0 = time.perf_counter()
m = V.train(Xm, MNW, 11, 1)
model_s = time.perf_counter() - t0
t0 = time.perf_counter()
dev = train_vocabulary(ctx, Xm, MNW, iterations=11, seed=1)
dev_small_ms = (time.perf_counter() - t0) * 1e3
ctx.close()

out = [f"svs_vocab_train, {N} x {K} descriptors -> {NW} words (1 x MI355X; device times from events, wall time of the blocking call).  First numbers of this code: no bar was set in advance.",
       "",
       "| iterations asked / run | seeding (ms) | per seeding step: 2 launches (us) | assignment, all iterations (ms) | per iteration (ms) | update, all iterations (ms) | per iteration (ms) | wall (ms) | words out | empty |",
       "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
for it, o, ms, wall in rows:
    r = max(o.iterations_run, 1)
    out.append(f"| {it} / {o.iterations_run} | {ms[0]:.1f} | {1e3 * ms[0] / max(NW - 1, 1):.1f} | {ms[1]:.2f} | {ms[1] / r:.2f} | {ms[2]:.2f} | {ms[2] / r:.2f} | {wall:.1f} | {o.n_words_out} | {o.n_empty} |")
flop = 2.0 * N * NW * K
it, o, ms, wall = rows[-1]
if o.iterations_run:
    out += ["", f"Assignment: {flop / 1e9:.1f} GFLOP per iteration, {flop * o.iterations_run / (ms[1] * 1e-3) / 1e12:.1f} TFLOP/s in f32-input MFMA.  "
            f"Update: 64-bit integer atomics, one wave instruction per point's row ({N * K * 8 / 1e6:.0f} MB of added int64 per iteration, "
            f"{N * K * 8 * o.iterations_run / (ms[2] * 1e-3) / 1e9:.0f} GB/s including the reset and the division pass); the counting-sort form was not built."]
out += ["", f"NumPy restatement (tests/vocab_model.py) at {MN} x {K} -> {MNW} words, 11 iterations: {model_s:.2f} s on the host; the device call on the same input: {dev_small_ms:.1f} ms wall "
        f"({dev.iterations_run} iterations, model {m['iterations_run']})."]
text = "\n".join(out)
print(text)
if args:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    open(args[0], "w").write(text + "\n")
