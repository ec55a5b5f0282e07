"""The arithmetic half of the reference's dictionary program (create_dictionary.cpp:144-177) on the device: descriptors in, visual words out.
DESCRIPTORS.npy holds [n][64 or 128] f32 rows (any extractor; the reference's image loading, SURF and PNG container are not covered).  Like the reference
(:218) it refuses fewer than 10 x TARGET_NUM_WORDS rows.  Writes surfwords<N>.npy, N = the number of words that came back, into the current directory.
usage: python tools/create_dictionary.py DESCRIPTORS.npy [TARGET_NUM_WORDS = 10000] [--iterations 11] [--seed 0]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("descriptors")
    ap.add_argument("target_num_words", nargs="?", type=int, default=10000)
    ap.add_argument("--iterations", type=int, default=11)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    d = np.load(a.descriptors)
    if d.ndim != 2 or d.shape[1] not in (64, 128):
        sys.exit(f"{a.descriptors}: [n][64] or [n][128] expected, got {d.shape}")
    if a.target_num_words < 1 or len(d) < 10 * a.target_num_words:
        sys.exit(f"{len(d)} descriptors are too few for {a.target_num_words} words: at least {10 * a.target_num_words} are needed")
    from scavislam_amd import capi
    from scavislam_amd.loop import train_vocabulary, vocabulary_stage_times_ms
    ctx = capi.Context(0)
    out = train_vocabulary(ctx, d, a.target_num_words, iterations=a.iterations, seed=a.seed)
    ms = vocabulary_stage_times_ms(ctx)
    ctx.close()
    name = f"surfwords{out.n_words_out}.npy"
    np.save(name, out.words)
    print(f"{name}: {out.n_words_out} words of {d.shape[1]} from {len(d)} descriptors; seeded {out.n_seeded}, {out.iterations_run} iterations"
          f"{' (converged)' if out.converged else ''}, {out.n_empty} empty, changed {out.changed.tolist()}, mean d2 {out.inertia_q28 / 2.0 ** 28 / len(d):.6f}; "
          f"device ms: seeding {ms[0]:.1f}, assignment {ms[1]:.1f}, update {ms[2]:.1f}")


if __name__ == "__main__":
    main()
