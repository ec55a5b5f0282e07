"""NumPy restatement of the front half of PlaceRecognizer::addLocation (placerecognizer.cpp:248-318: visual words, the inverted index, TF-IDF place scores, the
candidate test): the yardstick of tests/test_place_cpu.py and tests/test_gpu_place_index.py.  Written from the reference's text and from the header's
(include/scavislam_hip.h, svs_loop_set_vocabulary / svs_loop_add_locations), not from the kernels:

  words()          the exact nearest word inside the squared radius (what flann_index_->radiusSearch approximates), f64 distances on the differences
  LiteralIndex     addLocation / calcLoopStatistics with dicts where the reference has unordered_maps, every operation wrapped in np.float32
  DenseIndex       the same state as matrices cnt[w][slot], df[w], nw[slot]: an independent second restatement
  make_places()    the seeded scenario of the GPU tests
"""
import os

import numpy as np

import loop_model as L

RADIUS = 0.1          # placerecognizer.cpp:264; cvflann's L2 is the squared distance
MIN_SCORE = 2.0       # :316
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surfwords_head1024.npz")


def fixture_words():
    return np.load(GOLDEN)["words"]


# ---- words -----------------------------------------------------------------------------------------------------------------------------------------------
def words(desc, vocab, radius=RADIUS):
    """word [n] (-1: none inside the radius), the f64 distance matrix D [n][n_words] and the bound B [n] of loop_model.match_bound"""
    D = L.sqdist(desc, vocab)
    j = np.argmin(D, axis=1).astype(np.int32)
    best = D[np.arange(len(D)), j]
    return np.where(best < radius, j, -1).astype(np.int32), D, L.match_bound(desc, vocab)


def bands_empty(D, B, radius=RADIUS):
    """the preconditions under which the device's words must EQUAL the model's: the best two distances further apart than 2 B, the best further than B
    from the radius"""
    srt = np.sort(D, axis=1)
    gap = srt[:, 1] - srt[:, 0] > 2 * B if D.shape[1] > 1 else np.ones(len(D), bool)
    return bool(gap.all()), bool((np.abs(srt[:, 0] - radius) > B).all())


def pick_best(stats):
    """the greatest score above 0; the lowest slot on a tie (the reference: the first in hash-map order)"""
    best, score = -1, F32(0)
    for o in sorted(stats):
        if stats[o] > score:
            best, score = o, stats[o]
    return best, score


# ---- the literal restatement -----------------------------------------------------------------------------------------------------------------------------
class LiteralIndex:
    def __init__(self, n_words):
        self.inverted_index = [dict() for _ in range(n_words)]      # word -> {slot: count}           inverted_index_
        self.location_map = {}                                      # slot -> number_of_words          location_map_

    def calc_loop_statistics(self, cur, exclude, kf_to_wordcount, location_stats, terms):
        number_of_locations = F32(len(self.location_map))
        number_of_locations_containing_word = F32(len(kf_to_wordcount))
        if number_of_locations_containing_word > 0:
            idf = F32(number_of_locations / number_of_locations_containing_word)
            for other, count in kf_to_wordcount.items():
                if other == cur or other in exclude:
                    continue
                tf = F32(F32(count) / F32(self.location_map[other]))
                val = F32(tf * idf)
                location_stats[other] = F32(location_stats.get(other, F32(0)) + val)
                terms.setdefault(other, []).append(val)

    def add_location(self, slot, word, do_loop_detection=True, exclude=(), min_score=MIN_SCORE):
        exclude = set(int(e) for e in exclude)
        location_stats, terms, number_of_words = {}, {}, 0
        for w in word:
            if w < 0:
                continue
            number_of_words += 1
            m = self.inverted_index[int(w)]
            if do_loop_detection:
                self.calc_loop_statistics(slot, exclude, m, location_stats, terms)
            m[slot] = m.get(slot, 0) + 1
        self.location_map[slot] = number_of_words
        best, score = pick_best(location_stats) if do_loop_detection else (-1, F32(0))
        return dict(number_of_words=number_of_words, stats=location_stats, terms=terms, n_scored=len(location_stats), best_slot=best, best_score=score,
                    candidate=bool(score > F32(min_score)))


# ---- the dense restatement -------------------------------------------------------------------------------------------------------------------------------
class DenseIndex:
    def __init__(self, n_words, max_places):
        self.cnt = np.zeros((n_words, max_places), np.int32)
        self.df = np.zeros(n_words, np.int32)
        self.nw = np.zeros(max_places, np.int32)
        self.n_loc = 0

    def add_location(self, slot, word, do_loop_detection=True, exclude=(), min_score=MIN_SCORE):
        P = self.cnt.shape[1]
        allowed = np.ones(P, bool)
        allowed[slot] = False
        allowed[list(exclude)] = False
        score, got, number_of_words = np.zeros(P, F32), np.zeros(P, bool), 0
        for w in word:
            if w < 0:
                continue
            number_of_words += 1
            if do_loop_detection and self.df[w] > 0:
                idf = F32(self.n_loc) / F32(self.df[w])
                m = (self.cnt[w] > 0) & allowed
                tf = self.cnt[w][m].astype(F32) / self.nw[m].astype(F32)
                score[m] = score[m] + tf * idf
                got |= m
            if self.cnt[w, slot] == 0:
                self.df[w] += 1
            self.cnt[w, slot] += 1
        self.nw[slot] = number_of_words
        self.n_loc += 1
        pos = np.where(got & (score > 0))[0]
        best = int(pos[np.argmax(score[pos])]) if len(pos) else -1          # argmax: the first, hence the lowest slot
        bs = score[best] if best >= 0 else F32(0)
        return dict(number_of_words=number_of_words, scores=score, n_scored=int(got.sum()), best_slot=best, best_score=bs, candidate=bool(bs > F32(min_score)))


def scores_row(stats, max_places):
    row = np.zeros(max_places, F32)
    for o, v in stats.items():
        row[o] = v
    return row


# ---- the scenario ----------------------------------------------------------------------------------------------------------------------------------------
def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def descriptors(rng, vocab, src):
    """normalise(word + sigma noise): sigma 0.02 for four of five descriptors (well inside the radius), 0.08 for the fifth (far outside)"""
    n = len(src)
    sigma = np.where(np.arange(n) % 5 == 4, 0.08, 0.02)[:, None]
    return _unit(vocab[src].astype(np.float64) + sigma * rng.normal(size=(n, vocab.shape[1]))).astype(np.float32)


def make_places(vocab, seed=5, n_places=12, lo=200, hi=330, revisit=(9, 2, 0.7), geometry=True):
    """n_places places of lo .. hi descriptors on words drawn from the vocabulary.  revisit = (a, b, frac): place a sees place b again -- the pair is one
    loop_model.make_scene (a = query, b = train; with geometry=False a's observations are unrelated), and the planted frac of a's descriptors re-draw the
    words of the train descriptors they observe.  Each place: dict(desc, uvu, src)"""
    rng = np.random.default_rng(seed)
    n = rng.integers(lo, hi + 1, n_places)
    src = [rng.integers(0, len(vocab), int(k)) for k in n]
    uvu = []
    for k in n:
        u = rng.uniform(0, L.CAM["w"], int(k))
        uvu.append(np.stack([u, rng.uniform(0, L.CAM["h"], int(k)), u - rng.uniform(10.0, 40.0, int(k))], 1))
    if revisit is not None:
        a, b, frac = revisit
        sc = L.make_scene(seed + 100, int(n[a]), int(n[b]), vocab.shape[1], inlier_frac=frac)
        uvu[b] = sc["t_uvu"]
        if geometry:
            uvu[a] = sc["q_uvu"]
        src[a] = np.where(sc["truth"] >= 0, src[b][np.maximum(sc["truth"], 0)], src[a])
    out = []
    for p in range(n_places):
        out.append(dict(desc=descriptors(rng, vocab, src[p]), uvu=np.ascontiguousarray(uvu[p]), src=src[p]))
    return out


def excludes(p):
    """every place excludes itself and its two predecessors"""
    return [q for q in (p, p - 1, p - 2) if q >= 0]
