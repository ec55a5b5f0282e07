"""newpoint_map on the device (svs_frontend_newpoints_*, svs_newpoints_prune, svs_frontend_seed_newpoints, svs_frontend_set_candidates_from_newpoints) against
tests/newpoint_model.py, which tests/test_newpoint_cpu.py holds to the reference's three uses of the map.

Bounds.  Everything here is copying and integer compaction: every output byte must be the model's.  What lies in a stream's record row BEHIND its live records is
unspecified (a compaction leaves the old bytes there) and not compared; what lies outside a stream's rows must stay untouched and is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import newpoint_model as NM

pytestmark = pytest.mark.gpu
FILL = 0xAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
NM_RESULT = ("n_points", "n_head", "n_groups", "n_no_slot", "over_capacity")


# ---- the stateless prune at its edges -------------------------------------------------------------------------------------------------------------------------
def step_case(rng, groups, P_want, n_extra=0, n_new=None):
    """a stream: `groups` (a list of record arrays, the store) and a fabricated step whose new list holds exactly the ids P_want (and n_extra records that are
    no part of it: not OK, not accepted, skipped)"""
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, GATED_POINT_DTYPE, MATCH_RESULT_DTYPE
    ids = list(P_want)
    n = len(ids) + n_extra
    res, gated, pts = np.zeros(n, MATCH_RESULT_DTYPE), np.zeros(n, GATED_POINT_DTYPE), np.zeros(n, CANDIDATE_DTYPE)
    place = rng.permutation(n)[:len(ids)]
    place.sort()
    res["status"], gated["accepted"], gated["is_new"] = rng.choice([0, 0, 1, 2, 3, 4, 5, 6, 7], n), rng.integers(0, 2, n), 1
    pts["point_id"] = 10 ** 7 + np.arange(n)                       # ids the store does not hold, unless placed below
    live = [int(i) for g in groups for i in g["point_id"]]
    for i in range(n):                                             # the records that must NOT prune carry ids of the store: a wrong test would show
        if live and i not in place:
            pts["point_id"][i] = live[int(rng.integers(0, len(live)))]
            if res["status"][i] == 0 and gated["accepted"][i]:
                gated["accepted"][i] = 0                           # matched, not accepted
    res["status"][place], gated["accepted"][place], pts["point_id"][place] = 0, 1 + rng.integers(0, 3, len(ids)), ids
    return dict(res=res, gated=gated, pts=pts, n_new=n if n_new is None else n_new, groups=groups)


def make_groups(rng, sizes, first_id=1):
    out = []
    for s in sizes:
        out.append(NM.random_records(rng, s, first_id, kf_index=int(rng.integers(0, 4))))
        first_id += s
    return out


def run_prune(gpu_ctx, cases, indexed=False, expect_error=False, group_stride=None):
    """one svs_newpoints_prune call; returns per case (n_removed, counts, live records) and checks the canaries between the streams' rows.  indexed: the batch
    names its streams through d_stream, in reverse, among rows of streams the call does not name"""
    import torch
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, GATED_POINT_DTYPE, MATCH_RESULT_DTYPE, NewpointsPruneArgs
    ctx, stream = gpu_ctx
    R = len(cases)
    rows = list(range(R)) if not indexed else [2 * (R - 1 - r) + 1 for r in range(R)]
    S = R if not indexed else 2 * R + 1
    n = max(len(c["res"]) for c in cases)
    cap = max(1, max(sum(len(g) for g in c["groups"]) for c in cases))
    NG = max(1, max(len(c["groups"]) for c in cases))
    GS = group_stride or (NG + 1 if NG < 64 else 64)              # a canary column behind the groups wherever the row may be wider than they are
    res, pts, gated = np.zeros((S, n + 2), MATCH_RESULT_DTYPE), np.zeros((S, n + 3), CANDIDATE_DTYPE), np.zeros((S, n + 1), GATED_POINT_DTYPE)
    gated["accepted"], pts["point_id"] = 1, 1                      # behind a stream's own records: OK and accepted garbage with a live id, which d_n keeps out
    ns, nn, ng = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    store = np.full((S, cap + 2, 64), FILL, np.uint8)
    counts = np.full((S, GS), -9, np.int32)
    for r, c in zip(rows, cases):
        k = len(c["res"])
        res[r, :k], pts[r, :k], gated[r, :k] = c["res"], c["pts"], c["gated"]
        ns[r], nn[r], ng[r] = k, c["n_new"], len(c["groups"])
        rec = np.concatenate(c["groups"]) if c["groups"] else np.zeros(0, CANDIDATE_DTYPE)
        store[r, :len(rec)] = rec.view(np.uint8).reshape(-1, 64)
        counts[r, :len(c["groups"])] = [len(g) for g in c["groups"]]
    before = store.copy()
    with torch.cuda.stream(stream):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        d = dict(res=dev(res), pts=dev(pts), gated=dev(gated), n=dev(ns), nn=dev(nn), ng=dev(ng), store=dev(store), counts=dev(counts),
                 rows=dev(np.array(rows, np.int32)), removed=dev(np.full(R + 1, -7, np.int32)))
    a = NewpointsPruneArgs()
    a.d_res, a.res_bstride, a.d_pts, a.pts_bstride, a.d_gated, a.gated_bstride = d["res"].data_ptr(), n + 2, d["pts"].data_ptr(), n + 3, d["gated"].data_ptr(), n + 1
    a.d_n, a.d_n_new, a.n, a.batch = d["n"].data_ptr(), d["nn"].data_ptr(), n, R
    a.d_store, a.store_bstride, a.d_group_count, a.group_bstride, a.d_n_groups = d["store"].data_ptr(), cap + 2, d["counts"].data_ptr(), GS, d["ng"].data_ptr()
    a.d_stream = d["rows"].data_ptr() if indexed else None
    err = None
    try:
        ctx.call("svs_newpoints_prune", C.byref(a), d["removed"].data_ptr())
    except SvsError as e:
        err = e
    ctx.sync()
    assert (err is not None) == expect_error, err
    h_store = d["store"].cpu().numpy().reshape(S, cap + 2, 64)
    h_counts = d["counts"].cpu().numpy().view(np.int32).reshape(S, GS)
    h_removed = d["removed"].cpu().numpy().view(np.int32)
    if expect_error:
        assert np.array_equal(h_store, before) and np.array_equal(h_counts, counts) and (h_removed == -7).all(), "a refused call wrote"
        return err
    assert h_removed[R] == -7
    out = []
    for i, (r, c) in enumerate(zip(rows, cases)):
        live = int(sum(len(g) for g in c["groups"]))
        assert np.array_equal(h_store[r, live:], before[r, live:]), f"case {i}: wrote behind the stream's records"
        assert (h_counts[r, len(c['groups']):] == -9).all(), f"case {i}: wrote behind the stream's groups"
        cnt = h_counts[r, :len(c["groups"])].copy()
        out.append((int(h_removed[i]), cnt, h_store[r, :int(cnt.sum())].copy().view(CANDIDATE_DTYPE).reshape(-1)))
    for r in set(range(S)) - set(rows):
        assert np.array_equal(h_store[r], before[r]) and np.array_equal(h_counts[r], counts[r]), f"row {r} belongs to no stream of the call"
    return out


def assert_pruned_like_the_model(got, cases, what=""):
    for i, ((n_removed, counts, rec), c) in enumerate(zip(got, cases)):
        s = NM.Store(10 ** 9)
        s.keys, s.groups = list(range(len(c["groups"]))), [g.copy() for g in c["groups"]]
        want_removed, want_counts = s.prune(NM.prune_set(c["res"], c["gated"], c["pts"], c["n_new"]))
        assert n_removed == want_removed and counts.tolist() == want_counts, f"{what} case {i}: removed {n_removed} / {counts} vs the model's {want_removed} / {want_counts}"
        assert rec.tobytes() == s.records().tobytes(), f"{what} case {i}: records differ from the model's"


@pytest.mark.parametrize("sizes", [[63], [64], [65], [255], [256], [257], [63, 64, 65, 255, 256, 257], [100, 0, 300, 0, 0, 41], [30, 70, 1, 27, 513]])
def test_prune_at_the_wave_chunk_and_group_edges(gpu_ctx, sizes):
    """groups that end on, before and behind a wave (64) and a chunk (256), group boundaries inside a wave, empty groups between full ones; P: none of the store,
    all of it, every other record, the first / last record of every group, a random third, and ids the store does not hold"""
    rng = np.random.default_rng(sum(sizes))
    total = sum(sizes)
    cases = []
    for mode in ("none", "all", "alt", "edges", "third", "strangers"):
        groups = make_groups(rng, sizes)
        ids = np.arange(1, total + 1)
        ends = np.cumsum(sizes)
        P = dict(none=[], all=ids, alt=ids[::2], edges=sorted(set(ends[np.array(sizes) > 0]) | set(ends[np.array(sizes) > 0] - np.array(sizes)[np.array(sizes) > 0] + 1)),
                 third=rng.permutation(ids)[:total // 3], strangers=list(ids[:5]) + [900000 + k for k in range(40)])[mode]
        cases.append(step_case(rng, groups, [int(p) for p in rng.permutation(list(P))], n_extra=int(rng.integers(0, 300))))
    got = run_prune(gpu_ctx, cases)
    assert_pruned_like_the_model(got, cases, str(sizes))
    assert got[0][0] == 0 and got[1][0] == total and got[1][1].sum() == 0 and got[5][0] == 5


def test_prune_reads_only_the_new_accepted_matched_records(gpu_ctx):
    rng = np.random.default_rng(3)
    from scavislam_amd.ctypes_types import MATCH_SKIPPED
    assert MATCH_SKIPPED == 7
    cases = []
    # an accepted match at index n_new - 1 prunes, the one at n_new does not: it is no new record
    groups = make_groups(rng, [40, 40])
    c = step_case(rng, groups, [5, 45], n_extra=0, n_new=1)
    assert c["pts"]["point_id"].tolist() == [5, 45]
    cases.append(c)
    cases.append(dict(c, n_new=2))
    cases.append(dict(c, n_new=0))
    cases.append(dict(c, n_new=-3))
    cases.append(dict(c, n_new=1000))                              # above the step's record count: every record is new
    # matched but not accepted; accepted but skipped / not matched
    c = step_case(rng, make_groups(rng, [40, 40]), [5, 45, 46, 47])
    c["gated"]["accepted"][1] = 0
    c["res"]["status"][2] = MATCH_SKIPPED
    c["res"]["status"][3] = 5
    cases.append(c)
    cases.append(step_case(rng, [], [1, 2, 3], n_extra=10))        # a stream with no groups
    cases.append(dict(res=c["res"][:0], gated=c["gated"][:0], pts=c["pts"][:0], n_new=0, groups=make_groups(rng, [10])))      # a step without records
    got = run_prune(gpu_ctx, cases)
    assert_pruned_like_the_model(got, cases, "edges of P")
    assert [g[0] for g in got] == [1, 2, 0, 0, 2, 1, 0, 0]


def test_prune_batch_of_33_equals_each_alone_indexed_and_repeated(gpu_ctx):
    rng = np.random.default_rng(33)
    cases = []
    for b in range(33):
        sizes = [int(s) for s in rng.integers(0, 200, int(rng.integers(0, 8)))]
        groups = make_groups(rng, sizes)
        ids = np.arange(1, sum(sizes) + 1)
        cases.append(step_case(rng, groups, [int(p) for p in rng.permutation(ids)[:len(ids) // 4]], n_extra=int(rng.integers(0, 500))))
    batch = run_prune(gpu_ctx, cases)
    assert_pruned_like_the_model(batch, cases, "batch of 33")
    same = lambda a, b: a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()
    assert all(same(a, b) for a, b in zip(batch, run_prune(gpu_ctx, cases))), "a second run differs"
    assert all(same(a, b) for a, b in zip(batch, run_prune(gpu_ctx, cases, indexed=True))), "streams named through d_stream differ"
    for b in (0, 7, 32):
        assert same(run_prune(gpu_ctx, [cases[b]])[0], batch[b]), f"stream {b} alone differs from its place in the batch"
    # 64 groups is the most a row can hold; a wider table is refused with nothing written
    many = step_case(rng, make_groups(rng, [3] * 64), [1, 4, 190, 192])
    assert_pruned_like_the_model(run_prune(gpu_ctx, [many]), [many], "64 groups")
    err = run_prune(gpu_ctx, [many], expect_error=True, group_stride=65)
    assert "status 4" in str(err)


# ---- the store, through a front end ---------------------------------------------------------------------------------------------------------------------------
def bare_frontend(gpu_ctx, B, max_points=256, max_keyframes=4):
    """a front end that has seen no frame: enough for put / get / drop and for a hand-over without kept slots"""
    import register_model as RM
    from scavislam_amd.frontend import StereoFrontend
    return StereoFrontend(gpu_ctx[0], RM.SMALL_CAM, max_points=max_points, max_keyframes=max_keyframes, n_streams=B)


def assert_stores(fe, models, what=""):
    got = fe.newpoints()
    for b, (g, m) in enumerate(zip(got, models)):
        ng, keys, counts = m.table_rows()
        assert g["raw"] == (ng, keys.tobytes(), counts.tobytes()), f"{what} stream {b}: table {g['keys']} / {g['counts']} vs the model's {m.keys} / {counts[:ng]}"
        assert g["records"].tobytes() == m.records().tobytes(), f"{what} stream {b}: records differ from the model's"


def refused(call, status):
    from scavislam_amd.capi import SvsError
    with pytest.raises(SvsError, match=f"status {status}"):
        call()


def test_put_get_drop_against_the_model(gpu_ctx):
    from scavislam_amd.capi import SvsError
    rng = np.random.default_rng(1)
    fe = bare_frontend(gpu_ctx, 3)
    refused(lambda: fe.putNewpoints([dict(stream=0, kf_id=1)]), 1)                # nothing reserved yet
    fe.reserveNewpoints(400, 64)
    refused(lambda: fe.reserveNewpoints(400, 64), 1)
    models = [NM.Store(400) for _ in range(3)]
    assert_stores(fe, models, "empty")
    rec = lambda n, first: NM.random_records(rng, n, first, kf_index=int(rng.integers(-1, 4)))
    calls = [[dict(stream=0, kf_id=5, records=rec(70, 1)), dict(stream=2, kf_id=9, records=rec(65, 1)), dict(stream=0, kf_id=3, records=rec(130, 100)),
              dict(stream=0, kf_id=8)],                                                                       # an absent key with n = 0 creates its group
             [dict(stream=0, kf_id=3, records=rec(64, 300)), dict(stream=0, kf_id=5, records=rec(1, 400)), dict(stream=0, kf_id=3, records=rec(2, 500))],      # prepend to a middle group, twice in one call
             [dict(stream=0, kf_id=5, records=rec(10, 600), mode=NM.REPLACE), dict(stream=2, kf_id=9, records=rec(0, 0), mode=NM.REPLACE), dict(stream=1, kf_id=0, records=rec(400, 1))],
             [dict(stream=0, kf_id=8, records=rec(3, 700)), dict(stream=0, kf_id=8, records=rec(5, 800), mode=NM.REPLACE), dict(stream=0, kf_id=8, records=rec(4, 900))]]
    for k, call in enumerate(calls):
        fe.putNewpoints(call)
        for b in range(3):
            models[b].put_all([q for q in call if q["stream"] == b])
        assert_stores(fe, models, f"put call {k}")
    assert models[0].keys == [5, 3, 8] and models[1].total() == 400
    # refusals: state unchanged on the device
    for call, status in (([dict(stream=1, kf_id=0, records=rec(1, 5000))], 4), ([dict(stream=1, kf_id=77, records=rec(1, 5000))], 4),
                         ([dict(stream=0, kf_id=5, records=rec(1, 1)), dict(stream=1, kf_id=0, records=rec(1, 5000))], 4),      # the whole call: stream 0 stays too
                         ([dict(stream=3, kf_id=1)], 1), ([dict(stream=0, kf_id=-1)], 1), ([dict(stream=0, kf_id=1, mode=2)], 1)):
        refused(lambda: fe.putNewpoints(call), status)
        assert_stores(fe, models, "after a refusal")
    # drop: named groups go, the others keep their order; absent and repeated keys
    found = fe.dropNewpointGroups([dict(stream=0, keys=[3, 44, 3]), dict(stream=2, keys=[]), dict(stream=0, keys=[3])])
    assert found == [models[0].drop([3, 44, 3]), models[2].drop([]), models[0].drop([3])] == [1, 0, 0]
    assert_stores(fe, models, "drop")
    back = rec(7, 1000)
    fe.putNewpoints([dict(stream=0, kf_id=3, records=back)])                      # a dropped key comes back at the END
    models[0].put(3, back)
    assert models[0].keys == [5, 8, 3]
    assert_stores(fe, models, "put behind a drop")
    fe.close()


def test_the_64th_and_65th_group_and_a_full_store(gpu_ctx):
    rng = np.random.default_rng(2)
    fe = bare_frontend(gpu_ctx, 2)
    fe.reserveNewpoints(130, 64)
    models = [NM.Store(130), NM.Store(130)]
    call = [dict(stream=1, kf_id=1000 - k, records=NM.random_records(rng, 2, 10 * k)) for k in range(64)]
    fe.putNewpoints(call)
    models[1].put_all(call)
    assert_stores(fe, models, "64 groups")
    refused(lambda: fe.putNewpoints([dict(stream=1, kf_id=5)]), 4)                # the 65th
    assert_stores(fe, models, "65th group refused")
    two = NM.random_records(rng, 2, 5000)
    fe.putNewpoints([dict(stream=1, kf_id=1000, records=two)])                    # 128 + 2 = record_cap exactly
    models[1].put(1000, two)
    assert models[1].total() == 130
    assert_stores(fe, models, "exactly full")
    refused(lambda: fe.putNewpoints([dict(stream=1, kf_id=999, records=NM.random_records(rng, 1, 6000))]), 4)      # one over
    assert_stores(fe, models, "one over refused")
    assert fe.dropNewpointGroups([dict(stream=1, keys=list(range(937, 1000)))]) == [63]
    models[1].drop(list(range(937, 1000)))
    assert_stores(fe, models, "63 groups dropped")
    # a smaller group_cap is held too
    fe2 = bare_frontend(gpu_ctx, 1)
    refused(lambda: fe2.reserveNewpoints(10, 65), 1)
    fe2.reserveNewpoints(10, 2)
    fe2.putNewpoints([dict(kf_id=1), dict(kf_id=2)])
    refused(lambda: fe2.putNewpoints([dict(kf_id=3)]), 4)
    fe2.close()
    fe.close()


def test_hand_over_without_slots_batch_of_33(gpu_ctx):
    """33 streams in one call against the model of each, one of them alone, and a repetition; absent keys, key order, max_points exactly full and one over"""
    rng = np.random.default_rng(4)
    B, MP = 33, 256
    fe = bare_frontend(gpu_ctx, B, max_points=MP)
    fe.reserveNewpoints(500, 8)
    models = [NM.Store(500, 8) for _ in range(B)]
    puts = []
    for b in range(B):
        for k in rng.permutation(6)[:int(rng.integers(1, 6))]:
            puts.append(dict(stream=b, kf_id=int(k), records=NM.random_records(rng, int(rng.integers(0, 40)), 1000 * int(k), kf_index=3)))
    puts += [dict(stream=31, kf_id=7, records=NM.random_records(rng, 200, 50000, kf_index=2)), dict(stream=32, kf_id=7, records=NM.random_records(rng, 200, 50000, kf_index=2))]
    fe.putNewpoints(puts)
    for b in range(B):
        models[b].put_all([q for q in puts if q["stream"] == b])
    slot = [-1] * 4
    reqs = []
    for b in range(B):
        keys = [int(k) for k in rng.permutation(8)[:int(rng.integers(1, 8))]]      # 6 and (mostly) 7 are absent keys
        reqs.append(dict(stream=b, keys=keys, slot_kf=slot, tail=NM.random_records(rng, int(rng.integers(0, 40)), 90000, kf_index=-1)))
    reqs[31].update(keys=[7], tail=NM.random_records(rng, 56, 90000, kf_index=-1))      # 200 + 56 = max_points
    reqs[32].update(keys=[7], tail=NM.random_records(rng, 57, 90000, kf_index=-1))      # one over
    order = [int(r) for r in rng.permutation(B)]                                        # the place in the batch is not the stream
    first = fe.setCandidatesFromNewpoints([reqs[r] for r in order], want_records=True)
    table, ends = first[0]["table"].copy(), first[0]["group_end"].copy()
    want_len = [0] * B
    for o, r in zip(first, order):
        q = reqs[r]
        rec, ge, res = models[r].compose(q["keys"], q["slot_kf"], q["tail"], MP)
        assert {k: o[k] for k in res} == res, f"stream {r}: {o} vs the model's {res}"
        if res["over_capacity"]:
            assert r == 32 and (table[r].view(np.uint8) == 0xFF).all() and fe.n_points[r] == 0      # the stream is untouched
            continue
        want_len[r] = len(rec)
        assert table[r, :len(rec)].tobytes() == rec.tobytes(), f"stream {r}: the list differs from the model's"
        assert (table[r, len(rec):].view(np.uint8) == 0xFF).all(), f"stream {r}: no 0xff tail"
        assert ends[r, :len(ge)].tolist() == ge and (ends[r, len(ge):] == 0).all(), f"stream {r}: group ends {ends[r, :len(ge)]} vs {ge}"
        assert (rec["kf_index"][:res["n_head"]] == -1).all() and fe.n_points[r] == len(rec)
    assert first[order.index(31)]["n_points"] == MP
    again = fe.setCandidatesFromNewpoints(reqs, want_records=True)                        # stream order this time
    assert again[0]["table"].tobytes() == table.tobytes() and again[0]["group_end"].tobytes() == ends.tobytes(), "a second run differs"
    # one stream alone, with a shorter list: the records behind it become 0xff, the others stay
    short = dict(reqs[5], keys=reqs[5]["keys"][:1], tail=reqs[5]["tail"][:1])
    alone = fe.setCandidatesFromNewpoints([short], want_records=True)[0]
    rec, ge, res = models[5].compose(short["keys"], slot, short["tail"], MP)
    assert alone["table"][5, :len(rec)].tobytes() == rec.tobytes() and (alone["table"][5, len(rec):].view(np.uint8) == 0xFF).all()
    keep = [b for b in range(B) if b != 5]
    assert alone["table"][keep].tobytes() == table[keep].tobytes() and alone["group_end"][keep].tobytes() == ends[keep].tobytes()
    assert_stores(fe, models, "the hand-over changes no store")
    # streams alone, each with its own unchanged request, on a fresh front end that holds only that stream's store: the bytes of its place in the batch
    for b in (0, 13, 31, 32):
        one = bare_frontend(gpu_ctx, 1, max_points=MP)
        one.reserveNewpoints(500, 8)
        one.putNewpoints([dict(q, stream=0) for q in puts if q["stream"] == b])
        o = one.setCandidatesFromNewpoints([dict(reqs[b], stream=0)], want_records=True)[0]
        assert {k: o[k] for k in NM_RESULT} == {k: first[order.index(b)][k] for k in NM_RESULT}, f"stream {b} alone: result"
        assert o["table"][0].tobytes() == table[b].tobytes(), f"stream {b} alone differs from its place in the batch"
        if not o["over_capacity"]:
            assert o["group_end"][0].tobytes() == ends[b].tobytes(), f"stream {b} alone: group ends"
        one.close()
    # refusals, nothing uploaded: a key twice, no key, a negative key, a stream twice, a slot that was never kept
    for bad in ([dict(reqs[0], keys=[1, 2, 1])], [dict(reqs[0], keys=[])], [dict(reqs[0], keys=[-1])], [reqs[0], reqs[0]], [dict(reqs[0], slot_kf=[3, -1, -1, -1])]):
        refused(lambda: fe.setCandidatesFromNewpoints(bad), 1)
    refused(lambda: fe.setCandidatesFromNewpoints([dict(reqs[0], keys=list(range(64)))]), 4)
    after = fe.setCandidatesFromNewpoints([], want_records=True)
    assert after == []
    fe.close()


def test_a_staging_block_that_grows_in_mid_life_batch_of_33(gpu_ctx):
    """putNewpoints, newpoints and setCandidatesFromNewpoints with one request, then 33, then one again, on ONE front end: the staging block starts at twice the first
    call's need, so the 33 outgrow it and the third call reuses the bigger block.  Every store against the model; the rows a call names against a fresh front end
    that makes only that call (a hand-over: behind one put of the same stores)"""
    rng = np.random.default_rng(6)
    B, MP = 33, 256
    rec = lambda n, first, kf=3: NM.random_records(rng, n, first, kf_index=kf)
    put33 = [dict(stream=b, kf_id=3, records=rec(int(rng.integers(1, 40)), 1000 * b), mode=NM.REPLACE) for b in range(B)]
    put33 += [dict(stream=b, kf_id=int(k), records=rec(int(rng.integers(0, 40)), 100000 + 1000 * b + 100 * int(k))) for b in range(2, B) for k in rng.permutation([0, 1, 2])[:b % 3]]
    puts = [[dict(stream=0, kf_id=3, records=rec(5, 70000), mode=NM.REPLACE)], put33, [dict(stream=1, kf_id=3, records=rec(9, 80000), mode=NM.REPLACE)]]
    slot = [-1] * 4
    reqs = [dict(stream=b, keys=[int(k) for k in rng.permutation(5)[:int(rng.integers(1, 5))]], slot_kf=slot, tail=rec(int(rng.integers(0, 40)), 90000, kf=-1)) for b in range(B)]
    lists = [[reqs[0]], [reqs[int(r)] for r in rng.permutation(B)], [reqs[1]]]

    def fresh():
        fe = bare_frontend(gpu_ctx, B, max_points=MP)
        fe.reserveNewpoints(500, 8)
        return fe

    def stores(fe, call):
        got = fe.newpoints()
        return [(got[b]["raw"], got[b]["records"].tobytes()) for b in sorted({q["stream"] for q in call})]

    def handed(fe, call):
        outs = fe.setCandidatesFromNewpoints(call, want_records=True)
        return [({k: o[k] for k in NM_RESULT}, outs[0]["table"][q["stream"]].tobytes(), outs[0]["group_end"][q["stream"]].tobytes()) for o, q in zip(outs, call)]

    fe = fresh()
    models = [NM.Store(500, 8) for _ in range(B)]
    got_put, got_list = [], []
    for k, call in enumerate(puts):
        fe.putNewpoints(call)
        for b in range(B):
            models[b].put_all([q for q in call if q["stream"] == b])
        assert_stores(fe, models, f"put call {k}")
        got_put.append(stores(fe, call))
    for call in lists:
        got_list.append(handed(fe, call))
        for (res, row, _), q in zip(got_list[-1], call):
            want, ge, want_res = models[q["stream"]].compose(q["keys"], slot, q["tail"], MP)
            assert res == want_res and not res["over_capacity"] and row[:want.nbytes] == want.tobytes() and set(row[want.nbytes:]) <= {0xFF}, f"stream {q['stream']}"
    assert_stores(fe, models, "the hand-over changes no store")
    fe.close()
    final = [q for q in put33 if q["stream"] != 1] + puts[2]          # one call that leaves every stream's store as the three left it
    for call, g in zip(puts, got_put):
        one = fresh()
        one.putNewpoints(call)
        assert stores(one, call) == g, f"putNewpoints, {len(call)} request(s)"
        one.close()
    for call, g in zip(lists, got_list):
        one = fresh()
        one.putNewpoints(final)
        assert handed(one, call) == g, f"setCandidatesFromNewpoints, {len(call)} request(s)"
        one.close()


# ---- seeding, pruning and the hand-over on a front end that tracks -----------------------------------------------------------------------------------------------
def tracking_frontend(gpu_ctx, B=2):
    import test_gpu_seed as TS
    fe, cam, keep = TS.frontend_after_first_frames(gpu_ctx, "default", B=B)
    fe.reserveNewpoints(1090, 8)
    return fe, cam, keep


def step(gpu_ctx, fe, B, frame=1):
    import torch
    import seed_common as S
    import seq_common
    from scavislam_amd import synth
    traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)
    img, disp = S.frame("default", frame)
    with torch.cuda.stream(gpu_ctx[1]):
        left = torch.as_tensor(np.stack([img] * B)).cuda()
        dd = torch.as_tensor(np.stack([disp] * B).astype(np.float32)).cuda()
    fe.processFrames(np.stack([I34.reshape(12)] * B), np.stack([traj[0].reshape(12)] * B), left=left, disp=dd)
    return [fe.results(b) for b in range(B)]


def test_seed_prune_and_hand_over_on_a_tracking_front_end(gpu_ctx):
    """one drop cycle and a half on two streams: seed (first) into the store = seedKeyframes' download; hand-over with the slot rewrite; a step; the front end's
    prune = the model on the downloaded records; seed (more) on top, two requests for one stream; the SVS_SEED_MORE refusal; a twin fed from the host tracks the same"""
    import seq_common
    import test_gpu_seed as TS
    from scavislam_amd import synth
    from scavislam_amd.ctypes_types import SEED_FIRST, SEED_MORE
    B = 2
    fe, cam, keep = tracking_frontend(gpu_ctx, B)
    traj = synth.trajectory_there_and_back(seq_common.N_FRAMES, seq_common.TURN)
    models = [NM.Store(1090, 8) for _ in range(B)]
    rng = np.random.default_rng(8)
    reqs = [dict(stream=0, mode=SEED_FIRST, kf_index=0, first_point_id=1, seed=5, kf_id=20), dict(stream=1, mode=SEED_FIRST, kf_index=0, first_point_id=1, seed=6, kf_id=10)]
    host = fe.seedKeyframes(reqs)
    old = [host[b][0][:520:13].copy() for b in range(B)]           # 40 points a keyframe seeded earlier: real positions, ids of their own
    for o in old:
        o["point_id"] += 9000
    fe.putNewpoints([dict(stream=b, kf_id=20, records=old[b]) for b in range(B)])
    for b in range(B):
        models[b].put(20, old[b])
    refused(lambda: fe.pruneNewpoints(), 1)                        # no step yet
    # SVS_SEED_FIRST: the records seedKeyframes downloads, prepended to an existing group (stream 0) and into a new one (stream 1)
    dev = fe.seedNewpoints(reqs, want_records=True)
    for r in range(2):
        assert np.array_equal(dev[r][1], host[r][1]) and dev[r][0].tobytes() == host[r][0].tobytes() and len(host[r][0]) == 528
        models[r].put(reqs[r]["kf_id"], host[r][0])
    assert_stores(fe, models, "seed first")
    refused(lambda: fe.seedNewpoints([dict(reqs[0], kf_id=21)]), 4)               # 568 + the most a request can produce (528) = 1096 > 1090: nothing seeded
    refused(lambda: fe.seedNewpoints([dict(reqs[0], kf_id=-2)]), 1)
    assert_stores(fe, models, "refused seeds")
    # hand-over: group order as named, an absent key, the kept slot's index written into the head, a key without a slot
    fe.keepKeyframes(1, np.stack([traj[0].reshape(12)] * B))
    tail = [NM.random_records(rng, 5, 70000, kf_index=-1), NM.random_records(rng, 0, 0)]
    lists = [dict(stream=0, keys=[20, 33], slot_kf=[-1, 20], tail=tail[0]), dict(stream=1, keys=[33, 10, 20], slot_kf=[-1, 10], tail=tail[1])]
    refused(lambda: fe.setCandidatesFromNewpoints([dict(lists[0], slot_kf=[20, -1])]), 1)      # slot 0 was never kept
    refused(lambda: fe.setCandidatesFromNewpoints([dict(lists[0], tail=NM.random_records(rng, 2, 1, kf_index=0))]), 1)      # ... nor may a tail record name it
    got = fe.setCandidatesFromNewpoints(lists, want_records=True)
    want = [models[b].compose(lists[b]["keys"], lists[b]["slot_kf"], lists[b]["tail"], fe.max_points) for b in range(B)]
    for b in range(B):
        rec, ge, res = want[b]
        assert {k: got[b][k] for k in res} == res
        assert got[b]["table"][b, :len(rec)].tobytes() == rec.tobytes() and got[b]["group_end"][b, :len(ge)].tolist() == ge
    assert want[0][2]["n_no_slot"] == 0 and want[1][2]["n_no_slot"] == 40 and (want[0][0]["kf_index"][:568] == 1).all()
    # a step; a twin front end fed the model's lists from the host returns the same records
    res = step(gpu_ctx, fe, B)
    tfe, _, _ = TS.frontend_after_first_frames(gpu_ctx, "default", B=B)
    tfe.keepKeyframes(1, np.stack([traj[0].reshape(12)] * B))
    for b in range(B):
        ge = want[b][1]
        tfe.setCandidateLists(want[b][0], ge if len(ge) >= 2 else [ge[0], ge[0]], stream=b)
    tres = step(gpu_ctx, tfe, B)
    for b in range(B):
        assert bytes(res[b][0]) == bytes(tres[b][0]) and res[b][1].tobytes() == tres[b][1].tobytes() and res[b][2].tobytes() == tres[b][2].tobytes(), f"stream {b}: the twin tracks differently"
        assert (res[b][1]["status"] == 0).sum() > 100
    tfe.close()
    # the front end's prune = the stateless svs_newpoints_prune on the downloaded records and the store's read-back, and both = the model
    stateless = run_prune(gpu_ctx, [dict(res=res[b][1], gated=res[b][2], pts=want[b][0], n_new=want[b][2]["n_head"], groups=[g.copy() for g in models[b].groups])
                                    for b in range(B)])
    pruned = fe.pruneNewpoints([1, 0])
    for (n_removed, counts), b in zip(pruned, (1, 0)):
        _, m, g = res[b]
        P = NM.prune_set(m, g, want[b][0], want[b][2]["n_head"])
        want_removed, want_counts = models[b].prune(P)
        assert n_removed == want_removed == len(P) > 100 and counts[:len(want_counts)].tolist() == want_counts and (counts[len(want_counts):] == 0).all()
        assert stateless[b][0] == n_removed and stateless[b][1].tolist() == want_counts, f"stream {b}: the stateless prune counts differently"
        assert stateless[b][2].tobytes() == fe.newpoints([b])[0]["records"].tobytes(), f"stream {b}: the stateless prune leaves other records"
    assert_stores(fe, models, "prune")
    assert fe.pruneNewpoints([0])[0][0] == 0                       # again: nothing left to remove
    # SVS_SEED_MORE behind the step, two requests for one stream (in request order) and one for the other
    T = np.hstack([np.array([[0.999, -0.04, 0.0], [0.04, 0.999, 0.01], [0.0, -0.01, 1.0]]), [[0.1], [-0.2], [0.05]]])
    fe.dropNewpointGroups([dict(stream=0, keys=[20])])
    models[0].drop([20])
    more = [dict(stream=1, mode=SEED_MORE, kf_index=1, first_point_id=4000, seed=900, T_newkey_from_cur=T, kf_id=10),
            dict(stream=0, mode=SEED_MORE, kf_index=1, first_point_id=5000, seed=901, kf_id=30),
            dict(stream=0, mode=SEED_FIRST, kf_index=0, first_point_id=6000, seed=902, kf_id=30)]
    host = fe.seedKeyframes(more)
    counts = fe.seedNewpoints(more)
    for r, q in enumerate(more):
        assert np.array_equal(counts[r], host[r][1])
        models[q["stream"]].put(q["kf_id"], host[r][0])
    assert len(host[2][0]) == 528
    assert_stores(fe, models, "seed more")
    # the list is replaced: the step's records are no longer this list's -- prune and SVS_SEED_MORE are refused, the stores stay
    fe.setCandidatesFromNewpoints([dict(stream=0, keys=[30], slot_kf=[-1, -1])])
    refused(lambda: fe.pruneNewpoints([0]), 1)
    refused(lambda: fe.seedNewpoints(more[:1]), 1)
    refused(lambda: fe.pruneNewpoints([0, 0]), 1)
    assert_stores(fe, models, "refused behind a new list")
    fe.close()


def test_cpp_adaptor_keeps_newpoint_map_on_the_device(gpu_ctx, tmp_path):
    """tests/cpp/newpoints_smoke.cpp: the resident newpoint_map of include/scavislam_hip.hpp's StereoFrontend, compiled with g++ -std=c++11, against the same
    front end fed from the host"""
    exe = tmp_path / "newpoints_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "newpoints_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("NEWPOINTS ")]
    assert tok and tok[0].split()[1] == "ok", out
    assert int(tok[0].split()[2]) > 100
