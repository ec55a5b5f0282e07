"""The prefetch of the dense tracker's sample loop, read off the gfx950 assembly (tools/tracker_loop_isa.py; no GPU needed).

A trip of the sweep issues the term store of the sample before and the loads of the NEXT sample's cloud point and previous-frame byte, projects the current
sample, and then issues its four tap loads.  vmcnt counts loads and stores in one queue: a `s_waitcnt vmcnt(N)` between those requests and the taps makes all but
the N youngest of them complete before the taps go out -- two memory round trips per trip, one after the other, and nothing in the results shows it.  The compiler
placed such a wait (vmcnt(1) behind three requests) as long as the taps' own wait was an inline-asm statement it could not see (profiles/tracker_prefetch.md).
This holds the four u8 kernels that run in practice to "no wait in front of the taps forces a request of its own trip", and the two hot ones to their registers."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("tracker_loop_isa", os.path.join(ROOT, "tools", "tracker_loop_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

U8_IN_PRACTICE = isa.HOT + ("dense_track_cpu_sem_kernel<true, false, false>", "dense_track_cpu_sem_kernel<true, true, false>")
SCRATCH_BAR = {"dense_track_batch_kernel<true, true, 0>": 16, "dense_track_batch_kernel<true, false, 1>": 64}


@pytest.fixture(scope="module")
def records():
    if isa.find_hipcc() is None:
        pytest.skip("no hipcc")
    return {r["name"]: r for r in isa.run()}


@pytest.mark.parametrize("name", U8_IN_PRACTICE)
def test_no_wait_in_front_of_the_taps_forces_the_trips_own_requests(records, name):
    assert name in records, "no sample loop found in %s" % name
    r = records[name]
    print(name, [(l["memory_order"], l["prefetch_waits"]) for l in r["loops"]])
    assert r["loops"]
    for l in r["loops"]:
        assert l["tap_loads"] == 4
        assert l["prefetch_verdict"] and l["prefetch_forced"] == 0, "a wait in front of the taps completes requests of its own trip: " + " -> ".join(l["memory_order"])
        # the one wait of a trip that covers memory is the taps' own, and it covers everything older
        assert l["verdict"] and l["first_wait"] == "vmcnt(0)", " -> ".join(l["memory_order"])
    assert r["prefetch_verdict"]


@pytest.mark.parametrize("name", isa.HOT)
def test_hot_kernels_keep_their_registers(records, name):
    r = records[name]
    print(name, {k: r[k] for k in ("vgpr", "scratch", "occupancy")})
    assert r["vgpr"] <= 128 and r["occupancy"] == 4
    assert r["scratch"] <= SCRATCH_BAR[name]
    assert all(l["scratch_in_loop"] == 0 for l in r["loops"])
