"""The memory pipeline of the dense tracker's sample loop, read off the gfx950 assembly (tools/tracker_loop_isa.py; no GPU needed).

A sample's 4 x 4 neighbourhood is four row loads.  The compiler once issued row 0, waited for it, and only then issued rows 1..3 -- two dependent memory
round trips per sample in the kernels the big batches run -- and nothing in the results could show it.  This holds the two hot instantiations of the
flat tracker kernel to one round trip and to the register budget they are built for."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("tracker_loop_isa", os.path.join(ROOT, "tools", "tracker_loop_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

# scratch bytes per lane of the two kernels before the tap loads were taken out of the compiler's hands: the change may not buy its order with spills
SCRATCH_BEFORE = {"dense_track_batch_kernel<true, true, 0>": 16, "dense_track_batch_kernel<true, false, 1>": 64}


@pytest.fixture(scope="module")
def records():
    if isa.find_hipcc() is None:
        pytest.skip("no hipcc")
    return {r["name"]: r for r in isa.run()}


@pytest.mark.parametrize("name", isa.HOT)
def test_hot_tracker_kernel_fetches_the_taps_in_one_round_trip(records, name):
    assert name in records, "no sample loop found in %s" % name
    r = records[name]
    print(name, {k: r[k] for k in ("vgpr", "scratch", "occupancy")}, [{k: l[k] for k in ("instructions", "classes", "memory_order", "first_wait", "between_issue_and_wait")} for l in r["loops"]])
    assert r["loops"]
    for l in r["loops"]:
        assert l["tap_loads"] == 4, "a trip handles one sample: four row loads"
        assert l["taps_before_wait"] == 4 and l["verdict"], "a wait covers a tap load before all four are issued: " + " -> ".join(l["memory_order"])
        assert l["dest_untouched"], "something reads or writes a tap load's destination between its issue and the wait"
        assert l["scratch_in_loop"] == 0, "scratch access inside the sample loop"
    assert r["vgpr"] <= 128 and r["occupancy"] == 4
    assert r["scratch"] <= SCRATCH_BEFORE[name]


def test_every_u8_sweep_issues_its_taps_together(records):
    # the other functions that inline the sweep (latency-mode kernels, the sweep as a call): the same order, without the register limits of the hot two
    u8 = [r for r in records.values() for l in r["loops"] if l["tap_loads"]]
    assert len(u8) >= 4
    for r in u8:
        for l in r["loops"]:
            assert l["verdict"] and l["dest_untouched"], r["name"] + ": " + " -> ".join(l["memory_order"])
