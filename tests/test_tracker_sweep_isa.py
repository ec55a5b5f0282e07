"""The dense tracker's sample loop after its instruction diet, read off the gfx950 assembly (tools/tracker_loop_isa.py; no GPU needed; profiles/tracker_sweep.md).

The loop ran 216 vector-ALU instructions per sample, 23 of them for nothing: 12 selects that zeroed an invalid sample's contribution (now skipped under one
`if (ok)`), 6 moves for the constants of an out-of-range prefetch (it reads the level's first sample now), 5 moves that copied the prefetched sample into the
current one (two trips per iteration on alternating register sets now).  216 - 23 = 193, and 5 are left to the register allocator: at most 198 per processed
sample in the two hot kernels -- for the two-trip loop the loop's count over two.  The tap and wait verdicts of the earlier changes hold in EACH trip of the
loop, and the kernels keep their registers, scratch and occupancy."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("tracker_loop_isa", os.path.join(ROOT, "tools", "tracker_loop_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

U8_WITH_A_SAMPLE_LOOP = isa.HOT + ("dense_track_cpu_sem_kernel<true, false, false>", "dense_track_cpu_sem_kernel<true, true, false>")
VALU_PER_SAMPLE_BAR = 198
SCRATCH_BAR = {"dense_track_batch_kernel<true, true, 0>": 16, "dense_track_batch_kernel<true, false, 1>": 64}
# waves per SIMD of every tracker instantiation before this change (profiles/kernel_resources.md): none may lose occupancy
OCCUPANCY_BEFORE = {
    "dense_track_batch_kernel<true, true, 0>": 4, "dense_track_batch_kernel<true, false, 1>": 4, "dense_track_batch_kernel<true, false, 0>": 4,
    "dense_track_batch_kernel<false, true, 0>": 4, "dense_track_batch_kernel<false, false, 0>": 4, "dense_track_batch_kernel<false, false, 1>": 4,
    "dense_track_cpu_sem_kernel<true, false, false>": 2, "dense_track_cpu_sem_kernel<true, false, true>": 2, "dense_track_cpu_sem_kernel<true, true, false>": 2,
    "dense_track_cpu_sem_kernel<false, false, false>": 2, "dense_track_cpu_sem_kernel<false, false, true>": 2, "dense_track_cpu_sem_kernel<false, true, false>": 2,
}


@pytest.fixture(scope="module")
def records():
    if isa.find_hipcc() is None:
        pytest.skip("no hipcc")
    return {r["name"]: r for r in isa.run()}


@pytest.mark.parametrize("name", isa.HOT)
def test_valu_per_sample_in_the_hot_kernels(records, name):
    r = records[name]
    assert r["loops"]
    for l in r["loops"]:
        print(name, l["header"], "samples per iteration", l["samples_in_loop"], "VALU of the loop", l["loop_valu"], "per sample", l["valu_per_sample"], l["classes"])
        assert l["samples_in_loop"] * 4 == sum(x["tap_loads"] for x in r["loops"] if x["header"].split(",")[0] == l["header"].split(",")[0])
        assert l["valu_per_sample"] <= VALU_PER_SAMPLE_BAR


def test_the_tool_counts_the_parents_loop_as_the_issue_does():
    """the counting itself, on a loop written out here: one sample (one f64 reciprocal), 3 vector-ALU instructions, scalar and memory instructions not counted"""
    loop = ["global_load_dwordx4 v[4:7], v[4:5], off", "v_rcp_f64_e32 v[0:1], v[2:3]", "v_mov_b32_e32 v0, v4", "s_add_u32 s4, s33, s12", "v_add_u32_e32 v1, v2, v3",
            "s_waitcnt vmcnt(0)", "ds_read_b32 v96, v76"]
    a = isa.analyse_loop(loop)
    assert sum(a["classes"][c] for c in isa.VALU_CLASSES) == 3
    two = ["global_load_dword v1, v0, s[0:1]"] * 4 + ["s_waitcnt vmcnt(0)", "v_rcp_f64_e32 v[0:1], v[2:3]", "global_load_ubyte v9, v8, s[2:3]"] \
        + ["global_load_dword v1, v0, s[0:1]"] * 4 + ["s_waitcnt vmcnt(0)", "v_rcp_f64_e32 v[0:1], v[2:3]"]
    trips = isa.split_trips(two)
    assert [sum(1 for s in t if isa.is_tap_load(s)) for t in trips] == [4, 4] and sum(len(t) for t in trips) == len(two)
    assert trips[1][0].startswith("global_load_ubyte")      # a trip begins with its first memory request


@pytest.mark.parametrize("name", U8_WITH_A_SAMPLE_LOOP)
def test_tap_and_wait_verdicts_hold_in_every_trip(records, name):
    assert name in records, "no sample loop found in %s" % name
    r = records[name]
    print(name, [(l["header"], l["memory_order"], l["prefetch_waits"]) for l in r["loops"]])
    assert r["loops"]
    for l in r["loops"]:
        assert l["tap_loads"] == 4 and l["taps_before_wait"] == 4 and l["verdict"], "a wait covers a tap load before all four are issued: " + " -> ".join(l["memory_order"])
        assert l["first_wait"] == "vmcnt(0)" and l["dest_untouched"]
        assert l["prefetch_verdict"] and l["prefetch_forced"] == 0, "a wait in front of the taps completes requests of its own trip: " + " -> ".join(l["memory_order"])
        assert l["scratch_in_loop"] == 0
    assert r["verdict"] and r["prefetch_verdict"]


@pytest.mark.parametrize("name", isa.HOT)
def test_hot_kernels_keep_registers_scratch_and_occupancy(records, name):
    r = records[name]
    print(name, {k: r[k] for k in ("vgpr", "scratch", "occupancy", "lds")})
    assert r["vgpr"] <= 128 and r["occupancy"] == 4
    assert r["scratch"] <= SCRATCH_BAR[name]
    assert all(l["scratch_in_loop"] == 0 for l in r["loops"])
    # (the accumulators stay in registers -- stage B of the plan, accumulators in LDS, is not part of the kernels: see profiles/tracker_sweep.md --, so the flat
    # kernels' LDS stays far below the 80 KB at which a CU still takes two workgroups)
    assert r["lds"] is not None and 2 * r["lds"] <= 160 * 1024


def test_no_tracker_instantiation_loses_occupancy(records):
    kernels = {n: r for n, r in records.items() if not n.endswith(":: lambda")}
    print({n: (r["vgpr"], r["scratch"], r["occupancy"]) for n, r in kernels.items()})
    assert set(OCCUPANCY_BEFORE) <= set(kernels), set(OCCUPANCY_BEFORE) - set(kernels)
    for n, occ in OCCUPANCY_BEFORE.items():
        assert kernels[n]["occupancy"] >= occ, (n, kernels[n]["occupancy"], occ)
