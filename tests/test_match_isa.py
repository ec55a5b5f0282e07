"""match_kernel3 as the compiler made it, read off the gfx950 assembly (tools/match_isa.py; no GPU needed).

The kernel asks for the pixel rows of a point's first hits in stage (3b) so that their round trip runs under the f64 arithmetic of stage (4), and for the
eight rows of a later trip of stage (5) in one go.  Neither shows in the results when it is lost: a flat load counts on lgkmcnt too, so every wait for the LDS
waits for the rows; a record re-read with a vector load behind the rows makes the arithmetic's own wait force them (vmcnt retires in order); one loop body for
the first and the later trips made the later ones wait for each of their first four rows (profiles/match_isa.md has the assembly of both sides).  The same
for the quarter-rate multiplies in the address arithmetic, which svs_match's 24-bit refusal exists to avoid."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("match_isa", os.path.join(ROOT, "tools", "match_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


@pytest.fixture(scope="module")
def rec():
    if isa.T.find_hipcc() is None:
        pytest.skip("no hipcc")
    r = isa.run()
    print(isa.render(r, "match_kernel3"))
    return r


def test_no_flat_instruction(rec):
    assert rec["flat"] == 0, rec["flat_ops"]


def test_rows_of_3b_fly_under_stage_4(rec):
    p = rec["prefetch"]
    assert p["rows"] >= 4 and p["f64"] >= 100, (p["rows"], p["f64"])      # the landmarks were found: the M3_PRE row requests, the bilinear arithmetic of four samples
    for w in p["waits"]:
        assert w["forced"] == 0, "a wait between the first row request of (3b) and the last f64 instruction of (4) covers a row: %r" % (w,)
    assert p["verdict"]


def test_later_trips_request_their_rows_before_the_one_wait(rec):
    lt = rec["later_trips"]
    assert lt is not None, "no loop with eight row requests and the dot products"
    assert lt["rows"] == 8 and lt["rows_before_wait"] == 8 and lt["verdict"], " -> ".join(lt["memory_order"])


def test_quarter_rate_multiplies_only_in_byte_path_and_quad_less(rec):
    print({k: v for k, v in rec["multiplies"].items()})
    for name, m in rec["multiplies"].items():
        assert m["common_path"] == 0, (name, m)


def test_resources(rec):
    print({k: rec[k] for k in ("vgpr", "sgpr", "scratch", "lds", "occupancy")})
    assert rec["vgpr"] <= 64 and rec["scratch"] == 0 and rec["lds"] <= 16384 and rec["occupancy"] == 8
