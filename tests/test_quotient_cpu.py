"""scavislam_amd/csrc/devutil.h: rcp_rn / div_rn (one refined reciprocal, a three-instruction quotient per numerator) and their guarded forms, which the dense
clouds, processMatchedPoints' gate and gate.h's residual divide with, must give the bits of the plain division a / b.  The header is compiled for the host
(tests/cpp/quotient_host.cpp, -ffp-contract=off; the device's v_rcp_f64 is stood in for by 1 / b cut to 24 bits) and driven with random operands, the clouds'
own ranges and hostile ones.

What holds, and is asserted here:
  * div_rn(a, b, RN(1 / b)) == a / b wherever nothing overflows or underflows (Markstein's theorem);
  * two Newton steps from a 24-bit seed give RN(1 / b) -- for every operand tried EXCEPT a mantissa of all ones (b = 2^k (2 - 2^-52): 1 / b lies 2^-107 above
    a rounding midpoint, the iteration lands on the midpoint and the tie goes to the even neighbour below).  That is a fact about the iteration, not a defect of the
    code under test; the test pins it (rcp_rn returns exactly the neighbour below) and holds the guarded forms to a / b there;
  * rcp_rn_checked never accepts a reciprocal that is not RN(1 / b), and accepts nearly all;
  * the guarded forms equal a / b for EVERY pair: zeros of either sign, subnormals, huge values, infinities, NaN, operands just inside and outside the window."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from quotient_pools import (SPECIAL, WINDOW_HI, WINDOW_LO, _cloud_operands, _f64, _hostile_mantissas, _random_mantissa, _with_exponents, all_ones, subnormals,
                            window_edge_values)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 3_000_000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("quotient") / "libquotient_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "quotient_host.cpp"), "-o", str(out)])
    L = C.CDLL(str(out))
    P, LP = C.c_void_p, C.POINTER(C.c_long)
    L.svs_host_div_rn_exact_rcp.restype = C.c_long
    L.svs_host_div_rn_exact_rcp.argtypes = [P, P, C.c_long, LP]
    L.svs_host_rcp_rn.restype = C.c_long
    L.svs_host_rcp_rn.argtypes = [P, C.c_long, LP, P]
    L.svs_host_rcp_seed_error.restype = C.c_double
    L.svs_host_rcp_seed_error.argtypes = [P, C.c_long]
    L.svs_host_rcp_checked.restype = C.c_long
    L.svs_host_rcp_checked.argtypes = [P, C.c_long, LP, LP]
    L.svs_host_div_guarded.restype = C.c_long
    L.svs_host_div_guarded.argtypes = [P, P, C.c_long, LP, LP]
    L.svs_host_quot_exp_ok.restype = C.c_int
    L.svs_host_quot_exp_ok.argtypes = [C.c_double]
    return L


def _check(fn, *arrays, extra=()):
    arrays = [np.ascontiguousarray(a, np.float64) for a in arrays]
    first = C.c_long(-1)
    outs = [C.c_long(0) for _ in extra]
    miss = fn(*[a.ctypes.data for a in arrays], len(arrays[0]), C.byref(first), *[C.byref(o) for o in outs])
    where = tuple(a[first.value].hex() for a in arrays) if miss else ()
    return miss, where, [o.value for o in outs]


def test_seed_is_a_24_bit_seed(lib):
    b = _random_mantissa(np.random.default_rng(1), 200_000, -300, 300)
    err = lib.svs_host_rcp_seed_error(b.ctypes.data, len(b))
    assert 2.0 ** -30 < err <= 2.0 ** -23, err


def test_div_rn_with_the_rounded_reciprocal_is_the_quotient(lib):
    rng = np.random.default_rng(2)
    a, b = _random_mantissa(rng, N_RANDOM, -200, 200), _random_mantissa(rng, N_RANDOM, -200, 200)
    miss, where, _ = _check(lib.svs_host_div_rn_exact_rcp, a, b)
    assert miss == 0, (miss, where)
    a, b = _cloud_operands(rng, 1_000_000)
    miss, where, _ = _check(lib.svs_host_div_rn_exact_rcp, a, b)
    assert miss == 0, ("cloud ranges", miss, where)
    h = _with_exponents(_hostile_mantissas(), [0, 1, -1, 37, -52, 200, -200])
    a, b = np.repeat(h, 64), np.tile(rng.permutation(h)[:64 * 8], len(h) // 8 + 1)[:len(h) * 64]
    miss, where, _ = _check(lib.svs_host_div_rn_exact_rcp, a, b)
    assert miss == 0, ("hostile mantissas", miss, where)
    ones = _with_exponents(np.asarray([(1 << 52) - 1], np.uint64), [0, 5, -7])           # b = all ones against every hostile numerator
    a, b = np.tile(h, len(ones)), np.repeat(ones, len(h))
    miss, where, _ = _check(lib.svs_host_div_rn_exact_rcp, a, b)
    assert miss == 0, ("all-ones denominators", miss, where)


def test_two_newton_steps_reach_the_rounded_reciprocal(lib):
    rng = np.random.default_rng(3)
    for name, b in (("random", _random_mantissa(rng, N_RANDOM, -400, 400)), ("cloud ranges", _cloud_operands(rng, 1_000_000)[1])):
        first = C.c_long(-1)
        miss = lib.svs_host_rcp_rn(b.ctypes.data, len(b), C.byref(first), None)
        assert miss == 0, (name, miss, b[first.value].hex())
    # hostile mantissas: every one but the all-ones pattern
    man = _hostile_mantissas()
    ones = np.uint64((1 << 52) - 1)
    b = _with_exponents(man[man != ones], [0, 1, -1, 37, -52, 300, -300])
    first = C.c_long(-1)
    miss = lib.svs_host_rcp_rn(b.ctypes.data, len(b), C.byref(first), None)
    assert miss == 0, ("hostile", miss, b[first.value].hex())
    # the all-ones mantissa: the documented exception, pinned -- the iteration returns the double just below RN(1 / b)
    b = _with_exponents(np.asarray([ones], np.uint64), [0, 1, -1, 37, -52, 300, -300])
    out = np.empty_like(b)
    miss = lib.svs_host_rcp_rn(b.ctypes.data, len(b), C.byref(first), out.ctypes.data)
    assert miss == len(b)
    assert np.array_equal(np.abs(out), np.nextafter(np.abs(1.0 / b), 0.0)) and np.array_equal(np.signbit(out), np.signbit(b))
    # ... and rcp_rn_checked refuses every one of them
    miss, where, (n_ok,) = _check(lib.svs_host_rcp_checked, b, extra=(1,))
    assert miss == 0 and n_ok == 0, (miss, where, n_ok)


def test_checked_reciprocal_accepts_only_the_rounded_one(lib):
    rng = np.random.default_rng(4)
    b = _random_mantissa(rng, N_RANDOM, -520, 520)
    miss, where, (n_ok,) = _check(lib.svs_host_rcp_checked, b, extra=(1,))
    inside = int(((np.frexp(b)[1] - 1 >= WINDOW_LO) & (np.frexp(b)[1] - 1 <= WINDOW_HI)).sum())
    assert miss == 0, (miss, where)
    assert inside - 50 <= n_ok <= inside, (n_ok, inside)          # inside the window all but the near-ties (2^-20 of them) are accepted; outside none
    b = _with_exponents(_hostile_mantissas(), [0, 1, -1, 37, WINDOW_LO, WINDOW_LO - 1, WINDOW_HI, WINDOW_HI + 1, 1023, -1022])
    miss, where, _ = _check(lib.svs_host_rcp_checked, b, extra=(1,))
    assert miss == 0, (miss, where)


def test_window_edges(lib):
    for e, want in ((WINDOW_LO, 1), (WINDOW_LO - 1, 0), (WINDOW_HI, 1), (WINDOW_HI + 1, 0)):
        for man in (1.0, 1.5, float(_f64([(1023 << 52) | ((1 << 52) - 1)])[0])):
            for s in (1.0, -1.0):
                assert lib.svs_host_quot_exp_ok(s * man * 2.0 ** e) == want, (e, man, s)
    for x in (0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, float("inf"), float("-inf"), float("nan")):
        assert lib.svs_host_quot_exp_ok(x) == 0, x


def test_guarded_forms_equal_the_division_everywhere(lib):
    rng = np.random.default_rng(5)
    with np.errstate(all="ignore"):
        # the whole range of doubles, subnormal and huge operands included
        a, b = _random_mantissa(rng, N_RANDOM, -1022, 1023), _random_mantissa(rng, N_RANDOM, -1022, 1023)
        miss, where, (n_fast,) = _check(lib.svs_host_div_guarded, a, b, extra=(1,))
        assert miss == 0, (miss, where)
        assert 0.15 * N_RANDOM < n_fast < 0.35 * N_RANDOM, n_fast      # (1001 / 2046)^2 of the pairs are inside the window
        # the clouds' ranges: all on the short path but the near-ties
        a, b = _cloud_operands(rng, 1_000_000)
        miss, where, (n_fast,) = _check(lib.svs_host_div_guarded, a, b, extra=(1,))
        assert miss == 0, ("cloud ranges", miss, where)
        assert n_fast >= len(a) - 50, n_fast
        # hostile mantissas at the edges of the window and of the format, against each other
        pool = np.concatenate([window_edge_values(), SPECIAL, subnormals(rng)])      # (tests/quotient_pools.py: the device test divides the same operands)
        a = np.tile(pool, 40)
        b = rng.permutation(np.tile(pool, 40))
        miss, where, _ = _check(lib.svs_host_div_guarded, a, b, extra=(1,))
        assert miss == 0, ("hostile pairs", miss, where)
        ones = all_ones([0, 3, WINDOW_LO, WINDOW_HI])
        a, b = np.tile(pool, len(ones)), np.repeat(ones, len(pool))
        miss, where, _ = _check(lib.svs_host_div_guarded, a, b, extra=(1,))
        assert miss == 0, ("all-ones denominators", miss, where)
