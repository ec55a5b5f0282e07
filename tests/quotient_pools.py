"""Operand pools for the exact quotients of scavislam_amd/csrc/devutil.h (rcp_rn / div_rn and their guarded forms), shared by tests/test_quotient_cpu.py (the header
compiled for the host) and tests/test_gpu_gate_edges.py (the device's own reciprocal seed, frexp_mant and subnormal handling, through processMatchedPoints' gate)."""
import numpy as np

WINDOW_LO, WINDOW_HI = -500, 500      # unbiased exponents the guard lets through (devutil.h: quot_exp_ok)
ALL_ONES = np.uint64((1 << 52) - 1)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.225073858507201e-308, -2.225073858507201e-308, 1.7976931348623157e308, 1.0, -1.0])


def _f64(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def _random_mantissa(rng, n, emin, emax):
    """doubles with uniform random mantissa bits, sign and an unbiased exponent uniform in [emin, emax]"""
    man = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    exp = rng.integers(emin + 1023, emax + 1024, n, dtype=np.uint64)
    sign = rng.integers(0, 2, n, dtype=np.uint64)
    return _f64((sign << np.uint64(63)) | (exp << np.uint64(52)) | man)


def _hostile_mantissas():
    """mantissa fields: all ones and its neighbours, powers of two and their neighbours, single bits, alternating patterns"""
    one = (1 << 52) - 1
    m = [0, 1, 2, 3, one, one - 1, one - 2, one >> 1, (one >> 1) + 1, 1 << 51, (1 << 51) + 1, (1 << 51) - 1, 0x5555555555555, 0xAAAAAAAAAAAAA, 0x3333333333333]
    m += [1 << k for k in range(52)] + [one ^ (1 << k) for k in range(52)] + [one >> k for k in range(1, 40)] + [one ^ (one >> k) for k in range(1, 40)]
    return np.unique(np.asarray(m, np.uint64))


def _with_exponents(man, exps):
    e = np.asarray(exps, np.int64) + 1023
    assert e.min() >= 1 and e.max() <= 2046
    g = (e.astype(np.uint64)[:, None] << np.uint64(52)) | man[None, :]
    return np.concatenate([_f64(g.ravel()), -_f64(g.ravel())])


def _cloud_operands(rng, n):
    """r[3] = d / b and r[0..2] of computeDensePointCloudCpu for disparities 2^-10 ... 2^10 (floats, as the cloud reads them), baselines 0.05 ... 0.6 m, pixel
    coordinates of a frame up to 2048 wide around its principal point and f = 200 ... 1500, at poses with a rotation and a translation of a few metres"""
    d = (2.0 ** rng.uniform(-10, 10, n)).astype(np.float32).astype(np.float64)
    b = rng.uniform(0.05, 0.6, n)
    ib = 1.0 / b
    r3 = ib * d                                                   # TQ[14] * q[2] with TQ[14] = 1 / b: the denominator at any pose (last row of TQ is 0 0 1/b 0)
    x, y, f = rng.uniform(-1024, 1024, n), rng.uniform(-1024, 1024, n), rng.uniform(200, 1500, n)
    R = rng.normal(size=(n, 3))
    R /= np.linalg.norm(R, axis=1, keepdims=True)
    num = R[:, 0] * x + R[:, 1] * y + R[:, 2] * f + rng.uniform(-5, 5, n) * r3
    return num, r3


def all_ones(exps):
    """the denominators two Newton steps do not reach RN(1 / b) for: mantissa of all ones, both signs"""
    return _with_exponents(np.asarray([ALL_ONES], np.uint64), exps)


def window_edge_values(exps=(0, -1, WINDOW_LO, WINDOW_LO - 1, WINDOW_HI, WINDOW_HI + 1, 1023, -1022, -1000, 1000)):
    """hostile mantissas at the edges of the window and of the format"""
    return _with_exponents(_hostile_mantissas(), list(exps))


def subnormals(rng, n=500):
    sub = _f64(rng.integers(1, 1 << 52, n, dtype=np.uint64))
    return np.concatenate([sub, -sub])


def exponent(x):
    """unbiased exponent of finite non-zero doubles (frexp's convention shifted to IEEE's); subnormals below -1022"""
    return np.frexp(x)[1] - 1


def in_window(x):
    """devutil.h's quot_exp_ok: the exponent FIELD inside [1023 - 500, 1023 + 500]; zeros, subnormals, infinities and NaN are outside"""
    f = (np.asarray(x, np.float64).view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7FF
    return (f >= 1023 + WINDOW_LO) & (f <= 1023 + WINDOW_HI)
