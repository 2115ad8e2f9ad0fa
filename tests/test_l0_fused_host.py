"""The fused level 0 (charon_amd/csrc/bls_rlc.h, top) on the host: level 0's
scalar of a partial as a fixed linear form of its 18 subgroup digits, the
key product by 10 + 8 windows of the per-key table, and the signature side
S = sum_j psi^j(2 A_j + T) from the subgroup test's sums -- the kernels' math
compiled for the CPU (tests/l0fused, lane pairs emulated, value bounds
checked) against oracle/bls12_381.py.
"""
import ctypes
import random

import numpy as np
import pytest

from oracle import bls12_381 as bls

FIRST = [0, 5, 10, 14, 18]
BITS = [20, 20, 16, 16]
SEEDS = [
    np.array([0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0x4B5A6978, 0x11111111, 0x22222222, 0x33333333, 0x44444444],
             dtype=np.uint32),
    np.array([0, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint32),
    np.array([0xFFFFFFFF] * 8, dtype=np.uint32),
    np.array([7, 6, 5, 4, 3, 2, 1, 0x80000000], dtype=np.uint32),
]
INDICES = [0, 1, 2, 1023, 1024, 2399, 639999, 0x0FFFFFFF]


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def hc():
    from tests.l0fused import lib
    h = lib()
    h.l0f_hc_digits.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    h.l0f_hc_digits.restype = None
    h.l0f_hc_scalars.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    h.l0f_hc_scalars.restype = None
    h.l0f_hc_g1.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p]
    h.l0f_hc_g1.restype = ctypes.c_int
    h.l0f_hc_g2.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                            ctypes.c_char_p]
    h.l0f_hc_g2.restype = ctypes.c_int
    return h


def digits(hc, seed, i):
    out = np.zeros(18, dtype=np.int32)
    hc.l0f_hc_digits(vp(seed), i, vp(out))
    return out


def scalars(hc, c):
    c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1, 18)
    a = np.zeros((len(c), 4), dtype=np.int32)
    u = np.zeros((len(c), 4), dtype=np.uint32)
    hc.l0f_hc_scalars(vp(c), len(c), vp(a), vp(u))
    return a, u


def a_of(c):
    """a_j = 2 sum_e 13^e c_(first_j + e) + 1, in Python."""
    return [2 * sum(13 ** e * int(c[FIRST[j] + e]) for e in range(FIRST[j + 1] - FIRST[j])) + 1 for j in range(4)]


def r_of(a):
    return (int(a[0]) + int(a[1]) * bls.X + int(a[2]) * bls.X ** 2 + int(a[3]) * bls.X ** 3) % bls.R


def test_scalars_from_the_digits(hc):
    for seed in SEEDS:
        cs = [digits(hc, seed, i) for i in INDICES]
        a, u = scalars(hc, np.stack(cs))
        for c, aj, uj in zip(cs, a, u):
            assert c.min() >= -6 and c.max() <= 6
            assert [int(v) for v in aj] == a_of(c)
            for j in range(4):
                n = BITS[j]
                assert int(aj[j]) % 2 == 1
                assert abs(int(aj[j])) <= (371293 if j < 2 else 28561) < 2 ** (n - 1)
                assert 0 <= int(uj[j]) < 2 ** n
                assert 2 * int(uj[j]) - (2 ** n - 1) == int(aj[j])  # the signed-binary form round-trips


def test_extreme_digit_vectors(hc):
    a, u = scalars(hc, np.stack([np.full(18, 6), np.full(18, -6)]))
    assert [int(v) for v in a[0]] == [371293, 371293, 28561, 28561] == a_of(np.full(18, 6))
    assert [int(v) for v in a[1]] == [-371291, -371291, -28559, -28559] == a_of(np.full(18, -6))
    for k in range(2):
        for j in range(4):
            assert 0 <= int(u[k][j]) < 2 ** BITS[j] and 2 * int(u[k][j]) - (2 ** BITS[j] - 1) == int(a[k][j])


def test_distinct_digit_vectors_give_distinct_scalars(hc):
    rng = np.random.default_rng(0x10F)
    c = np.unique(rng.integers(-6, 7, size=(100000, 18), dtype=np.int32), axis=0)
    assert len(c) > 99990
    a, _ = scalars(hc, c)
    assert len({r_of(aj) for aj in a}) == len(c)
    # the bound behind it: coefficient differences < 2^20 < |x| and 2^20 |x|^3 < r
    assert 2 * 371293 < 2 ** 20 < bls.X_ABS and 2 ** 20 * bls.X_ABS ** 3 < bls.R


def digit_cases():
    rng = random.Random(0xF0)
    return [[6] * 18, [-6] * 18, [0] * 18] + [[rng.randrange(-6, 7) for _ in range(18)] for _ in range(3)]


def test_key_product_by_windows(hc):
    rng = random.Random(0x61)
    keys = [bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R)) for _ in range(3)] + [bls.G1_GEN]
    for pk in keys:
        for c in digit_cases():
            out = ctypes.create_string_buffer(48)
            assert hc.l0f_hc_g1(bls.g1_compress(pk), vp(np.array(c, dtype=np.int32)), out) == 0
            assert out.raw == bls.g1_compress(bls.g1_mul(pk, r_of(a_of(c)))), c


def test_signature_side_horner_form(hc):
    rng = random.Random(0x5C)
    pts = [bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R)) for _ in range(40)]
    buf = b"".join(bls.g2_compress(p) for p in pts)
    for seed, i0 in ((SEEDS[0], 0), (SEEDS[3], 2048)):
        acc = None
        for i, p in enumerate(pts):
            t = bls.g2_mul(p, r_of(a_of(digits(hc, seed, i0 + i))))
            acc = t if acc is None else bls.g2_add(acc, t)
        out = ctypes.create_string_buffer(96)
        assert hc.l0f_hc_g2(buf, 40, 20, vp(seed), i0, out) == 0  # two groups of 20
        assert out.raw == bls.g2_compress(acc)


def test_signature_side_equal_points(hc):
    """Small multiples of ONE point: the Horner steps meet the doubling case."""
    p = bls.g2_mul(bls.G2_GEN, 0xABCDEF)
    buf = bls.g2_compress(p) * 6
    seed = SEEDS[0]
    k = sum(r_of(a_of(digits(hc, seed, i))) for i in range(6)) % bls.R
    out = ctypes.create_string_buffer(96)
    assert hc.l0f_hc_g2(buf, 6, 3, vp(seed), 0, out) == 0
    assert out.raw == bls.g2_compress(bls.g2_mul(p, k))
