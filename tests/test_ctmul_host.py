"""The hardened signer's ladder (charon_amd/csrc/bls_ctmul.h) on the host.

tests/ctmul compiles the template for the CPU with the value bound checks on
(a violated bound aborts the process) and runs it over Fp, over Fp2 through
the device's table layout, and over a counting field type that has no zero
test and no comparison.  Checked against oracle/bls12_381.py:

  * [k] G1 and [k] H(m) for every scalar of tests/edge_scalars.py;
  * the complete addition and doubling on the seven exceptional cases;
  * the recoding: 64 digits in [-7, 8] that sum to k;
  * the schedule: identical operation counts for every scalar, and
    windows x table entries x coordinates selects -- the whole table is
    scanned in every window.
"""
import ctypes

import numpy as np
import pytest

from oracle import bls12_381 as bls
from tests import edge_scalars as es

WINDOWS, ENTRIES, COORDS = 64, 9, 3
KINDS = ["mul", "sqr", "add", "sub", "reduce", "small", "b3", "select", "cneg"]


@pytest.fixture(scope="module")
def hc():
    from tests.ctmul import lib
    h = lib()
    vp, u32, cp = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p
    h.ctm_g1_mul.argtypes = [cp, u32, vp]
    h.ctm_g2_mul.argtypes = [cp, cp, u32, u32, cp, u32, vp]
    h.ctm_g1_law.argtypes = [cp, cp, cp, cp]
    h.ctm_g2_law.argtypes = [cp, cp, cp, cp]
    h.ctm_digits.argtypes = [cp, vp]
    h.ctm_count_kinds.restype = u32
    h.ctm_count.argtypes = [cp, u32, vp, vp]
    return h


SK = b"".join(es.be32(k) for k in es.VALID)
N = len(es.VALID)


@pytest.fixture(scope="module")
def h_m():
    return bls.hash_to_g2(b"ctmul host twin")


def test_g1_products_match_the_oracle(hc):
    out = np.zeros((N, 48), dtype=np.uint8)
    assert hc.ctm_g1_mul(SK, N, out.ctypes.data) == 0
    for k, got in zip(es.VALID, out):
        assert bytes(got) == bls.g1_compress(bls.g1_mul(bls.G1_GEN, k)), hex(k)


@pytest.mark.parametrize("n_tab,slot", [(1, 0), (3, 1)])
def test_g2_products_match_the_oracle(hc, h_m, n_tab, slot):
    out = np.zeros((N, 96), dtype=np.uint8)
    assert hc.ctm_g2_mul(bls.g2_compress(h_m), bls.g2_compress(bls.G2_GEN), n_tab, slot, SK, N, out.ctypes.data) == 0
    for k, got in zip(es.VALID, out):
        assert bytes(got) == bls.g2_compress(bls.g2_mul(h_m, k)), hex(k)


def _law_cases(gen, mul, neg):
    p, q = mul(gen, 5), mul(gen, 11)
    # (P, Q): P+Q, P+P, P+(-P), P+O, O+P, O+O; the doubling of each P covers 2 O
    return [(p, q), (p, p), (p, neg(p)), (p, None), (None, p), (None, None)]


def test_g1_laws_on_the_exceptional_cases(hc):
    for p, q in _law_cases(bls.G1_GEN, bls.g1_mul, bls.g1_neg):
        s, d = ctypes.create_string_buffer(48), ctypes.create_string_buffer(48)
        assert hc.ctm_g1_law(bls.g1_compress(p), bls.g1_compress(q), s, d) == 0
        want = q if p is None else p if q is None else bls.g1_add(p, q)
        assert s.raw == bls.g1_compress(want)
        assert d.raw == bls.g1_compress(None if p is None else bls.g1_add(p, p))


def test_g2_laws_on_the_exceptional_cases(hc):
    for p, q in _law_cases(bls.G2_GEN, bls.g2_mul, bls.g2_neg):
        s, d = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        assert hc.ctm_g2_law(bls.g2_compress(p), bls.g2_compress(q), s, d) == 0
        want = q if p is None else p if q is None else bls.g2_add(p, q)
        assert s.raw == bls.g2_compress(want)
        assert d.raw == bls.g2_compress(None if p is None else bls.g2_add(p, p))


def test_recoding_is_regular(hc):
    for k in es.VALID:
        d = np.zeros(64, dtype=np.int32)
        hc.ctm_digits(es.be32(k), d.ctypes.data)
        assert d.min() >= -7 and d.max() <= 8, hex(k)
        assert sum(int(v) << (4 * i) for i, v in enumerate(d)) == k, hex(k)


def test_schedule_is_the_same_for_every_scalar(hc):
    assert hc.ctm_count_kinds() == len(KINDS)
    counts = np.zeros((N, len(KINDS)), dtype=np.uint64)
    out = np.zeros((N, 48), dtype=np.uint8)
    ref = np.zeros((N, 48), dtype=np.uint8)
    assert hc.ctm_count(SK, N, counts.ctypes.data, out.ctypes.data) == 0
    assert hc.ctm_g1_mul(SK, N, ref.ctypes.data) == 0
    assert (out == ref).all()  # the counting instantiation computes the same products
    c = dict(zip(KINDS, counts[0].tolist()))
    print("ladder counts per scalar:", c)
    assert (counts == counts[0]).all()
    # the table is scanned: every entry's every coordinate, in every window
    assert c["select"] == WINDOWS * ENTRIES * COORDS
    assert c["cneg"] == WINDOWS
    # 256 doublings of 6 products + 2 squarings, 64 additions of 12 products
    assert c["mul"] == 256 * 6 + 64 * 12
    assert c["sqr"] == 256 * 2
    assert c["b3"] == 256 * 1 + 64 * 2
