"""Fr on a fixed schedule (charon_amd/csrc/bls_frct.h) on the host.

tests/frct compiles the header for the CPU twice: over uint32_t, as the
kernels of k_shares.hip use it, and over a counting word type that defines no
comparison, no operator bool and no conversion to an integer -- that the
library builds at all shows the header tests no value.  Exact against Python
integers:

  * add, sub, mul, the byte conversions, select and the zero mask over every
    ordered pair of tests/edge_scalars.VALID plus {0, 1, r - 1}: a + b == r,
    a - a, 0 - 1, (r - 1)^2 and an operand whose nine low limbs are all
    0xFFFFFFF (edge_scalars.SIX_F; the top limb of a value below r is at
    most 7) are among them;
  * Horner's rule and the interpolation at 0, as the two kernels compose them,
    against tbls._split_host and tbls.combine_shares;
  * identical operation counts per kind for every operand value at fixed
    (t, i) and at fixed identifiers;
  * the stand-alone program under AddressSanitizer and UBSan over the same
    operands: a subprocess, nothing loaded into Python.
"""
import ctypes
import itertools
import random
import subprocess

import numpy as np
import pytest

from charon_amd import tbls
from tests import edge_scalars as es

R = es.R
OPERANDS = [0, 1, R - 1] + [k for k in es.VALID if k not in (1, R - 1)]
OP_ADD, OP_SUB, OP_MUL, OP_ROUND, OP_SELECT_A, OP_SELECT_B, OP_ZERO_MASK = range(7)
KINDS = ["add", "sub", "mul", "and", "or", "xor", "not", "shl", "shr", "widen", "narrow"]
PAIRS = list(itertools.product(OPERANDS, repeat=2))
A32 = b"".join(es.be32(a) for a, _ in PAIRS)
B32 = b"".join(es.be32(b) for _, b in PAIRS)


@pytest.fixture(scope="module")
def hc():
    from tests.frct import lib
    return lib()


def run(hc, op):
    out = np.zeros((len(PAIRS), 32), dtype=np.uint8)
    a, b = np.frombuffer(A32, np.uint8), np.frombuffer(B32, np.uint8)
    assert hc.frh_ops(op, a.ctypes.data, b.ctypes.data, len(PAIRS), out.ctypes.data) == 0
    return [int.from_bytes(bytes(o), "big") for o in out]


def test_the_operands_hold_the_directed_cases():
    assert {0, 1, R - 1, es.SIX_F} <= set(OPERANDS) and all(0 <= k < R for k in OPERANDS)
    assert any(a + b == R for a, b in PAIRS) and (0, 1) in PAIRS and (R - 1, R - 1) in PAIRS
    limbs = [(es.SIX_F >> (28 * i)) & 0xFFFFFFF for i in range(10)]
    assert limbs[:9] == [0xFFFFFFF] * 9 and limbs[9] == 6


@pytest.mark.parametrize("op,want", [(OP_ADD, lambda a, b: (a + b) % R), (OP_SUB, lambda a, b: (a - b) % R),
                                     (OP_MUL, lambda a, b: a * b % R), (OP_ROUND, lambda a, b: a),
                                     (OP_SELECT_A, lambda a, b: a), (OP_SELECT_B, lambda a, b: b),
                                     (OP_ZERO_MASK, lambda a, b: 0xFFFFFFFF if a == 0 else 0)],
                         ids=["add", "sub", "mul", "bytes", "select_a", "select_b", "zero_mask"])
def test_operations_are_exact(hc, op, want):
    for (a, b), got in zip(PAIRS, run(hc, op)):
        assert got == want(a, b), (hex(a), hex(b))


class Fixed:
    """An rng that hands out a given list (tbls._split_host draws with randrange)."""

    def __init__(self, vals):
        self.vals = list(vals)

    def randrange(self, lo, hi):
        return self.vals.pop(0)


def horner(hc, poly, i, count=False):
    coef = np.frombuffer(b"".join(es.be32(c) for c in poly), np.uint8)
    sh, la = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    z = ctypes.c_uint32(7)
    counts = np.zeros(len(KINDS), dtype=np.uint64)
    if count:
        assert hc.frh_count_horner(coef.ctypes.data, len(poly), i, counts.ctypes.data, sh.ctypes.data, la.ctypes.data,
                                   ctypes.addressof(z)) == 0
    else:
        assert hc.frh_horner(coef.ctypes.data, len(poly), i, sh.ctypes.data, la.ctypes.data, ctypes.addressof(z)) == 0
    return int.from_bytes(bytes(sh), "big"), int.from_bytes(bytes(la), "big"), z.value, counts.tolist()


def combine(hc, shares, count=False):
    val = np.frombuffer(b"".join(es.be32(s.value) for s in shares), np.uint8)
    ids = np.array([s.identifier for s in shares], dtype=np.uint8)
    out = np.zeros(32, np.uint8)
    z = ctypes.c_uint32(7)
    counts = np.zeros(len(KINDS), dtype=np.uint64)
    if count:
        assert hc.frh_count_combine(val.ctypes.data, ids.ctypes.data, len(shares), counts.ctypes.data, out.ctypes.data,
                                    ctypes.addressof(z)) == 0
    else:
        assert hc.frh_combine(val.ctypes.data, ids.ctypes.data, len(shares), out.ctypes.data, ctypes.addressof(z)) == 0
    return int.from_bytes(bytes(out), "big"), z.value, counts.tolist()


SPLITS = [(2, 2), (3, 4), (7, 10), (20, 255)]


@pytest.mark.parametrize("t,n", SPLITS)
def test_horner_equals_the_host_split(hc, t, n):
    rng = random.Random(0x5EC0 + t)
    pool = [k for k in OPERANDS if k] + [rng.randrange(1, R) for _ in range(t)]
    poly = [pool[(3 * j + t) % len(pool)] for j in range(t)]
    shares, got_poly = tbls._split_host(poly[0], t, n, Fixed(poly[1:]))
    assert got_poly == poly
    for s in shares if n <= 10 else shares[:3] + shares[-3:]:
        assert horner(hc, poly, s.identifier)[:3] == (s.value, s.value, 0), s.identifier


def test_a_zero_share_is_flagged_and_its_ladder_scalar_is_one(hc):
    a = es.VALID[20]
    assert horner(hc, [R - a, a], 1)[:3] == (0, 1, 1)      # f(1) = 0
    assert horner(hc, [R - a, a], 2)[:3] == (a, a, 0)
    assert horner(hc, [R - 2, 0, 1, 0], 1)[:3] == (R - 1, R - 1, 0)  # zero coefficients are arithmetic like any other


@pytest.mark.parametrize("t,n", SPLITS)
def test_interpolation_equals_combine_shares(hc, t, n):
    rng = random.Random(0xC0B1 + t)
    secret = es.VALID[(5 * t) % len(es.VALID)]
    shares, _ = tbls._split_host(secret, t, n, rng)
    picks = [shares[:t], shares[-t:], shares] if n <= 10 else [shares[:t], rng.sample(shares, t + 1)]
    for pick in picks:
        pick = list(pick)
        rng.shuffle(pick)  # (unsorted identifiers)
        assert combine(hc, pick)[:2] == (tbls.combine_shares(pick, t, n), 0) == (secret, 0)
    # shares of f(x) = a x recombine to 0, which is flagged
    line = [tbls.SecretKeyShare(i, secret * i % R) for i in (254, 255, 3)]
    assert combine(hc, line)[:2] == (0, 1)


def test_counts_do_not_depend_on_the_operands(hc):
    assert hc.frh_count_kinds() == len(KINDS)
    rng = random.Random(7)
    for t, i in [(2, 1), (3, 4), (7, 255)]:
        polys = [[OPERANDS[(j + s) % len(OPERANDS)] for j in range(t)] for s in range(0, len(OPERANDS), 3)]
        polys += [[0] * t, [R - 1] * t, [rng.randrange(R) for _ in range(t)]]
        seen = set()
        for poly in polys:
            value, ladder, zero, counts = horner(hc, poly, i, count=True)
            assert (value, ladder, zero) == horner(hc, poly, i)[:3]  # the counting instantiation computes the same
            assert value == sum(c * i ** j for j, c in enumerate(poly)) % R
            seen.add(tuple(counts))
        assert len(seen) == 1, (t, i, seen)
        c = dict(zip(KINDS, seen.pop()))
        print("horner counts at t=%d, i=%d:" % (t, i), c)
        assert c["mul"] > 0 and c["not"] == 0
    ids = [9, 2, 255, 17]
    seen = set()
    for s in range(0, len(OPERANDS), 2):
        shares = [tbls.SecretKeyShare(i, OPERANDS[(s + j) % len(OPERANDS)]) for j, i in enumerate(ids)]
        value, zero, counts = combine(hc, shares, count=True)
        assert (value, zero) == combine(hc, shares)[:2]
        seen.add(tuple(counts))
    assert len(seen) == 1


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """frct_main.cpp, -fsanitize=address,undefined, as a subprocess over the same operands."""
    from tests.frct import build_sanitized
    exe = build_sanitized()
    data = tmp_path / "operands.bin"
    data.write_bytes(b"".join(es.be32(k) for k in OPERANDS))
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "frct_main ok: %d operands" % len(OPERANDS) in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
