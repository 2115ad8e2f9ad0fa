"""The fused level 0's per-duty key side (charon_amd/csrc/bls_rlc.h
rlc_duty_keys_l0f: P_d = sum_i [r_i] pk_i in Straus' joint form, the doublings
shared by the duty's candidates) on the host, built from the kernel's own
template (tests/l0straus) against

  * sum_i rlc_mul_key_l0f(tab_i, beta, u_i) -- the per-partial product --
    added with the complete additions: the same affine point, and
  * for a few duties, Python integers: sum_i [r_i] pk_i with r_i = a_0 + a_1 x
    + a_2 x^2 + a_3 x^3, a_j = 2 u_j - (2^n_j - 1).

The additions of the joint form meet points of different keys and of one key
named twice: equal operands, opposite operands and an infinite accumulator are
legal input.  `complete=False` is the control that shows the duplicate-key
cases do reach the doubling branch.
"""
import ctypes
import random

import numpy as np
import pytest

X = -0xD201000000010000
NBITS = (20, 20, 16, 16)
UMAX = tuple((1 << n) - 1 for n in NBITS)


@pytest.fixture(scope="module")
def ls():
    from tests.l0straus import lib
    return lib()


@pytest.fixture(scope="module")
def keys():
    """12 keys; key 11 is -key 0."""
    from oracle import bls12_381 as bls
    rng = random.Random(0x10F5)
    pts = [bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R)) for _ in range(11)]
    pts.append(bls.g1_neg(pts[0]))
    return pts, b"".join(bls.g1_compress(p) for p in pts)


def rand_digits(rng, n):
    return [[rng.randrange(0, m + 1) for m in UMAX] for _ in range(n)]


def _args(pid, u, cand):
    pid = np.ascontiguousarray(pid, dtype=np.uint32)
    u = np.ascontiguousarray(u, dtype=np.uint32).reshape(-1)
    cand = np.ascontiguousarray(cand, dtype=np.uint8)
    assert len(u) == 4 * len(pid) and len(cand) == len(pid)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return (pid, u, cand), (vp(pid), vp(u), vp(cand), len(pid))


def straus(ls, keys, pid, u, cand=None, complete=True):
    """(compressed P_d, infinite?, an addition met equal operands?)"""
    cand = [1] * len(pid) if cand is None else cand
    keep, a = _args(pid, u, cand)
    out = ctypes.create_string_buffer(48)
    exc = ctypes.c_int(-1)
    rc = ls.ls_duty(keys[1], len(keys[0]), a[0], a[1], a[2], a[3], 1 if complete else 0, ctypes.byref(exc), out)
    assert rc in (0, 1), rc
    return out.raw, rc == 1, exc.value == 1


def reference(ls, keys, pid, u, cand=None):
    cand = [1] * len(pid) if cand is None else cand
    keep, a = _args(pid, u, cand)
    out = ctypes.create_string_buffer(48)
    rc = ls.ls_reference(keys[1], len(keys[0]), a[0], a[1], a[2], a[3], out)
    assert rc in (0, 1), rc
    return out.raw, rc == 1


def integers(keys, pid, u, cand=None):
    from oracle import bls12_381 as bls
    cand = [1] * len(pid) if cand is None else cand
    acc = None
    for p, uu, c in zip(pid, u, cand):
        if not c:
            continue
        r = sum((2 * uu[j] - UMAX[j]) * X ** j for j in range(4)) % bls.R
        acc = bls.g1_add(acc, bls.g1_mul(keys[0][p], r))
    return acc


def test_fused_digits_are_the_kernels(ls):
    """u_j = rho_j + 2^(n_j - 1) for the extreme digit vectors: 0 < u_j < 2^n_j."""
    c = np.array([[6] * 18, [-6] * 18, [0] * 18], dtype=np.int32)
    u = np.zeros(12, dtype=np.uint32)
    ls.ls_digits(c.ctypes.data_as(ctypes.c_void_p), 3, u.ctypes.data_as(ctypes.c_void_p))
    u = u.reshape(3, 4)
    assert (u[2] == [1 << 19, 1 << 19, 1 << 15, 1 << 15]).all()
    assert (u[0] == [(1 << 19) + 185646, (1 << 19) + 185646, (1 << 15) + 14280, (1 << 15) + 14280]).all()
    assert ((u[0].astype(np.int64) + u[1]) == [1 << 20, 1 << 20, 1 << 16, 1 << 16]).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 10])
def test_duty_sum_is_the_sum_of_the_partial_products(ls, keys, n):
    rng = random.Random(100 + n)
    for rep in range(3):
        pid = [rng.randrange(0, 11) for _ in range(n)] if rep else list(range(n))
        u = rand_digits(rng, n)
        got, inf, _ = straus(ls, keys, pid, u)
        assert (got, inf) == reference(ls, keys, pid, u) and not inf


@pytest.mark.parametrize("n", [1, 3, 10])
def test_reference_matches_python_integers(ls, keys, n):
    from oracle import bls12_381 as bls
    rng = random.Random(200 + n)
    pid = [rng.randrange(0, 11) for _ in range(n)]
    u = rand_digits(rng, n)
    want = bls.g1_compress(integers(keys, pid, u))
    assert reference(ls, keys, pid, u) == (want, False)
    assert straus(ls, keys, pid, u)[:2] == (want, False)


@pytest.mark.parametrize("where", ["first", "middle", "last", "first_and_last"])
def test_non_candidates_are_left_out(ls, keys, where):
    rng = random.Random(300)
    n = 7
    pid, u = list(range(n)), rand_digits(rng, n)
    out = {"first": [0], "middle": [3], "last": [n - 1], "first_and_last": [0, 1, n - 1]}[where]
    cand = [0 if k in out else 1 for k in range(n)]
    got = straus(ls, keys, pid, u, cand)
    assert got[:2] == reference(ls, keys, pid, u, cand) and not got[1]
    kept = [k for k in range(n) if cand[k]]
    assert got[0] == straus(ls, keys, [pid[k] for k in kept], [u[k] for k in kept])[0]
    assert got[0] != straus(ls, keys, pid, u)[0]


def test_no_candidate_is_infinity(ls, keys):
    got = straus(ls, keys, [0, 1, 2], [[5, 6, 7, 8]] * 3, [0, 0, 0])
    assert got[1] and got[:2] == reference(ls, keys, [0, 1, 2], [[5, 6, 7, 8]] * 3, [0, 0, 0])


@pytest.mark.parametrize("n", [1, 3, 4])
@pytest.mark.parametrize("digits", ["zero", "max"])
def test_extreme_digits(ls, keys, n, digits):
    from oracle import bls12_381 as bls
    u = [[0, 0, 0, 0] if digits == "zero" else list(UMAX)] * n
    pid = list(range(n))
    got = straus(ls, keys, pid, u)
    assert got[:2] == reference(ls, keys, pid, u) and not got[1]
    assert got[0] == bls.g1_compress(integers(keys, pid, u))


def test_same_key_twice_with_identical_digits(ls, keys):
    """P = 2 [r] pk: every addition of the second copy meets acc == entry in
    window 9 and equal multiples later on."""
    from oracle import bls12_381 as bls
    rng = random.Random(400)
    for n, dup in ((2, (0, 1)), (4, (1, 3)), (7, (0, 6))):
        pid, u = list(range(n)), rand_digits(rng, n)
        pid[dup[1]], u[dup[1]] = pid[dup[0]], u[dup[0]]
        got = straus(ls, keys, pid, u)
        assert got[:2] == reference(ls, keys, pid, u) and not got[1]
        assert got[0] == bls.g1_compress(integers(keys, pid, u))
    # the lone pair: exactly twice the single product
    u1 = rand_digits(rng, 1)
    one = integers(keys, [2], u1)
    assert straus(ls, keys, [2, 2], u1 * 2)[0] == bls.g1_compress(bls.g1_add(one, one))


def test_same_key_twice_with_equal_top_windows(ls, keys):
    """Digits equal in windows 9 and 8 only (bits 16..19 of u_0, u_1): the
    first addition of the second copy is a doubling, the rest are not."""
    from oracle import bls12_381 as bls
    rng = random.Random(500)
    a = rand_digits(rng, 1)[0]
    b = rand_digits(rng, 1)[0]
    b[0] = (a[0] & 0xF0000) | (b[0] & 0xFFFF)
    b[1] = (a[1] & 0xF0000) | (b[1] & 0xFFFF)
    assert a != b
    for pid, u in (([4, 4], [a, b]), ([1, 4, 2, 4], [rand_digits(rng, 1)[0], a, rand_digits(rng, 1)[0], b])):
        got = straus(ls, keys, pid, u)
        assert got[:2] == reference(ls, keys, pid, u) and not got[1]
        assert got[0] == bls.g1_compress(integers(keys, pid, u))


def test_opposite_keys_cancel_and_infinity_is_reported(ls, keys):
    """pk and -pk with identical digits: the accumulator returns to infinity
    in every window; a duty whose only candidates cancel has P_d = infinity
    (the kernel's RLC_EACH), and beside other candidates the pair adds nothing."""
    rng = random.Random(600)
    u = rand_digits(rng, 1)[0]
    got = straus(ls, keys, [0, 11], [u, u])
    assert got[1] and got[:2] == reference(ls, keys, [0, 11], [u, u])
    # ... with a non-candidate between them
    v = rand_digits(rng, 1)[0]
    got = straus(ls, keys, [0, 5, 11], [u, v, u], [1, 0, 1])
    assert got[1] and got[:2] == reference(ls, keys, [0, 5, 11], [u, v, u], [1, 0, 1])
    # ... first, so that the next candidate's first entry meets an infinite accumulator
    got = straus(ls, keys, [0, 11, 5, 6], [u, u, v, u])
    assert got[:2] == reference(ls, keys, [0, 11, 5, 6], [u, u, v, u]) and not got[1]
    assert got[0] == straus(ls, keys, [5, 6], [v, u])[0]
    # ... and last
    got = straus(ls, keys, [5, 6, 0, 11], [v, u, u, u])
    assert got[0] == straus(ls, keys, [5, 6], [v, u])[0] and not got[1]


def test_incomplete_addition_fails_on_duplicate_keys(ls, keys):
    """Control: with the mixed addition that has no doubling branch the
    duplicate-key duties meet equal operands and give another point; duties
    of distinct keys never reach that branch."""
    rng = random.Random(700)
    u = rand_digits(rng, 4)
    got = straus(ls, keys, [0, 1, 2, 3], u, complete=False)
    assert not got[2] and got[:2] == reference(ls, keys, [0, 1, 2, 3], u)
    a, b = list(u[0]), list(u[1])
    b[0] = (a[0] & 0xF0000) | (b[0] & 0xFFFF)
    b[1] = (a[1] & 0xF0000) | (b[1] & 0xFFFF)
    # (the two copies lead the duty: in window 9 the accumulator IS the first copy's entry)
    for pid, uu in (([2, 2], [u[0], u[0]]), ([3, 3, 0, 1], [u[1], u[1], u[2], u[3]]), ([4, 4], [a, b])):
        bad = straus(ls, keys, pid, uu, complete=False)
        assert bad[2], pid
        assert bad[:2] != reference(ls, keys, pid, uu), pid
        assert straus(ls, keys, pid, uu)[:2] == reference(ls, keys, pid, uu)
