"""Directed Feldman commitment polynomials for tbg_eval_commitments
(charon_amd/csrc/bls_feldman.h, k_feldman.hip), shared by the CPU run through
the host twin tests/feldman (test_feldman_host.py, TBG_BOUNDS_CHECK on) and
the GPU run through the engine (test_gpu_feldman.py).  Deterministic; built
with Python integers and oracle/bls12_381.py only.

A polynomial is its integer coefficients a_0 .. a_(t-1) mod r.  Commitment j
is g1_compress([a_j] G1), the identity encoding for a_j = 0, and the expected
result at an identifier is ALWAYS g1_compress([f(id) mod r] G1) from the
integers -- no group law of the code under test is restated for it.

What the Horner chain (acc = C_(t-1); acc = [id] acc + C_j, j = t-2 .. 0)
meets on a polynomial is decided from the integers by horner_events(), and
every directed case asserts its branch at import:

  dbl      [id] acc == C_j: the addition is a doubling (jac_add_aff's P == Q arm)
  cancel   [id] acc == -C_j: the sum is infinity in mid-chain
  inf_acc  the running value is infinity when a Horner step starts
  inf_c    C_j is the identity (j >= 1: it contributes infinity)
"""
import collections
import functools
import random

from oracle import bls12_381 as bls

R = bls.R
FV_OK, FV_ID, FV_COMMIT, FV_KEY_IDENTITY, FV_IDENTITY = 0, -50, -51, -52, -53
IDENT48 = bytes([0xC0]) + bytes(47)
ZERO48 = bytes(48)

# the directed identifiers (0: TBG_FV_ID)
IDS = [1, 2, 3, 128, 255, 256, 1 << 31, (1 << 32) - 1, 0]

Case = collections.namedtuple("Case", "name coeffs ids")


# ---------------------------------------------------------------------------
# [k] G1 from a fixed-base table (8-bit windows): 32 additions per product
@functools.lru_cache(None)
def _gen_table():
    F = bls._Fp
    tab, base = [], bls.pt_from_affine(bls.G1_GEN, F)
    for _ in range(32):
        row, acc = [None], None
        for _d in range(255):
            acc = base if acc is None else bls.pt_add(acc, base, F)
            row.append(acc)
        tab.append(row)
        base = bls.pt_add(row[255], base, F)
    return tab


@functools.lru_cache(None)
def gen_mul(k):
    """[k mod r] G1, affine, None for the identity."""
    F = bls._Fp
    k %= R
    tab, acc = _gen_table(), None
    for w in range(32):
        d = (k >> (8 * w)) & 0xFF
        if d:
            acc = tab[w][d] if acc is None else bls.pt_add(acc, tab[w][d], F)
    return None if acc is None else bls.pt_to_affine(acc, F)


assert gen_mul(1) == bls.G1_GEN and gen_mul(0) is None
assert gen_mul(R - 1) == bls.g1_neg(bls.G1_GEN) and gen_mul(0x1234567 << 200) == bls.g1_mul(bls.G1_GEN, 0x1234567 << 200)


def commit(a):
    return bls.g1_compress(gen_mul(a))


def commits(coeffs):
    return [commit(a) for a in coeffs]


def f(coeffs, x):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % R
    return acc


def expected(coeffs, ident):
    """(eval status, 48 output bytes) of a polynomial whose commitments all decode."""
    if ident == 0:
        return FV_ID, ZERO48
    if coeffs[0] % R == 0:
        return FV_KEY_IDENTITY, ZERO48
    v = f(coeffs, ident)
    if v == 0:
        return FV_IDENTITY, IDENT48
    return FV_OK, bls.g1_compress(gen_mul(v))


def horner_events(coeffs, ident):
    """[(j, event)] of the chain at `ident`, from the integers."""
    a = [c % R for c in coeffs]
    ev = []
    acc = a[-1]
    if acc == 0 and len(a) > 1:
        ev.append((len(a) - 1, "inf_c"))
    for j in range(len(a) - 2, -1, -1):
        if acc == 0:
            ev.append((j, "inf_acc"))
        m = acc * ident % R
        if a[j] == 0:
            ev.append((j, "inf_c"))
        elif m != 0 and m == a[j]:
            ev.append((j, "dbl"))
        elif m != 0 and (m + a[j]) % R == 0:
            ev.append((j, "cancel"))
        acc = (m + a[j]) % R
    return ev


# ---------------------------------------------------------------------------
# the directed polynomials
def _cases():
    rng = random.Random(0xFE1D)
    rnd = lambda: rng.randrange(1, R)  # noqa: E731
    out = []
    a1 = rnd()
    out.append(Case("dbl_t2", [5 * a1 % R, a1], [5, 4, 6]))
    a2, a0 = rnd(), rnd()
    out.append(Case("dbl_mid_t3", [a0, 3 * a2 % R, a2], [3, 2, 4]))
    a2, a0 = rnd(), rnd()
    out.append(Case("cancel_mid_t3", [a0, -7 * a2 % R, a2], [7, 6, 8]))
    a = rnd()
    out.append(Case("root_3", [-3 * a % R, a], [1, 2, 3, 4, 5]))
    a = rnd()
    out.append(Case("roots_2_5", [10 * a % R, -7 * a % R, a], [1, 2, 3, 4, 5, 6]))
    out.append(Case("ident_top", [rnd(), rnd(), 0], [1, 2, 3]))
    out.append(Case("ident_mid", [rnd(), 0, rnd()], [1, 2, 3]))
    out.append(Case("ident_c0", [0, rnd(), rnd()], [1, 2, 3]))
    out.append(Case("t1", [rnd()], [1, 2, 255]))
    out.append(Case("generic_t3", [rnd(), rnd(), rnd()], []))
    # every case above also at every directed identifier; the long chain at three only
    out = [c._replace(ids=c.ids + [i for i in IDS if i not in c.ids]) for c in out]
    out.append(Case("long_t170", [rnd() for _ in range(170)], [1, 2, 255]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def _prove():
    c = BY_NAME
    assert horner_events(c["dbl_t2"].coeffs, 5) == [(0, "dbl")] and not horner_events(c["dbl_t2"].coeffs, 4)
    assert horner_events(c["dbl_mid_t3"].coeffs, 3) == [(1, "dbl")] and expected(c["dbl_mid_t3"].coeffs, 3)[0] == FV_OK
    k = c["cancel_mid_t3"]
    assert horner_events(k.coeffs, 7) == [(1, "cancel"), (0, "inf_acc")] and k.coeffs[0] != 0
    assert expected(k.coeffs, 7) == (FV_OK, commit(k.coeffs[0]))  # infinity in mid-chain, then C_0 alone
    assert [expected(c["root_3"].coeffs, i)[0] for i in (1, 2, 3, 4, 5)] == [0, 0, FV_IDENTITY, 0, 0]
    assert horner_events(c["root_3"].coeffs, 3) == [(0, "cancel")]
    assert [expected(c["roots_2_5"].coeffs, i)[0] for i in (1, 2, 3, 4, 5, 6)] == [0, FV_IDENTITY, 0, 0, FV_IDENTITY, 0]
    assert horner_events(c["ident_top"].coeffs, 2) == [(2, "inf_c"), (1, "inf_acc")]
    assert horner_events(c["ident_mid"].coeffs, 2) == [(1, "inf_c")]
    assert all(expected(c["ident_c0"].coeffs, i)[0] == (FV_KEY_IDENTITY if i else FV_ID) for i in c["ident_c0"].ids)
    assert len(set(expected(c["t1"].coeffs, i)[1] for i in IDS if i)) == 1  # every pubshare equals C_0
    assert expected(c["t1"].coeffs, 9)[1] == commit(c["t1"].coeffs[0])
    assert len(c["long_t170"].coeffs) == 170 and c["long_t170"].ids == [1, 2, 255]
    for case in CASES[:-1]:
        assert set(IDS) <= set(case.ids) and expected(case.coeffs, 0)[0] == FV_ID, case.name
    assert {len(case.coeffs) for case in CASES} == {1, 2, 3, 170}


_prove()


# ---------------------------------------------------------------------------
# one launch over every case
Launch = collections.namedtuple("Launch", "commit48 poly_first eval_poly eval_id want_status want_out case_of_poly")


@functools.lru_cache(None)
def launch():
    """The whole list as ONE call: the polynomials in an order that alternates
    their lengths, the evaluations round-robin over the polynomials so that
    failing, identity and ordinary lanes (and chains of every length) share
    waves.  n_evals is more than one workgroup and no multiple of 64."""
    order = sorted(range(len(CASES)), key=lambda i: (i % 2, i))  # t = 2, 3, 2, 3, ... next to 1 and 170
    polys = [CASES[i] for i in order]
    first = [0]
    for c in polys:
        first.append(first[-1] + len(c.coeffs))
    queues = [[(p, i) for i in c.ids] for p, c in enumerate(polys)]
    evals = []
    while any(queues):
        for q in queues:
            if q:
                evals.append(q.pop(0))
    if len(evals) % 64 == 0:
        evals.append((0, 1))
    want = [expected(polys[p].coeffs, i) for p, i in evals]
    assert len(evals) > 64 and len(evals) % 64 != 0
    st = [w[0] for w in want]
    assert {FV_OK, FV_ID, FV_KEY_IDENTITY, FV_IDENTITY} == set(st)
    assert all(len({s == FV_OK for s in st[k:k + 64]}) == 2 for k in range(0, len(st), 64))  # mixed in every wave
    return Launch(b"".join(b for c in polys for b in commits(c.coeffs)), first, [p for p, _ in evals],
                  [i for _, i in evals], st, [w[1] for w in want], [c.name for c in polys])


def random_polys(n, ts, seed):
    """n random polynomials (nonzero coefficients), t drawn from ts."""
    rng = random.Random(seed)
    return [[rng.randrange(1, R) for _ in range(rng.choice(ts))] for _ in range(n)]
