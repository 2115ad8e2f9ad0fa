"""Directed inputs for the hash-to-G2 kernel chain (k_hash.hip,
k_hash_clear.hip), shared by the CPU run through tests/hostcheck
(hc_map_pair_u, hc_sqrt_or_z; TBG_BOUNDS_CHECK on) and the GPU run through
tests/devcheck (dc_h2c, dc_h2c_sqrt; test_gpu_devcheck_h2c.py).  Deterministic.

The chain is entered stage by stage (dc_h2c's stages, STAGES below): from
message bytes, from injected field elements (u0, u1), from preloaded SSWU
slots, and from preloaded points in front of the cofactor clearing and of its
last kernel alone.  Values cross as raw limbs in canonical Montgomery form
(tests/edge_operands.py); expected values are Python integers from
oracle/bls12_381.py -- hash_to_g2, map_to_curve_g2, f2_is_square and the exact
group law -- and every result is compared exactly, as an affine point
(tests/edge_points.py point_of).  There are no tolerances.

Every list fills more than one wave of its kernels' lanes (or lane pairs) and
ends in a partly filled one; rare and ordinary items alternate, so
neighbouring lanes and pairs take different branches.  The rare branches the
lists are for, and the list that reaches each:
  * k_hash_map's `ok == false` (an SSWU denominator is zero) and, through it,
    k_hash_sswu's fallback to map_to_curve_g2: u_pairs (0, r), (r, 0), (0, 0);
  * k_hash_sswu's fallback after fp2_sqrt_or_z_in refused, and the slot's u
    still intact for it: sswu_slots (flag 1, g(x1) in Fp);
  * both `return false` exits of fp2_sqrt_or_z_in and both arms of its final
    select: sqrt_values;
  * px_add_complete_at(.., psi = false) in k_hash_clear_x1 (Q0 == Q1):
    u_pairs (u, u), (0, 0) and clear_pairs' doublings;
  * px_add_complete_at(.., psi = true) (t1 == psi(P): Q0 + Q1 in G2, where
    psi acts as [x]): clear_pairs' G2 sums;
  * clear_fin_complete, from each of k_hash_clear_fin's four additions:
    fin_triples (no point of E2[13] reaches it through the whole chain).
NOT reached: px_mul_x_complete.  Its doubling case needs the running multiple
[k]P to meet P at one of the five additions of [|x|]P, i.e. a point whose
order divides 11, 103, 53759 or 230901736800255 (the prefixes of |x| minus
one); all four are coprime to #E2(Fp2), so no point of the curve gets there,
and no off-curve input is invented for it.
"""
import functools
import random

from oracle import bls12_381 as bls
from tests import edge_operands as eo
from tests.edge_points import XLaw, add, bank, jac, jac_words, mul, neg, point_of, psi

P = bls.P
NL = eo.NL
SENT = eo.SENTINEL
FP2_W, AFF_W, JAC_W = 2 * NL, 4 * NL, 6 * NL
STAGES = ["MAP_MSG", "MAP_U", "SSWU", "CLEAR_X1", "CLEAR_X2", "CLEAR_FIN", "AFFINE"]
Z = bls.SSWU_Z
# bls_constants.h SSWU_SQRT_NEG_NORM_Z: the root K of -norm(Z) that fp2_sqrt_or_z_in multiplies gamma by
K_SQRT = eo.unmont([0xa300f16, 0xb5407f4, 0xf2e0189, 0x109f289, 0xd163476, 0xd082982, 0x2514131, 0x572eaf2,
                    0x257fc31, 0x8076e7b, 0x27e19ba, 0x2e91e67, 0x40ab7bb, 0x000f077])
assert K_SQRT * K_SQRT % P == P - 5


# ---------------------------------------------------------------------------
# limbs
def fp2_words(a):
    return eo.mont(a[0] % P) + eo.mont(a[1] % P)


def f2_of(words):
    """The Fp2 value of 28 result words, or a string saying what is wrong."""
    w = [int(v) for v in words]
    if len(w) != FP2_W:
        return "wrong length"
    if any(not 0 <= v <= eo.M28 for v in w):
        return "limbs not below 2^28"
    return (eo.unmont(w[:NL]), eo.unmont(w[NL:]))


def aff_of(words):
    """The affine point of 56 result words (the value of each coordinate
    below 2p), or a string."""
    w = [int(v) for v in words]
    if len(w) != AFF_W:
        return "wrong length"
    if any(eo.val(w[i * NL:(i + 1) * NL]) >= 2 * P for i in range(4)):
        return "coordinate not below 2p"
    x, y = f2_of(w[:FP2_W]), f2_of(w[FP2_W:])
    return x if isinstance(x, str) else y if isinstance(y, str) else (x, y)


def _rand_f2(rng):
    return (rng.randrange(1, P), rng.randrange(1, P))


def _alternate(rare, ordinary, n):
    """n items: the rare ones at the odd positions until they run out, the
    ordinary ones (cycled) everywhere else."""
    rare, out, k = list(rare), [], 0
    for i in range(n):
        if i % 2 == 1 and rare:
            out.append(rare.pop(0))
        else:
            out.append(ordinary[k % len(ordinary)])
            k += 1
    assert not rare
    return out


# ---------------------------------------------------------------------------
# the oracle's side
@functools.lru_cache(None)
def map_point(u):
    return bls.map_to_curve_g2(u)


def sswu_x1(u):
    """x1 of the SSWU map (None where the denominator is zero)."""
    zu2 = bls.f2_mul(Z, bls.f2_sqr(u))
    den = bls.f2_add(bls.f2_sqr(zu2), zu2)
    if bls.f2_is_zero(den):
        return None
    return bls.f2_mul(bls.f2_mul(bls.f2_neg(bls.SSWU_B), bls.f2_inv(bls.SSWU_A)), bls.f2_add(bls.F2_ONE, bls.f2_inv(den)))


def sswu_gx(x1):
    return bls.f2_add(bls.f2_add(bls.f2_mul(bls.f2_sqr(x1), x1), bls.f2_mul(bls.SSWU_A, x1)), bls.SSWU_B)


def gx1_is_square(u):
    return bls.f2_is_square(sswu_gx(sswu_x1(u)))


def mul_x(p):
    """[x] p for the (negative) curve parameter x."""
    return neg(mul(p, bls.X_ABS))


@functools.lru_cache(None)
def clear_steps(p):
    """What the three clearing kernels leave for P = Q0 + Q1, by the exact
    law: t1 = [x]P, v = [x](t1 + psi(P)), h = psi^2(2P) - t1 + v - psi(P) - P."""
    t1 = mul_x(p)
    v = mul_x(add(t1, psi(p)))
    return t1, v, fin_value(p, t1, v)


def fin_value(p, t1, v):
    h = add(psi(psi(add(p, p))), neg(t1))
    h = add(h, v)
    h = add(h, neg(psi(p)))
    return add(h, neg(p))


def clear_formula(p):
    """[x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2P)  (RFC 9380 G.3)."""
    x = bls.X_ABS
    h = add(mul(p, x * x + x - 1), neg(mul(psi(p), x + 1)))
    return add(h, psi(psi(add(p, p))))


def clear_sites(q0, q1):
    """Which of k_hash_clear_x1's additions without a doubling branch meet
    their doubling case for Q0, Q1 ("sum": Q0 + Q1, "psi": t1 + psi(P),
    "mul": inside [x] P or [x] u), over the exact law."""
    sites = set()
    x = XLaw()
    x.add(q0, q1)
    if x.exc:
        sites.add("sum")
    p = add(q0, q1)
    x = XLaw()
    t1 = neg(x.mul_xabs(p))
    if x.exc:
        sites.add("mul")
    x = XLaw()
    x.add(t1, psi(p))
    if x.exc:
        sites.add("psi")
    x = XLaw()
    x.mul_xabs(add(mul_x(p), psi(p)))
    if x.exc:
        sites.add("mul")
    return sites


def fin_sites(p, t1, v):
    """Which of k_hash_clear_fin's four additions meet their doubling case
    (1: - t1, 2: + v, 3: - psi(P), 4: - P), in the kernel's order; after one
    the running sum is infinity, as jac_add_x returns it."""
    sites = set()
    t3 = psi(psi(add(p, p)))
    for k, operand in enumerate((neg(t1), v, neg(psi(p)), neg(p)), 1):
        x = XLaw()
        t3 = x.add(t3, operand)
        if x.exc:
            sites.add(k)
    return sites


# ---------------------------------------------------------------------------
# messages (MAP_MSG .. AFFINE against hash_to_g2)
MSG_LENGTHS = list(range(20)) + [31, 32, 33, 63, 64, 65, 71, 72, 73, 127, 128, 136, 200, 255, 300]
MSG_BATCHES = [1, 63, 64, 65, 130]


@functools.lru_cache(None)
def messages():
    """130 messages: two of every length, short and long ones side by side
    (neighbouring lanes compress different numbers of blocks); the smaller
    batches are prefixes of this list."""
    rng = random.Random(0x42C)
    lens = sorted(MSG_LENGTHS)
    order = [l for pair in zip(lens[:len(lens) // 2 + 1], reversed(lens)) for l in pair][:len(lens)]
    assert sorted(order) == lens
    pool = [bytes(rng.randrange(256) for _ in range(l)) for l in order + order[::-1]]
    out = [pool[i % len(pool)] for i in range(max(MSG_BATCHES))]
    assert {len(m) for m in out[:63]} == set(MSG_LENGTHS)
    return out


@functools.lru_cache(None)
def hash_point(msg):
    return bls.hash_to_g2(msg)


# ---------------------------------------------------------------------------
# (u0, u1) pairs (MAP_U .. SSWU, MAP_U .. AFFINE)
@functools.lru_cache(None)
def u_pairs():
    """[(kind, u0, u1)], 67 items: more than one BINV_BLOCK workgroup, the
    second partly filled."""
    rng = random.Random(0x0C0FFEE)
    want = {(a, b): 3 for a in (True, False) for b in (True, False)}
    ordinary = []
    while any(want.values()):
        u0, u1 = _rand_f2(rng), _rand_f2(rng)
        k = (gx1_is_square(u0), gx1_is_square(u1))
        if want[k]:
            want[k] -= 1
            ordinary.append(("sq%d%d" % k, u0, u1))
    r = [_rand_f2(rng) for _ in range(12)]
    rare = [("zero_u0", (0, 0), r[0]), ("fp", (rng.randrange(1, P), 0), r[1]), ("same", r[2], r[2]),
            ("zero_u1", r[3], (0, 0)), ("imag", (0, rng.randrange(1, P)), r[4]), ("opposite", r[5], bls.f2_neg(r[5])),
            ("zero_both", (0, 0), (0, 0)), ("one", (1, 0), r[6]), ("same", r[7], r[7]),
            ("minus_one", (P - 1, 0), r[8]), ("opposite", bls.f2_neg(r[9]), r[9]), ("fp", r[10], (rng.randrange(1, P), 0)),
            ("imag", r[11], (0, rng.randrange(1, P))), ("zero_u0", (0, 0), r[2]), ("one", r[3], (1, 0)),
            ("minus_one", r[4], (P - 1, 0))]
    return _alternate(rare, ordinary, 67)


def u_words(pairs):
    return [w for _, u0, u1 in pairs for w in fp2_words(u0) + fp2_words(u1)]


# ---------------------------------------------------------------------------
# SSWU slots (SSWU alone): X = u, Y = x1, Z.c0.l[0] = the flag
X1_REAL_GX = ((-1012 * pow(240, -1, P)) % P, 0)  # g(x1) lies in Fp: the closed-form root refuses


@functools.lru_cache(None)
def sswu_slots():
    """[(kind, u, x1, flag)], 70 maps (35 messages): more than one wave of
    k_hash_sswu's lanes, the second partly filled."""
    rng = random.Random(0x55AA)
    ordinary = []
    for _ in range(8):
        u = _rand_f2(rng)
        ordinary.append(("ordinary", u, sswu_x1(u), 1))
    r = [_rand_f2(rng) for _ in range(12)]
    rare = [("no_inverse", r[0], _rand_f2(rng), 0), ("real_gx", r[1], X1_REAL_GX, 1),
            ("no_inverse", (0, 0), (0, 0), 0), ("real_gx", r[2], X1_REAL_GX, 1),
            ("no_inverse", r[3], sswu_x1(r[3]), 0), ("real_gx", (5, 0), X1_REAL_GX, 1),
            ("no_inverse", (0, 0), _rand_f2(rng), 0), ("real_gx", r[4], X1_REAL_GX, 1),
            ("no_inverse", r[5], X1_REAL_GX, 0), ("real_gx", (0, 7), X1_REAL_GX, 1),
            ("no_inverse", r[6], (0, 0), 0), ("real_gx", r[7], X1_REAL_GX, 1)]
    return _alternate(rare, ordinary, 70)


def sswu_slot_words(slot):
    _, u, x1, flag = slot
    return fp2_words(u) + fp2_words(x1) + [flag] + [SENT] * (FP2_W - 1)


# ---------------------------------------------------------------------------
# square-root values (dc_h2c_sqrt / hc_sqrt_or_z)
def sqrt_model(a):
    """(flag, sq, arm) of fp2_sqrt_or_z_in on a: sq = a is a square; the flag
    is false when the value whose root is taken (a, or Z a) lies in Fp; arm:
    whether delta = (c0 + gamma) / 2 is a residue (None without a root)."""
    sq = bls.f2_is_square(a)
    t = a if sq else bls.f2_mul(Z, a)
    if t[1] == 0:
        return False, sq, None
    gamma = pow((a[0] * a[0] + a[1] * a[1]) % P, (P + 1) // 4, P)
    if not sq:
        gamma = gamma * K_SQRT % P
    delta = (t[0] + gamma) * pow(2, -1, P) % P
    return True, sq, pow(delta, (P - 1) // 2, P) == 1


@functools.lru_cache(None)
def sqrt_values():
    """[(kind, a)], 70 values: more than one wave, the second partly filled."""
    rng = random.Random(0x5C27)
    zi = bls.f2_inv(Z)
    want = {(sq, arm): 3 for sq in (True, False) for arm in (True, False)}
    ordinary = []
    while any(want.values()):
        a = _rand_f2(rng)
        _, sq, arm = sqrt_model(a)
        if want[(sq, arm)]:
            want[(sq, arm)] -= 1
            ordinary.append(("sq%d_arm%d" % (sq, arm), a))
    s = rng.randrange(2, P)
    nonres = next(v for v in range(2, 50) if pow(v, (P - 1) // 2, P) != 1)
    rare = [("zero", (0, 0)), ("fp_square", (s * s % P, 0)), ("fp_nonresidue", (nonres, 0)),
            ("imaginary", (0, rng.randrange(1, P))), ("imaginary", (0, 1)), ("fp_square", (1, 0)),
            ("fp_nonresidue", (P - 1, 0))]
    rare += [("over_z", bls.f2_muls(zi, t)) for t in (1, 2, P - 1, s, rng.randrange(1, P), nonres)]
    return _alternate(rare, ordinary, 70)


def check_sqrt(a, flag_word, root_words):
    """None, or what is wrong with the thin kernel's result for a."""
    flag, sq, _ = sqrt_model(a)
    if flag_word != (int(flag) | int(sq) << 1):
        return f"flags {flag_word}, expected done {int(flag)} sq {int(sq)}"
    r = f2_of(root_words)
    if isinstance(r, str):
        return r
    if not flag:
        return None if list(root_words) == [0] * FP2_W else "a root was written"
    a = (a[0] % P, a[1] % P)
    return None if bls.f2_sqr(r) == (a if sq else bls.f2_mul(Z, a)) else "root^2 differs"


# ---------------------------------------------------------------------------
# points in front of the cofactor clearing (CLEAR_X1 .. AFFINE)
@functools.lru_cache(None)
def clear_pairs():
    """[(kind, Q0, Q1)], 37 pairs of points: more than one wave of lane
    pairs, the second partly filled."""
    b = bank()
    g, ns, t13, t23, tor = b["g"], b["ns"], b["t13"], b["t23"], b["tor"]
    ordinary = [("generic", ns, t13), ("generic", t23, tor), ("generic", tor, ns), ("generic", t13, t23),
                ("generic", ns, g[5]), ("generic", t13, tor)]
    rare = [("double", ns, ns), ("g2_sum", g[0], g[1]), ("cancel", t13, neg(t13)), ("inf_q0", None, t23),
            ("double", t13, t13), ("g2_sum", g[2], neg(g[3])), ("inf_q1", tor, None), ("inf_both", None, None),
            ("double", g[4], g[4]), ("g2_sum", None, g[6]), ("cancel", g[7], neg(g[7])), ("inf_q1", ns, None),
            ("double", tor, tor), ("g2_sum", g[1], g[1]), ("inf_q0", None, t13)]
    return _alternate(rare, ordinary, 37)


# ... and in front of its last kernel alone (CLEAR_FIN): P, t1, v arbitrary
@functools.lru_cache(None)
def fin_triples():
    """[(kind, P, t1, v)], 37 triples; "addN": the running sum equals the
    operand of k_hash_clear_fin's N-th addition."""
    b = bank()
    g, ns, t13, t23, tor = b["g"], b["ns"], b["t13"], b["t23"], b["tor"]
    ordinary = [("generic", ns, t13, t23), ("generic", t23, g[0], ns), ("generic", g[1], tor, t13),
                ("generic", t13, None, g[2]), ("generic", None, ns, tor), ("generic", tor, t23, None)]

    def pp2(p):
        return psi(psi(add(p, p)))

    rare = []
    for p, t1 in ((ns, t13), (t23, g[3]), (g[4], ns)):
        rare.append(("add1", p, neg(pp2(p)), t1))                                           # psi^2(2P) == -t1
        rare.append(("add2", p, t1, add(pp2(p), neg(t1))))                                  # ... - t1 == v
        rare.append(("add3", p, t1, add(neg(psi(p)), add(neg(pp2(p)), t1))))                # ... + v == -psi(P)
        rare.append(("add4", p, t1, add(add(neg(p), psi(p)), add(neg(pp2(p)), t1))))        # ... - psi(P) == -P
    return _alternate(rare, ordinary, 37)


def point_words(rng, a):
    """A point in a random Jacobian form, canonical limbs."""
    return jac_words(jac(a, _rand_f2(rng)))


# ---------------------------------------------------------------------------
# the checker
def check_jac(words, want):
    """None, or what is wrong with a Jacobian result slot."""
    got = point_of(words)
    if isinstance(got, str):
        return got
    if got != want:
        return "point differs" if got is not None and want is not None else \
            f"infinity: got {got is None}, expected {want is None}"
    return None


def check_affine(words, status, want):
    """None, or what is wrong with k_hash_affine's output for the point
    `want`: status 0 and that point, or status 1 and all-zero words."""
    if want is None:
        if status != 1:
            return f"status {status}, expected 1"
        return None if list(words) == [0] * AFF_W else "h_aff not zero for the identity"
    if status != 0:
        return f"status {status}, expected 0"
    got = aff_of(words)
    if isinstance(got, str):
        return got
    return None if got == want else "affine point differs"
