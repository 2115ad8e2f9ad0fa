"""Directed operand lists for the field arithmetic, shared by the CPU run
through tests/hostcheck (test_devcheck_operands.py, TBG_BOUNDS_CHECK on: a
violated precondition aborts) and the GPU run through tests/devcheck
(test_gpu_devcheck.py).  Deterministic: fixed seeds for the random tails.

Values are RAW limb vectors -- 14 limbs of 28 bits, plain (unsigned, possibly
lazy: limbs < 2^31) or row form (signed redundant).  The arithmetic is
Montgomery with R = 2^392, so a product of raw values a, b is a b / R; no
conversion is needed to state what an operation must return.  The result
checkers live here too: each returns None or a string saying what is wrong.
"""
import functools
import random

from oracle import bls12_381 as bls

P = bls.P
NL = 14
R = 1 << 392
RINV = pow(R, -1, P)
M28 = (1 << 28) - 1
P16 = 16 * P
TOP_P = P >> 364  # floor(p / 2^364): p's top limb


# ---------------------------------------------------------------------------
# limb forms
def limbs(x):
    """Normalised limbs of 0 <= x < 2^396 (the top limb takes the excess)."""
    assert 0 <= x < (1 << 396)
    return [(x >> (28 * j)) & M28 for j in range(NL - 1)] + [x >> (28 * (NL - 1))]


def val(l):
    return sum(int(v) << (28 * j) for j, v in enumerate(l[:NL]))


def lazy(x):
    """The same value with un-propagated carries: every limb borrows up to 7
    units from the one above, pushing limbs towards 2^31 - 1."""
    l = limbs(x)
    for j in range(NL - 2, -1, -1):
        k = min(7, l[j + 1])
        l[j] += k << 28
        l[j + 1] -= k
    assert val(l) == x and max(l) < (1 << 31)
    return l


def signed_limbs(x):
    """Sign-magnitude row limbs of a signed value."""
    l = limbs(abs(x))
    return [-v for v in l] if x < 0 else l


def mont(x):
    return limbs(x * R % P)


def unmont(l):
    return val(l) * RINV % P


# ---------------------------------------------------------------------------
# host-side preconditions (bls_field.h's TBG_BOUNDs, in exact integers with a
# margin for the header's double estimates)
def columns_fit(*pairs):
    col = sum(14 * max(a) * max(b) for a, b in pairs)
    return col + 14 * (1 << 56) + (1 << 36) < (1 << 64)


def product_bound(*pairs):
    return sum(val(a) * val(b) for a, b in pairs) * 1001 < 2048 * P * P * 1000


def mul_ok(*pairs):
    return columns_fit(*pairs) and product_bound(*pairs)


def sqr_ok(a):
    return 16 * max(a) * max(a) + 14 * (1 << 56) + (1 << 36) < (1 << 64) and product_bound((a, a))


def sub_ok(a, b):  # a + 16p - b
    return max(b) <= M28 and val(b) * 1001 <= P16 * 1000 and max(a) < (1 << 31) and val(a) + P16 < (1 << 392)


def reduce_ok(a):
    return a[NL - 1] < (1 << 26) and max(a) < (1 << 31)


# ---------------------------------------------------------------------------
# plain Fp
EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (1 << 380) % P, (1 << 381) - 1 - P]
CANON_EDGES = EDGE + [(P + 1) // 2, 1 << 380, (1 << 381) % P]
TOP_2P = 2 * TOP_P - 1  # with every lower limb at its maximum the value stays below 2p


def _patterns(top):
    """Limb patterns over limbs 0..12 with the given top limb."""
    alt0 = [M28 if j % 2 == 0 else 0 for j in range(NL - 1)]
    alt1 = [M28 if j % 2 == 1 else 0 for j in range(NL - 1)]
    return [[0] * 13 + [top], [M28] * 13 + [top], alt0 + [top], alt1 + [top]]


def _single_limbs():
    out = []
    for j in range(NL - 1):
        l = [0] * NL
        l[j] = M28
        out.append(l)
    l = [0] * NL
    l[NL - 1] = TOP_2P
    out.append(l)
    return out


Q_MAX = ((1 << 390) - 2) // P  # the largest q with q p + 1 < 2^390


def _qp_values(qs):
    out = []
    for q in qs:
        for d in (-1, 0, 1):
            v = q * P + d
            if 0 <= v < (1 << 390) and v not in out:
                out.append(v)
    return out


@functools.lru_cache(None)
def fp_normal():
    """Normalised operands below 32p (the product / sum domain)."""
    rng = random.Random(0xF1E1D)
    vs = [limbs(v) for v in CANON_EDGES]
    for top in (0, TOP_P - 1, TOP_2P):
        vs += _patterns(top)
    vs += _single_limbs()
    vs += [limbs(v) for v in _qp_values([1, 2, 4, 8, 15, 16, 30])]
    vs += [limbs(rng.randrange(P)) for _ in range(40)]
    out = []
    for l in vs:
        if l not in out:
            out.append(l)
    return out


@functools.lru_cache(None)
def fp_reduce_values():
    """fp_reduce / fp_canon inputs: the quotient estimate on and beside every
    multiple of p it must tell apart, normalised and lazy, up to the a < 2^390
    limit; the limb patterns at the largest legal top limb."""
    qs = [0, 1, 2] + [1 << k for k in range(2, 10) if (1 << k) <= Q_MAX] + [Q_MAX - 1, Q_MAX]
    out = []
    for v in _qp_values(qs):
        out.append(limbs(v))
        lz = lazy(v)
        if lz != out[-1]:
            out.append(lz)
    for top in (0, TOP_P, (1 << 26) - 1):
        out += _patterns(top)
    out += [[(1 << 31) - 1] * 13 + [(1 << 26) - 9]]  # (the lazy limbs carry 8 units into the top: still < 2^390)
    out += fp_normal()[:len(CANON_EDGES)] + fp_normal()[-40:]
    assert all(reduce_ok(a) and val(a) < (1 << 390) for a in out)
    return out


@functools.lru_cache(None)
def fp_lazy():
    """Lazy product operands: limbs up to the documented 2^31 bound."""
    out = [[(1 << 31) - 1] * 13 + [t] for t in (0, TOP_P, 30 * TOP_P)]
    out += [[(1 << 31) - 1 if j % 2 == 0 else 0 for j in range(13)] + [TOP_P]]
    out += [lazy(v) for v in _qp_values([1, 2, 16, 30])]
    out += [lazy(val(a)) for a in fp_normal()[-6:]]
    return out


def _subset(vs, k, seed):
    rng = random.Random(seed)
    return vs[:k] + rng.sample(vs[k:], min(8, max(0, len(vs) - k)))


@functools.lru_cache(None)
def fp_cases():
    """op name -> list of operand tuples (limb vectors; mul_small: (a, k))."""
    N, L = fp_normal(), fp_lazy()
    B = _subset(N, 27, 1)
    rng = random.Random(0xCA5E5)
    c = {}
    c["mul"] = [(a, b) for a in N for b in B[::3] if mul_ok((a, b))]
    c["mul"] += [(a, b) for a in L for b in B if mul_ok((a, b))]
    c["mul"] += [(b, a) for a in L for b in B[::4] if mul_ok((a, b))]
    c["sqr"] = [(a,) for a in N + L if sqr_ok(a)]
    m2 = []
    for i, a in enumerate(N + L):
        b, cc, d = B[i % len(B)], (N + L)[(i * 7 + 3) % len(N + L)], B[(i * 5 + 1) % len(B)]
        for t in ((a, b, cc, d), (a, b, a, b), (b, a, d, cc)):
            if mul_ok((t[0], t[1]), (t[2], t[3])):
                m2.append(t)
    c["mul2"] = m2
    pairs = [(a, b) for a in N for b in B[::2]]
    c["add"] = [(a, b) for a, b in pairs if val(a) + val(b) < (1 << 392)]
    c["sub"] = [(a, b) for a, b in pairs if sub_ok(a, b)] + [(a, b) for a in L for b in B[::2] if sub_ok(a, b)]
    c["neg"] = [(a,) for a in N if sub_ok([0] * NL, a)]
    third = [N[(3 * i + 1) % len(N)] for i in range(len(pairs))]
    c["addl_mul"] = [(a, b, t) for (a, b), t in zip(pairs, third)
                     if val(t) < 2 * P and mul_ok(([x + y for x, y in zip(a, b)], t))]
    c["subl_mul"] = [(a, b, t) for (a, b), t in zip(pairs, third)
                     if val(t) < 2 * P and sub_ok(a, b)
                     and mul_ok(([x + s - y for x, y, s in zip(a, b, limbs_sub16p())], t))]
    c["negl_mul"] = [(a, b) for a, b in pairs
                     if sub_ok([0] * NL, b) and mul_ok((a, [s - y for y, s in zip(b, limbs_sub16p())]))]
    c["mul_small"] = [(a, k) for k in (2, 3, 8, 12) for a in N + L if val(a) * k < (1 << 392)]
    c["reduce"] = [(a,) for a in fp_reduce_values()]
    c["canon"] = [(a,) for a in fp_reduce_values()]
    inv = [a for a in N if val(a) < 32 * P]
    c["inv"] = [(a,) for a in inv]
    c["inv_fermat"] = [(a,) for a in inv[:24] + inv[-6:]]
    fs = [signed_limbs(s * v) for v in (0, 1, P - 1, P, P + 1, 2 * P - 1, 4 * P, 8 * P - 1) for s in (1, -1)]
    fs += [[s * ((1 << 31) - 1)] * 13 + [0] for s in (1, -1)]
    fs += [[((1 << 31) - 1) * (1 if j % 2 else -1) for j in range(13)] + [t] for t in (0, TOP_P, -TOP_P)]
    fs += [row for row in row_values() if abs(val(row)) < 8 * P][:40]
    fs += [signed_limbs(rng.randrange(-8 * P + 1, 8 * P)) for _ in range(20)]
    c["from_signed"] = [(a,) for a in fs]
    # the sign rule's comparison c > (p - 1) / 2 on and beside its boundary (no decodable point puts a y
    # there): Montgomery forms of the canonical value, canonical limbs and the same plus p
    lex = LEX_EDGES + [(P - 3) // 2, (P + 3) // 2, 2, P - 2] + [rng.randrange(P) for _ in range(8)]
    c["lex"] = [(mont(v),) for v in lex] + [(limbs(v * R % P + P),) for v in lex]
    return c


LEX_EDGES = [0, 1, (P - 1) // 2, (P + 1) // 2, P - 1]


def limbs_sub16p():
    """SUB16P_L: 16p with every limb but the top one >= 2^28 - 1."""
    l = limbs(P16)
    # move one unit of limb j + 1 down into limb j (top to bottom)
    for j in range(NL - 2, -1, -1):
        l[j + 1] -= 1
        l[j] += 1 << 28
    assert val(l) == P16 and min(l[:NL - 1]) >= M28
    return l


def fp_expect(op, t):
    """('mod', residue, hi) -- limbs < 2^28, value in [0, hi), value = residue
    mod p -- or ('exact', value): limbs 0..12 < 2^28 and that exact value."""
    v = [val(x) if isinstance(x, list) else x for x in t]
    if op == "mul":
        return ("mod", v[0] * v[1] * RINV, 2 * P)
    if op == "mul2":
        return ("mod", (v[0] * v[1] + v[2] * v[3]) * RINV, 2 * P)
    if op == "sqr":
        return ("mod", v[0] * v[0] * RINV, 2 * P)
    if op == "add":
        return ("exact", v[0] + v[1])
    if op == "sub":
        return ("exact", v[0] + P16 - v[1])
    if op == "neg":
        return ("exact", P16 - v[0])
    if op == "addl_mul":
        return ("mod", (v[0] + v[1]) * v[2] * RINV, 2 * P)
    if op == "subl_mul":
        return ("mod", (v[0] + P16 - v[1]) * v[2] * RINV, 2 * P)
    if op == "negl_mul":
        return ("mod", v[0] * (P16 - v[1]) * RINV, 2 * P)
    if op == "mul_small":
        return ("exact", v[0] * v[1])
    if op == "reduce":
        return ("mod", v[0], 2 * P)
    if op == "canon":
        return ("mod", v[0], P)
    if op in ("inv", "inv_fermat"):  # Montgomery inverse: (x R)^-1 R^2; 0 -> 0
        return ("mod", pow(v[0], P - 2, P) * R * R, 2 * P)
    if op == "from_signed":
        return ("mod", v[0], 2 * P)
    if op == "lex":  # fp_lex_largest_canon(fp_from_mont(a)): 1 or 0 in word 0
        return ("exact", int(v[0] * RINV % P > (P - 1) // 2))
    raise KeyError(op)


def check_plain(l, expect):
    """A plain result (14 words) against fp_expect's description."""
    l = [int(x) for x in l]
    if len(l) != NL:
        return "not 14 limbs"
    if expect[0] == "exact":
        if any(not 0 <= x <= M28 for x in l[:NL - 1]) or not 0 <= l[NL - 1] < (1 << 32):
            return f"limbs not normalised: {l}"
        if val(l) != expect[1]:
            return f"value {val(l):#x} != {expect[1]:#x}"
        return None
    _, residue, hi = expect
    if any(not 0 <= x <= M28 for x in l):
        return f"limbs not below 2^28: {l}"
    v = val(l)
    if not 0 <= v < hi:
        return f"value {v:#x} outside [0, {hi:#x})"
    if (v - residue) % P:
        return f"value {v:#x} has the wrong residue (want {residue % P:#x})"
    return None


# ---------------------------------------------------------------------------
# row Fp (signed redundant limbs)
@functools.lru_cache(None)
def row_values():
    M, B, C = M28, 1 << 28, 1 << 29
    pats = [[M] * 13, [-M] * 13, [M if j % 2 == 0 else -M for j in range(13)], [B] * 13, [C] * 13, [-C] * 13,
            [C if j % 2 == 0 else -C for j in range(13)], [-C if j % 2 == 0 else C for j in range(13)]]
    tops = [0, 1, -1, TOP_P, -TOP_P, 2 * TOP_P, 4 * TOP_P, -4 * TOP_P, 30 * TOP_P, -30 * TOP_P]
    return [p + [t] for p in pats for t in tops]


def row_pair_ok(*pairs):
    return sum(abs(val(a) * val(b)) for a, b in pairs) * 1001 < 2048 * P * P * 1000


@functools.lru_cache(None)
def row_cases():
    V = row_values()
    n = len(V)
    rng = random.Random(0x2070)
    rnd = [signed_limbs(rng.randrange(-2 * P, 2 * P)) for _ in range(40)]
    c = {}
    c["mul2"] = [t for t in ((V[i], V[j], V[(i + 3) % n], V[(j + 5) % n]) for i in range(n) for j in range(n))
                 if row_pair_ok((t[0], t[1]), (t[2], t[3]))]
    c["mul2"] += [(rnd[i], rnd[(i + 1) % 40], rnd[(i + 2) % 40], rnd[(i + 3) % 40]) for i in range(40)]
    c["mul"] = [(V[i], V[j]) for i in range(n) for j in range(i % 7, n, 7) if row_pair_ok((V[i], V[j]))]
    c["mul"] += [(rnd[i], rnd[(i + 5) % 40]) for i in range(40)]
    red = [v for v in V if abs(val(v)) < (1 << 388)]
    for q in list(range(-40, 41)) + [127, -128]:
        for d in (-1, 0, 1):
            red.append(signed_limbs(q * P + d))
    red += [signed_limbs(rng.randrange(-(1 << 388), 1 << 388)) for _ in range(40)]
    c["reduce"] = [(a,) for a in red]
    c["norm"] = [(a,) for a in V + rnd]
    return c


def row_expect(op, t):
    v = [val(x) for x in t]
    if op == "mul":
        return ("mod", v[0] * v[1] * RINV)
    if op == "mul2":
        return ("mod", (v[0] * v[1] + v[2] * v[3]) * RINV)
    if op == "reduce":
        return ("mod", v[0])
    if op == "norm":
        return ("exact", v[0])
    raise KeyError(op)


def check_row(w, expect):
    """A row result, 16 words (lane j's value; lanes 14, 15 must hold 0)."""
    w = [int(x) for x in w]
    if len(w) != 16:
        return "not 16 words"
    if w[14] or w[15]:
        return f"lanes 14, 15 hold {w[14]}, {w[15]}"
    if any(abs(x) > (1 << 28) for x in w[:NL - 1]):
        return f"|limb| above 2^28: {w}"
    v = val(w)
    if expect[0] == "exact":
        return None if v == expect[1] else f"value {v:#x} != {expect[1]:#x}"
    if not -P < v < 2 * P:
        return f"value {v:#x} outside (-p, 2p)"
    if (v - expect[1]) % P:
        return f"value {v:#x} has the wrong residue"
    return None


# ---------------------------------------------------------------------------
# Fp12 (oracle tuples ((c00, c01, c02), (c10, c11, c12)) of Fp2 pairs)
def _coeff(i, c):
    cs = [bls.F2_ZERO] * 6
    cs[i] = c
    return (tuple(cs[:3]), tuple(cs[3:]))


def easy_part(a):
    f = bls.f12_mul(bls.f12_conj(a), bls.f12_inv(a))
    return bls.f12_mul(bls.f12_frob_n(f, 2), f)


F12_ZERO = ((bls.F2_ZERO,) * 3, (bls.F2_ZERO,) * 3)


@functools.lru_cache(None)
def f12_values():
    """name -> element.  'cancel': e(P, Q) e(-P, Q) before the final
    exponentiation (it must exponentiate to 1); 'pairing': one Miller value."""
    rng = random.Random(0xF12)

    def rnd():
        return tuple(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3)) for _ in range(2))

    d = {"zero": F12_ZERO, "one": bls.F12_ONE}
    for i in range(6):
        d[f"coeff{i}"] = _coeff(i, (rng.randrange(1, P), rng.randrange(1, P)))
    d["pm1"] = (((P - 1, P - 1),) * 3, ((P - 1, P - 1),) * 3)
    d["cyclo"] = easy_part(rnd())
    p = bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R))
    q = bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))
    m1, m2 = bls.miller_loop(p, q), bls.miller_loop(bls.g1_neg(p), q)
    d["cancel"] = bls.f12_mul(m1, m2)
    d["pairing"] = m1
    for i in range(6):
        d[f"rand{i}"] = rnd()
    return d


def f12_to_quad(f):
    """The 12 Fp in trio / row order: A_q = (a.c0, a.c1, b.c0, b.c1) at 4 q, A0 =
    (c0.c0, c1.c1), A1 = (c1.c0, c0.c2), A2 = (c0.c1, c1.c2)  (bls_quad.h)."""
    (c00, c01, c02), (c10, c11, c12) = f
    out = []
    for a, b in ((c00, c11), (c10, c02), (c01, c12)):
        out += [a[0], a[1], b[0], b[1]]
    return out


def quad_to_f12(v):
    A = [((v[4 * q], v[4 * q + 1]), (v[4 * q + 2], v[4 * q + 3])) for q in range(3)]
    return ((A[0][0], A[2][0], A[1][1]), (A[1][0], A[0][1], A[2][1]))


def check_f12(fp_values, expect):
    """12 residues (already reduced mod p, Montgomery factor removed) in quad
    order against an oracle element."""
    got = quad_to_f12([int(x) % P for x in fp_values])
    return None if got == expect else f"Fp12 differs from the oracle: {got} != {expect}"


def line_f12(l0, l1, l4):
    """The sparse line (l0, l1, l4) as an Fp12 element (quad_line_lane)."""
    return ((l0, l1, bls.F2_ZERO), (bls.F2_ZERO, l4, bls.F2_ZERO))


def check_flag(got, want):
    return None if int(got) == int(bool(want)) else f"flag {got} != {int(bool(want))}"


def check_lines(got_words, ref_words):
    """Two line tables (plain limbs), Fp for Fp modulo p."""
    if len(got_words) != len(ref_words) or len(got_words) % NL:
        return "line tables differ in size"
    for i in range(0, len(got_words), NL):
        g, r = [int(x) for x in got_words[i:i + NL]], [int(x) for x in ref_words[i:i + NL]]
        if any(not 0 <= x <= M28 for x in g):
            return f"Fp {i // NL}: limbs not below 2^28"
        if (val(g) - val(r)) % P:
            return f"Fp {i // NL} (line {i // (6 * NL)}) differs"
    return None


# ---------------------------------------------------------------------------
# occupancy
HEX_COUNTS = [1, 4, 5, 6, 9, 10, 11, 23]
ROW_CHUNK = 400          # rows per 64-thread-block launch (the last launch of a list is partly empty)
ROW_BLOCK_ROWS = 36      # rows of the single 576-thread workgroup
BATCH_INV_SIZES = [1, 64, 65, 129, 256, 300]
SENTINEL = 0xA5C3F00D


def batch_inv_case(n, seed=0xB17C):
    """Values, presence mask as test_workgroup_batch_inversion_matches_per_value_inverse."""
    rng = random.Random(seed + n)
    vals = [rng.randrange(1, P) for _ in range(n)]
    present = [1] * n
    for k in (0, 63, 64, 200, n - 1):
        if k < n and n > 1:
            present[k] = 0
    vals[min(5, n - 1)] = 0
    present[min(5, n - 1)] = 0  # a zero element, marked absent as the kernels do
    vals[min(7, n - 1)] = 1
    if n == 1:
        vals, present = [rng.randrange(2, P)], [1]
    return vals, present


@functools.lru_cache(None)
def g2_points(n=3):
    """Affine G2 points (canonical coordinates) for the line kernels."""
    rng = random.Random(0x62)
    return [bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R)) for _ in range(n)]


def g2_raw(q):
    """x.c0 x.c1 y.c0 y.c1 as Montgomery limbs, flat."""
    return [w for c in (q[0][0], q[0][1], q[1][0], q[1][1]) for w in mont(c)]
