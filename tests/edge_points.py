"""Directed operand lists for the lane-pair G2 group law (bls_pair.h,
bls_sgb.h), shared by the CPU run through tests/hostcheck (hc_g2_op_raw,
TBG_BOUNDS_CHECK on: a violated precondition aborts) and the GPU run through
tests/devcheck (dc_g2, test_gpu_devcheck_g2.py).  Deterministic.

A point is None (infinity) or an affine pair of Fp2 pairs of Python integers,
as in oracle/bls12_381.py; what crosses to the code under test is raw limbs
(tests/edge_operands.py): Montgomery coordinates, an Fp2 as c0, c1.  Expected
values are computed here on affine points with Python integers: the exact
group law of the oracle for the complete operations, and for the operations
without a doubling branch (`exc` set, infinity returned) a restatement of
their schedule over that exact law, so the `exc` flag is compared exactly.
The result of the code under test is normalised X / Z^2, Y / Z^3 (infinity:
Z == 0 mod p) before it is compared.
"""
import functools
import json
import os
import random

from oracle import bls12_381 as bls
from tests import edge_operands as eo

P = bls.P
NL = eo.NL
HERE = os.path.dirname(os.path.abspath(__file__))
OPS = ["add_x", "add_aff_x", "dbl_lo", "add_in", "add_aff_in", "psi", "mul_xabs_x", "mul_xabs_aff_x",
       "in_subgroup_aff", "clear_cofactor", "sgb_sums", "sgb_sums_complete", "sgb_fold", "sgb_fold_complete"]
SUM_V, FOLD_S = 6, 4
PSI_X = bls.f2_inv(bls.f2_pow((1, 1), (P - 1) // 3))
PSI_Y = bls.f2_inv(bls.f2_pow((1, 1), (P - 1) // 2))


# ---------------------------------------------------------------------------
# the exact group law, and the schedules of the operations under test
def add(a, b):
    return bls.g2_add(a, b)


def neg(a):
    return bls.g2_neg(a)


def mul(a, k):
    return None if a is None else bls.g2_mul_raw(a, k)


def psi(a):
    return None if a is None else (bls.f2_mul(bls.f2_conj(a[0]), PSI_X), bls.f2_mul(bls.f2_conj(a[1]), PSI_Y))


class XLaw:
    """jac_add_x / jac_add_aff_x on exact points: P == Q sets `exc` and
    yields infinity (what the code returns; the caller discards it)."""

    def __init__(self):
        self.exc = False

    def add(self, a, b):
        if a is None:
            return b
        if b is None:
            return a
        if a == b:
            self.exc = True
            return None
        return add(a, b)

    def mul_xabs(self, p):  # jac_mul_xabs_x / jac_mul_xabs_aff_x: 63 doublings, 5 additions
        acc = p
        for i in range(62, -1, -1):
            acc = add(acc, acc)
            if (bls.X_ABS >> i) & 1:
                acc = self.add(acc, p)
        return acc

    def clear_cofactor(self, p):  # g2_clear_cofactor_g
        a = neg(self.mul_xabs(p))
        pp = psi(p)
        b = self.add(a, pp)
        u = psi(psi(add(p, p)))
        u = self.add(u, neg(pp))
        u = self.add(u, neg(a))
        u = self.add(u, neg(p))
        c = neg(self.mul_xabs(b))
        return self.add(u, c)

    def running_sums(self, buckets):  # sgb_running_sums_g<F, true>
        run = q = None
        for v in range(len(buckets), 0, -1):
            run = self.add(run, buckets[v - 1])
            q = self.add(q, run)
        return q

    def fold(self, slices):  # sgb_fold_g<F, true>
        acc = slices[0]
        for s in slices[1:]:
            acc = self.add(acc, s)
        return acc


def weighted_sum(buckets):
    q = None
    for v, b in enumerate(buckets, 1):
        q = add(q, mul(b, v))
    return q


def plain_sum(points):
    q = None
    for p in points:
        q = add(q, p)
    return q


# ---------------------------------------------------------------------------
# points
@functools.lru_cache(None)
def bank():
    """g: points of G2; t13 / t23: G2 points with a 13- / 23-torsion component
    added; tor: a bare point of order 13; ns: a point of E2 outside G2 with no
    special structure (tests/golden: sgb_points.json, invalid_g2.json)."""
    rng = random.Random(0x6E2)
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        sp = json.load(f)["points"]
    with open(os.path.join(HERE, "golden", "invalid_g2.json")) as f:
        ip = json.load(f)["pools"]

    def dec(h):
        return bls.g2_decompress(bytes.fromhex(h), subgroup_check=False)

    b = {"g": [bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R)) for _ in range(8)],
         "t13": dec(sp["t13"][0]), "t23": dec(sp["t23"][0]), "tor": dec(sp["torsion13"][0]),
         "ns": dec(ip["non_subgroup"][0])}
    assert mul(b["tor"], 13) is None and not bls.g2_in_subgroup(b["ns"]) and bls.g2_on_curve(b["ns"])
    return b


def _rand_f2(rng):
    while True:
        l = (rng.randrange(P), rng.randrange(P))
        if l != (0, 0):
            return l


def jac(a, lam=(1, 0)):
    """(lam^2 x, lam^3 y, lam); infinity as (1, 1, 0) scaled the same way."""
    x, y = ((1, 0), (1, 0)) if a is None else a
    l2 = bls.f2_sqr(lam)
    return (bls.f2_mul(x, l2), bls.f2_mul(y, bls.f2_mul(l2, lam)), (0, 0) if a is None else lam)


def _fp_words(v, form):
    """A coordinate's component as raw limbs: canonical Montgomery form, the
    same plus p (the top of [0, 2p), the range f_reduce leaves), or
    16p - (-v): a negated value before its reduction (what the square root's
    non-residue arm leaves in y.c1; the decoder reduces it before it stores)."""
    m = v * eo.R % P
    if form == "plus_p":
        return eo.limbs(m + P)
    if form == "neg16":
        return eo.limbs(16 * P - (P - m) % P) if m else eo.limbs(0)
    return eo.limbs(m)


def jac_words(J, form="canon"):
    """6 x 14 words; form: one name for every component or a tuple of six."""
    forms = (form,) * 6 if isinstance(form, str) else form
    comps = [J[0][0], J[0][1], J[1][0], J[1][1], J[2][0], J[2][1]]
    return [w for c, f in zip(comps, forms) for w in _fp_words(c, f)]


def aff_words(a, form="canon"):
    forms = (form,) * 4 if isinstance(form, str) else form
    comps = [a[0][0], a[0][1], a[1][0], a[1][1]]
    return [w for c, f in zip(comps, forms) for w in _fp_words(c, f)]


def point_of(words):
    """The affine point (or None) of 84 result words, or a string saying what
    is wrong with their form."""
    w = [int(v) for v in words]
    if len(w) != 6 * NL:
        return "wrong length"
    if any(not 0 <= v <= eo.M28 for v in w):
        return "limbs not below 2^28"
    c = [eo.unmont(w[i * NL:(i + 1) * NL]) for i in range(6)]
    X, Y, Z = (c[0], c[1]), (c[2], c[3]), (c[4], c[5])
    if Z == (0, 0):
        return None
    zi = bls.f2_inv(Z)
    zi2 = bls.f2_sqr(zi)
    return (bls.f2_mul(X, zi2), bls.f2_mul(Y, bls.f2_mul(zi2, zi)))


def check(op, words, flag, expect):
    """None, or what is wrong.  expect = (point, exc, verdict); point "any":
    not compared (an `exc` result of a single addition is still compared: the
    code returns infinity)."""
    want, exc, verdict = expect
    if (flag & 1) != int(exc):
        return f"exc {flag & 1}, expected {int(exc)}"
    if op == "in_subgroup_aff":
        return None if (flag >> 1) == int(verdict) else f"verdict {flag >> 1}, expected {int(verdict)}"
    if flag >> 1:
        return "verdict bit set"
    got = point_of(words)
    if isinstance(got, str):
        return got
    if got != want:
        return "point differs" if got is not None and want is not None else f"infinity: got {got is None}, expected {want is None}"
    return None


# ---------------------------------------------------------------------------
# cases: (a words, b words or None, expect, kind)
def _two_forms(rng, a):
    """The same point in two different Jacobian forms."""
    return jac(a, _rand_f2(rng)), jac(a, _rand_f2(rng))


def _addition_cases(mixed):
    """Operand pairs for the additions; `mixed`: the second operand affine."""
    rng = random.Random(0xADD2 + mixed)
    g = bank()["g"]
    ns, t13 = bank()["ns"], bank()["t13"]
    out = []

    def put(kind, p, q, pform="canon", qform="canon", lam_p=None, lam_q=None):
        pj = jac(p, lam_p or _rand_f2(rng))
        if mixed:
            if q is None:
                return
            qw = aff_words(q, qform)
        else:
            qw = jac_words(jac(q, lam_q or _rand_f2(rng)), qform)
        out.append((jac_words(pj, pform), qw, (p, q), kind))

    one = (1, 0)
    for i in range(6):
        p, q = g[i], g[(i + 3) % 8]
        put("generic", p, q)
        put("double", p, p)                       # the same point, two Jacobian forms: H, R zero after reduction
        put("cancel", p, neg(p))
        put("inf_q", None, q)
        put("p_inf", p, None)
        put("inf_inf", None, None)
    put("generic", ns, t13)
    put("double", ns, ns, pform="plus_p")
    put("cancel", t13, neg(t13), pform="plus_p")
    # Z = 1 in Montgomery form, coordinates at the top of [0, 2p)
    put("generic", g[0], g[1], lam_p=one, lam_q=one, pform="plus_p", qform="plus_p" if not mixed else "canon")
    put("double", g[2], g[2], lam_p=one, lam_q=one, pform="plus_p")
    put("cancel", g[3], neg(g[3]), lam_p=one, lam_q=one, pform="plus_p")
    put("generic", g[4], g[5], pform=("plus_p", "canon", "canon", "plus_p", "plus_p", "canon"))
    if mixed:  # an affine operand as the decoder leaves it: a negated root before its reduction (products only)
        put("generic", g[6], g[7], qform=("canon", "canon", "neg16", "neg16"))
        put("double", g[6], g[6], qform=("canon", "canon", "neg16", "neg16"))
        put("cancel", g[6], neg(g[6]), qform=("canon", "canon", "neg16", "neg16"))
        put("inf_q", None, g[7], qform=("canon", "canon", "neg16", "neg16"))
    else:
        put("generic", g[6], g[7], pform="plus_p", qform="plus_p")
        put("inf_q", None, g[7], qform="plus_p")
        put("p_inf", g[7], None, pform="plus_p")
    return out


def _interleave(cases):
    """Neighbouring pairs of a wave take different branches: the kinds in
    rotation."""
    by = {}
    for c in cases:
        by.setdefault(c[3], []).append(c)
    out = []
    while any(by.values()):
        for k in list(by):
            if by[k]:
                out.append(by[k].pop(0))
    return out


def _expect_add(op, p, q):
    if op in ("add_in", "add_aff_in"):
        return (add(p, q), False, False)
    x = XLaw()
    r = x.add(p, q)
    return (r, x.exc, False)


def _sum_cases():
    """Six buckets: every pattern of empty buckets with distinct points, all
    equal, equal pairs, a cancelling pair; in assorted Jacobian forms."""
    rng = random.Random(0x5B6)
    g = bank()["g"]
    sets = [[g[v] if (pat >> v) & 1 else None for v in range(SUM_V)] for pat in range(1 << SUM_V)]
    sets.append([g[0]] * SUM_V)                                  # all buckets equal
    sets.append([g[1], None, g[1], None, g[1], None])
    sets.append([None, g[2], g[2], None, None, g[3]])
    sets.append([g[4], g[5], None, None, neg(g[5]), None])       # the running sum returns to infinity
    sets.append([neg(mul(g[6], 2)), g[6], None, None, None, None])  # Q is the identity
    out = []
    for s in sets:
        words = [w for b in s for w in jac_words(jac(b, _rand_f2(rng)), "plus_p" if rng.random() < 0.3 else "canon")]
        out.append((words, s))
    return out


def _fold_cases():
    rng = random.Random(0xF01D)
    g = bank()["g"]
    sets = [[g[0], g[1], g[2], g[3]], [g[0], g[0], g[1], g[2]], [g[0]] * 4, [None, g[1], None, g[1]],
            [g[2], neg(g[2]), g[3], g[3]], [None] * 4, [g[4], None, None, None], [None, None, None, g[5]],
            [g[5], g[6], add(g[5], g[6]), g[7]], [g[1], g[2], neg(add(g[1], g[2])), None]]
    out = []
    for s in sets:
        words = [w for b in s for w in jac_words(jac(b, _rand_f2(rng)), "plus_p" if rng.random() < 0.3 else "canon")]
        out.append((words, s))
    return out


@functools.lru_cache(None)
def cases():
    """op -> list of (a words, b words or None, expect).  The additions'
    lists are interleaved by kind (generic, double, cancel, infinities), hold
    more than one wave of pairs and end in a partly filled wave."""
    b = bank()
    g = b["g"]
    rng = random.Random(0xCA5E)
    out = {}
    for op in ("add_x", "add_in", "add_aff_x", "add_aff_in"):
        lst = _interleave(_addition_cases(op in ("add_aff_x", "add_aff_in")))
        out[op] = [(aw, bw, _expect_add(op, p, q)) for aw, bw, (p, q), _ in lst]
    pts = [g[0], None, b["ns"], g[1], b["t13"], None, b["tor"], g[2], b["t23"]]
    out["dbl_lo"] = []
    out["psi"] = []
    for i, p in enumerate(pts * 4):
        form = ("canon", "plus_p", ("plus_p", "canon", "canon", "plus_p", "canon", "plus_p"))[i % 3]
        lam = (1, 0) if i % 5 == 0 else _rand_f2(rng)
        w = jac_words(jac(p, lam), form)
        out["dbl_lo"].append((w, None, (add(p, p), False, False)))
        out["psi"].append((w, None, (psi(p), False, False)))
    # [|x|] P, the subgroup test, cofactor clearing: G2 points, the crafted
    # torsion points and a plain non-subgroup point side by side in one wave
    mpts = [g[0], b["tor"], b["ns"], g[1], b["t13"], b["t23"], g[2], None, g[3]]
    out["mul_xabs_x"], out["mul_xabs_aff_x"], out["in_subgroup_aff"], out["clear_cofactor"] = [], [], [], []
    for i, p in enumerate(mpts):
        x = XLaw()
        m = x.mul_xabs(p)
        lam = (1, 0) if i % 2 == 0 else _rand_f2(rng)
        out["mul_xabs_x"].append((jac_words(jac(p, lam), "plus_p" if i % 3 == 0 else "canon"), None,
                                  (m, x.exc, False)))
        x = XLaw()
        out["clear_cofactor"].append((jac_words(jac(p, lam), "plus_p" if i % 3 == 1 else "canon"), None,
                                      (x.clear_cofactor(p), x.exc, False)))
        if p is None:
            continue
        x = XLaw()
        m = x.mul_xabs(p)
        form = ("canon", ("canon", "canon", "neg16", "neg16"), ("plus_p", "canon", "plus_p", "canon"))[i % 3]
        out["mul_xabs_aff_x"].append((aff_words(p, form), None, (m, x.exc, False)))
        out["in_subgroup_aff"].append((aff_words(p, form), None,
                                       (None, x.exc, m is not None and psi(p) == neg(m))))
    out["sgb_sums"], out["sgb_sums_complete"] = [], []
    for words, s in _sum_cases():
        x = XLaw()
        q = x.running_sums(s)
        out["sgb_sums"].append((words, None, (q, x.exc, False)))
        out["sgb_sums_complete"].append((words, None, (weighted_sum(s), False, False)))
    out["sgb_fold"], out["sgb_fold_complete"] = [], []
    for words, s in _fold_cases():
        x = XLaw()
        q = x.fold(s)
        out["sgb_fold"].append((words, None, (q, x.exc, False)))
        out["sgb_fold_complete"].append((words, None, (plain_sum(s), False, False)))
    assert set(out) == set(OPS)
    return out
