"""Directed encodings for the decode kernels (k_decode.hip: k_decode_sigs,
k_subgroup_sigs, k_decode_pubkeys), shared by the CPU run through
tests/hostcheck (test_decode_edges_host.py, TBG_BOUNDS_CHECK on) and the GPU
run through tests/devcheck (dc_decode_*, test_gpu_devcheck_decode.py) and the
engine (test_gpu_decode_edges.py).  Deterministic; built at import with Python
integers and oracle/bls12_381.py only.  No golden file is read for an
expectation and none is written.

Every expected status and point is the oracle's: g2_decompress(...,
subgroup_check=False) for k_decode_sigs, the full check for k_subgroup_sigs,
g1_decompress for keys.  Every entry also names the branch it was built for;
sqrt_model / g2_path restate the norm-method root of bls_tower.h
(gamma = norm^((p+1)/4), delta = (a0 + gamma) / 2) and the decoder's order of
checks in Python integers, and _prove() asserts at import that each entry
still takes its branch -- a list that stopped reaching a branch fails on the
CPU.

The branches the lists are for (none of them reached by an honest or random
input), and the kinds that reach them:
  * fp2_sqrt_in's real right-hand side, root (s, 0) and root (0, s); through
    it fp2_lex_largest's c1 == 0 arm and the negation of a root with a zero
    component: real_s0, real_0s (both sign flags);
  * coordinate >= p per component, at p - 1, p, p + 1, the largest value the
    bytes hold and two values that differ from p in opposite directions in
    their top and lower bytes: field_c0_*, field_c1_* (G2), field_* (G1);
  * bad infinity encodings (sign bit, x in one component only, x >= p under
    the infinity bit: a flags error, never a field error): flags_*;
  * both arms of the generic root's final select and its first refusal:
    delta_residue, delta_nonresidue, norm_nonresidue;
  * infinity in the middle of k_subgroup_sigs' [|x|] a: sub_tor, the bare
    point of order 13 ([12] a == -a at the second addition).  NOT reached: the
    single-lane fallback (`exc`).  It needs [k] a == a at one of the five
    additions, an order dividing 11, 103, 53759 or 230901736800255; all are
    coprime to #E2(Fp2), so no point of the curve -- and the decoder stores
    only points of the curve -- gets there (subgroup_events asserts it for
    every entry; the hash-to-G2 lists found the same for px_mul_x_complete);
  * g1_in_subgroup's two jac_mul_xabs ladders on points of order 3 and 11:
    the P == Q case of jac_add and infinity in mid-ladder: low3_*, low11
    (g1_ladder_events).
"""
import collections
import functools
import random

from oracle import bls12_381 as bls
from tests import edge_operands as eo
from tests.edge_points import XLaw, bank, neg

P = bls.P
NL = eo.NL
INV2 = pow(2, -1, P)
FP2_W, AFF_W, G1A_W = 2 * NL, 4 * NL, 2 * NL

# DecodeStatus (bls_curve.h) and the partial statuses the kernels store (tbls_gpu.h)
DEC_OK, DEC_IDENTITY, DEC_ERR_FLAGS, DEC_ERR_FIELD, DEC_ERR_NOT_ON_CURVE, DEC_ERR_SUBGROUP = 0, 1, -1, -2, -3, -4
PS_NOT_VERIFIED, PS_ERR_IDENTITY = 2, -5
DEC_NAMES = {0: "valid", 1: "identity", -1: "err_flags", -2: "err_field", -3: "err_curve", -4: "err_subgroup"}
_ERRORS = {"compressed flag must be set": DEC_ERR_FLAGS, "invalid infinity encoding": DEC_ERR_FLAGS,
           "x not in field": DEC_ERR_FIELD, "point is not on the curve": DEC_ERR_NOT_ON_CURVE,
           "point is not in the correct subgroup": DEC_ERR_SUBGROUP}

Entry = collections.namedtuple("Entry", "kind branch data")


def ps_of(dec):
    """k_decode_sigs' mapping of a DecodeStatus to the stored partial status."""
    return PS_NOT_VERIFIED if dec == DEC_OK else PS_ERR_IDENTITY if dec == DEC_IDENTITY else dec


# ---------------------------------------------------------------------------
# the oracle's side
@functools.lru_cache(None)
def g2_class(data, subgroup_check):
    """(DecodeStatus, point or None) of 96 bytes, from the oracle."""
    try:
        a = bls.g2_decompress(data, subgroup_check=subgroup_check)
    except bls.DecodeError as e:
        return _ERRORS[str(e)], None
    return (DEC_IDENTITY, None) if a is None else (DEC_OK, a)


@functools.lru_cache(None)
def g1_class(data):
    try:
        a = bls.g1_decompress(data)
    except bls.DecodeError as e:
        return _ERRORS[str(e)], None
    return (DEC_IDENTITY, None) if a is None else (DEC_OK, a)


def g1_mul_raw(a, k):
    """[k] a on E1 without reducing k mod r (points outside G1)."""
    return bls.pt_to_affine(bls.pt_mul(bls.pt_from_affine(a, bls._Fp), k, bls._Fp), bls._Fp)


def g1_x_key(a):
    """[x] key for the (negative) curve parameter x: the table's second entry."""
    return bls.g1_mul(a, bls.R - bls.X_ABS)


# ---------------------------------------------------------------------------
# the restatement: which branch an encoding takes
def sqrt_model(a):
    """(branch, root or None) of fp2_sqrt_in on a = (a0, a1), canonical."""
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (P + 1) // 4, P)
        if s * s % P == a0:
            return "real_s0", (s, 0)
        if s * s % P == (P - a0) % P:
            return "real_0s", (0, s)
        return "real_none", None  # (p = 3 mod 4: not reachable)
    norm = (a0 * a0 + a1 * a1) % P
    gamma = pow(norm, (P + 1) // 4, P)
    if gamma * gamma % P != norm:
        return "norm_nonresidue", None
    delta = (a0 + gamma) * INV2 % P
    t = pow(delta, (P - 3) // 4, P)
    x0 = delta * t % P
    if x0 * x0 % P == delta:
        branch, r = "delta_residue", (x0, a1 * t % P * INV2 % P)
    else:
        branch, r = "delta_nonresidue", (a1 * t % P * INV2 % P, (P - x0) % P)
    if bls.f2_sqr(r) != a:
        return branch + "_refused", None
    return branch, r


def _split96(data):
    x1 = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:48], "big")
    return int.from_bytes(data[48:], "big"), x1


def g2_path(data):
    """The path of g2_decompress_t<true, false> on 96 bytes, as a string:
    the exit it takes, or root branch / sign rule's arm / negated or kept."""
    c, inf, s = (data[0] >> 7) & 1, (data[0] >> 6) & 1, (data[0] >> 5) & 1
    if not c:
        return "flags_c"
    x0, x1 = _split96(data)
    if inf:
        return "identity" if (s == 0 and x0 == 0 and x1 == 0) else "flags_inf"
    if x0 >= P or x1 >= P:
        return "field" + ("_c0" if x0 >= P else "") + ("_c1" if x1 >= P else "")
    x = (x0, x1)
    rhs = bls.f2_add(bls.f2_mul(bls.f2_sqr(x), x), bls.B2)
    branch, r = sqrt_model(rhs)
    if r is None:
        return "curve/" + branch
    arm = "lex_c1" if r[1] != 0 else "lex_c0"
    largest = bls.fp_lex_largest(r[1]) if r[1] != 0 else bls.fp_lex_largest(r[0])
    assert largest == bls.f2_lex_largest(r)
    return "%s/%s/%s" % (branch, arm, "neg" if largest != bool(s) else "keep")


def g1_ladder_events(a):
    """What the additions of g1_in_subgroup's two jac_mul_xabs ladders meet on
    the affine point a, over the exact law: "dbl" (the running multiple equals
    P: jac_add's P == Q case), "cancel" (it equals -P: the sum is infinity),
    "inf" (it is infinity already), and "inf_dbl" (infinity is doubled)."""
    events = set()

    def ladder(p):
        acc = p
        for i in range(62, -1, -1):
            if acc is None:
                events.add("inf_dbl")
            acc = bls.g1_add(acc, acc)
            if (bls.X_ABS >> i) & 1:
                if acc is None:
                    events.add("inf")
                elif p is not None and acc == p:
                    events.add("dbl")
                elif p is not None and acc == bls.g1_neg(p):
                    events.add("cancel")
                acc = bls.g1_add(acc, p)
        return acc

    ladder(ladder(a))
    return events


# ---------------------------------------------------------------------------
# bytes
def enc96(x0, x1, flags):
    """c1 then c0, big-endian; the three flag bits OR-ed into the top byte."""
    assert 0 <= x0 < (1 << 384) and 0 <= x1 < (1 << 381)
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def enc48(x, flags):
    assert 0 <= x < (1 << 381)
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


# field-bound values: (name, value, side of p).  The last two differ from p
# in opposite directions in the top byte and in the lower 47 bytes, so a
# comparison that ran from the wrong end (or let the lower bytes decide)
# would put them on the wrong side.
TOP = 1 << 376  # the unit of the top byte
BOUND_VALUES = [("pm1", P - 1, "below"), ("p", P, "at"), ("pp1", P + 1, "above"),
                ("top_lo_bytes_hi", P - TOP + 1, "below"),      # top byte below p's, lower bytes above
                ("top_hi_bytes_lo", P + TOP - (1 << 368), "above"),  # top byte above p's, lower bytes below
                ("second_byte_hi", P + TOP - (1 << 375), "above")]   # = p + 2^375: top byte equal, the next above
for _n, _v, _side in BOUND_VALUES[3:5]:
    assert ((_v >> 376) < (P >> 376)) == (_side == "below") and ((_v % TOP) > (P % TOP)) == (_side == "below")
    assert (_v >> 376) != (P >> 376) and (_v < P) == (_side == "below")
assert all((v < P) == (side == "below") and (v == P) == (side == "at") for _, v, side in BOUND_VALUES)
MAX_C1, MAX_C0, MAX_G1 = (1 << 381) - 1, (1 << 384) - 1, (1 << 381) - 1


# ---------------------------------------------------------------------------
# G2
def _both_flags(kind, x):
    """The encodings of x under both sign flags."""
    return [Entry(kind, None, enc96(x[0], x[1], 0x80 | s)) for s in (0, 0x20)]


@functools.lru_cache(None)
def real_rhs_points():
    """x = (a, b) with x^3 + 4 (1 + u) in Fp: a^2 = (b^3 - 4) / (3 b).
    -> {"real_s0": [x, x, x], "real_0s": [x, x, x]} from seeded draws (half
    of the draws have a residue a^2, and those split evenly)."""
    rng = random.Random(0xDEC0DE)
    out = {"real_s0": [], "real_0s": []}
    while min(len(v) for v in out.values()) < 3:
        b = rng.randrange(1, P)
        a2 = (b * b * b - 4) * pow(3 * b, -1, P) % P
        a = pow(a2, (P + 1) // 4, P)
        if a * a % P != a2:
            continue
        x = (a, b)
        rhs = bls.f2_add(bls.f2_mul(bls.f2_sqr(x), x), bls.B2)
        assert rhs[1] == 0
        out[sqrt_model(rhs)[0]].append(x)
    return {k: v[:3] for k, v in out.items()}


@functools.lru_cache(None)
def generic_points():
    """Random x by the branch of the generic root: 4 of each."""
    rng = random.Random(0x6E0E21C)
    want = {"delta_residue": 4, "delta_nonresidue": 4, "norm_nonresidue": 4}
    out = {k: [] for k in want}
    while any(want.values()):
        x = (rng.randrange(P), rng.randrange(P))
        branch = sqrt_model(bls.f2_add(bls.f2_mul(bls.f2_sqr(x), x), bls.B2))[0]
        if want.get(branch):
            want[branch] -= 1
            out[branch].append(x)
    return out


def _interleave(groups):
    """Round-robin over the groups: neighbouring lanes take different branches."""
    groups = [list(g) for g in groups if g]
    out = []
    while any(groups):
        for g in groups:
            if g:
                out.append(g.pop(0))
    return out


@functools.lru_cache(None)
def g2_entries():
    """[Entry]: the whole G2 list, interleaved by group."""
    b = bank()
    real, gen = real_rhs_points(), generic_points()
    g_real = [e for k in ("real_s0", "real_0s") for x in real[k] for e in _both_flags(k, x)]
    g_gen = [e for k in ("delta_residue", "delta_nonresidue") for x in gen[k] for e in _both_flags(k, x)]
    g_gen += [Entry("norm_nonresidue", None, enc96(x[0], x[1], 0x80 | (0x20 * (i & 1))))
              for i, x in enumerate(gen["norm_nonresidue"])]
    g_sparse = [e for name, x in (("sparse_pm1_pm1", (P - 1, P - 1)), ("sparse_0_1", (0, 1)), ("sparse_2_0", (2, 0)))
                for e in _both_flags(name, x)]
    g_sparse += [Entry(name, None, enc96(x[0], x[1], 0x80 | s))
                 for name, x, s in (("off_0_0", (0, 0), 0), ("off_1_0", (1, 0), 0x20), ("off_0_2", (0, 2), 0))]
    g_field = []
    for i, (name, v, side) in enumerate(BOUND_VALUES + [("max", None, "above")]):
        s = 0x20 * (i & 1)
        g_field.append(Entry(f"field_c1_{name}_{side}", None, enc96(2, MAX_C1 if v is None else v, 0x80 | s)))
        g_field.append(Entry(f"field_c0_{name}_{side}", None, enc96(MAX_C0 if v is None else v, 3, 0x80 | s ^ 0x20)))
    valid = [bls.g2_compress(p) for p in b["g"][:4]] + [bls.g2_compress(neg(p)) for p in b["g"][:4]]
    g_valid = [Entry("valid", None, v) for v in valid]
    last = lambda c, n: bytes([c]) + bytes(n - 2) + b"\x01"  # noqa: E731
    g_flags = [Entry("flags_c_cleared", None, bytes([valid[0][0] & 0x7F]) + valid[0][1:]),
               Entry("identity", None, bytes([0xC0]) + bytes(95)),
               Entry("flags_inf_sign", None, bytes([0xE0]) + bytes(95)),
               Entry("flags_inf_c0_last", None, bytes([0xC0]) + bytes(94) + b"\x01"),
               Entry("flags_inf_c1_last", None, last(0xC0, 48) + bytes(48)),
               Entry("flags_inf_c0_p", None, enc96(P, 0, 0xC0)),
               Entry("flags_all_zero", None, bytes(96)),
               Entry("flags_c_cleared", None, bytes([valid[5][0] & 0x7F]) + valid[5][1:]),
               Entry("flags_inf_c1_p", None, enc96(0, P, 0xC0)),
               Entry("identity", None, bytes([0xC0]) + bytes(95))]
    g_sub = [e for name in ("t13", "t23", "tor", "ns") for e in
             (Entry("sub_" + name, None, bls.g2_compress(b[name])), Entry("sub_" + name, None, bls.g2_compress(neg(b[name]))))]
    out = _interleave([g_valid, g_real, g_flags, g_gen, g_field, g_sub, g_sparse])
    if len(out) % 64 == 0:
        out.append(g_valid[0])
    return [e._replace(branch=g2_path(e.data)) for e in out]


def g2_reached():
    """branch -> the kinds that reach it (the summary's table)."""
    t = {}
    for e in g2_entries():
        t.setdefault(e.branch, set()).add(e.kind)
    return {k: sorted(v) for k, v in sorted(t.items())}


def subgroup_events(a):
    """What the five mixed additions of k_subgroup_sigs' [|x|] a meet on the
    decoded point a, over the exact law: "exc" (the running multiple equals a:
    the doubling case, which sends the lane pair to the single-lane path),
    "cancel" (it equals -a) and "inf" (it is infinity: jac_add_aff_x returns
    a itself)."""
    events = set()
    acc = a
    for i in range(62, -1, -1):
        acc = bls.g2_add(acc, acc)
        if (bls.X_ABS >> i) & 1:
            if acc is None:
                events.add("inf")
            elif acc == a:
                events.add("exc")
            elif acc == neg(a):
                events.add("cancel")
            acc = bls.g2_add(acc, a)
    x = XLaw()
    assert x.mul_xabs(a) == acc or x.exc
    assert x.exc == ("exc" in events)
    return events


# k_subgroup_sigs entered alone: stored points in the limb forms of
# tests/edge_points.py (canonical, plus p, a negated y before its reduction)
SUBGROUP_FORMS = ["canon", "plus_p", ("canon", "canon", "neg16", "neg16"), ("plus_p", "canon", "plus_p", "canon")]


@functools.lru_cache(None)
def subgroup_points():
    """[(name, point)]: G2 points, the torsion and non-subgroup points of
    edge_points.bank() and the real-rhs points, G2 and other points in turn."""
    b = bank()
    out = [("g0", b["g"][0]), ("tor", b["tor"]), ("g1", b["g"][1]), ("ns", b["ns"]), ("g2", b["g"][2]),
           ("t13", b["t13"]), ("g3", b["g"][3]), ("t23", b["t23"])]
    real = [g2_class(e.data, False)[1] for e in g2_entries() if e.kind.startswith("real_")]
    for i, p in enumerate(real[::2]):
        out += [("g%d" % (4 + i % 4), b["g"][4 + i % 4]), ("real%d" % i, p)]
    return out


# ---------------------------------------------------------------------------
# G1
@functools.lru_cache(None)
def g1_low_order():
    """(0, 2), (0, -2) (order 3) and a point of order 11 on E1."""
    h1 = 3 * 11**2 * 10177**2 * 859267**2 * 52437899**2
    rng = random.Random(0x0E11)
    while True:
        x = rng.randrange(P)
        y2 = (x * x * x + bls.B1) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P != y2:
            continue
        q = g1_mul_raw((x, y), h1 * bls.R // 121)
        if q is None:
            continue
        if g1_mul_raw(q, 11) is not None:
            q = g1_mul_raw(q, 11)
        assert q is not None and g1_mul_raw(q, 11) is None
        return [(0, 2), (0, P - 2)], q


@functools.lru_cache(None)
def g1_entries():
    rng = random.Random(0x61E7)
    keys = [bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R)) for _ in range(6)]
    valid = [Entry("valid", None, bls.g1_compress(k)) for k in keys]
    valid += [Entry("valid_neg", None, bls.g1_compress(bls.g1_neg(k))) for k in keys[:3]]  # the same x, the other flag
    low3, low11 = g1_low_order()
    while True:  # a random curve point outside G1
        x = rng.randrange(P)
        y2 = (x * x * x + bls.B1) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2 and not bls.g1_in_subgroup((x, y)):
            ns = (x, y)
            break
    rare = [Entry("low3_plus", None, bls.g1_compress(low3[0])), Entry("low3_minus", None, bls.g1_compress(low3[1])),
            Entry("low11", None, bls.g1_compress(low11)), Entry("low11", None, bls.g1_compress(bls.g1_neg(low11))),
            Entry("non_subgroup", None, bls.g1_compress(ns)), Entry("off_pm1", None, enc48(P - 1, 0x80))]
    rare += [Entry(f"field_{name}_{side}", None, enc48(v, 0x80 | (0x20 * (i & 1))))
             for i, (name, v, side) in enumerate(BOUND_VALUES[1:] + [("max", MAX_G1, "above")])]
    v0 = valid[0].data
    rare += [Entry("flags_c_cleared", None, bytes([v0[0] & 0x7F]) + v0[1:]),
             Entry("identity", None, bytes([0xC0]) + bytes(47)),
             Entry("flags_inf_sign", None, bytes([0xE0]) + bytes(47)),
             Entry("flags_inf_x", None, bytes([0xC0]) + bytes(46) + b"\x01"),
             Entry("flags_inf_x_p", None, enc48(P, 0xC0)),
             Entry("flags_all_zero", None, bytes(48))]
    return [e._replace(branch=g1_path(e.data)) for e in _interleave([valid, rare])]


def g1_path(data):
    c, inf, s = (data[0] >> 7) & 1, (data[0] >> 6) & 1, (data[0] >> 5) & 1
    if not c:
        return "flags_c"
    x = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:], "big")
    if inf:
        return "identity" if (s == 0 and x == 0) else "flags_inf"
    if x >= P:
        return "field"
    y2 = (x * x * x + bls.B1) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return "curve"
    if bls.fp_lex_largest(y) != bool(s):
        y = P - y
    ev = g1_ladder_events((x, y))
    return "ladder" + "".join("/" + e for e in sorted(ev))


def g1_layout(blk):
    """The G1 list laid out for a launch of n = blk + 3 keys: failures at
    lanes 0, blk - 1, blk and n - 1, the other entries spread over lanes
    2, 4, ... with valid keys everywhere else.  -> [Entry] of length n."""
    entries = g1_entries()
    valid = [e for e in entries if e.kind.startswith("valid")]
    rare = [e for e in entries if not e.kind.startswith("valid")]
    n = blk + 3
    corners = [0, blk - 1, blk, n - 1]
    assert n >= 2 * len(rare) + 8
    out = [valid[i % len(valid)] for i in range(n)]
    spots = corners + [k for k in range(2, n, 2) if k not in corners and k + 1 not in corners and k - 1 not in corners]
    for k, e in zip(spots, rare):
        out[k] = e
    assert all(g1_class(out[k].data)[0] != DEC_OK for k in corners)
    assert all(g1_class(out[k].data)[0] == DEC_OK for k in (1, blk - 2, blk + 1))
    return out


# ---------------------------------------------------------------------------
# raw limbs
def coord_of(words):
    """The value mod p (Montgomery factor removed) of a stored coordinate, or
    a string: every limb below 2^28 and the value below 2p, the range
    bls_field.h gives for the output of fp_mul / fp_reduce."""
    w = [int(v) for v in words]
    if len(w) != NL:
        return "wrong length"
    if any(not 0 <= v <= eo.M28 for v in w):
        return "limbs not below 2^28"
    if eo.val(w) >= 2 * P:
        return "value not below 2p"
    return eo.unmont(w)


def check_g2_slot(words, status, want_status, want_point):
    """None, or what is wrong with one partial's sig_aff / partial_status."""
    if status != want_status:
        return f"status {status}, expected {want_status}"
    if want_status != PS_NOT_VERIFIED:
        return None if list(words) == [0] * AFF_W else "sig_aff of a failed partial is not all zero"
    c = [coord_of(words[i * NL:(i + 1) * NL]) for i in range(4)]
    for v in c:
        if isinstance(v, str):
            return v
    return None if ((c[0], c[1]), (c[2], c[3])) == want_point else "point differs"


def check_g1_slot(out, out_x, status, want_status, want_point):
    """None, or what is wrong with one key's out / out_x / status."""
    if status != want_status:
        return f"status {status}, expected {want_status}"
    if want_status != DEC_OK:
        return None if list(out) == [0] * G1A_W and list(out_x) == [0] * G1A_W else "a failed key's entries are not zero"
    for words, want in ((out, want_point), (out_x, g1_x_key(want_point))):
        c = [coord_of(words[i * NL:(i + 1) * NL]) for i in range(2)]
        for v in c:
            if isinstance(v, str):
                return v
        if (c[0], c[1]) != want:
            return "key differs" if words is out else "[x] key differs"
    return None


# ---------------------------------------------------------------------------
# the lists' own claims, asserted at import
def _prove():
    ents = g2_entries()
    assert len(ents) > 64 and len(ents) % 64 != 0
    by = {}
    for e in ents:
        by.setdefault(e.kind, []).append(e)
        # the restatement agrees with the oracle on every entry's class
        dec, pt = g2_class(e.data, False)
        exits = {"flags_c": DEC_ERR_FLAGS, "flags_inf": DEC_ERR_FLAGS, "identity": DEC_IDENTITY}
        if e.branch in exits:
            assert dec == exits[e.branch], e
        elif e.branch.startswith("field"):
            assert dec == DEC_ERR_FIELD, e
        elif e.branch.startswith("curve/"):
            assert dec == DEC_ERR_NOT_ON_CURVE, e
        else:
            assert dec == DEC_OK and bls.g2_on_curve(pt), e
    real = real_rhs_points()
    assert len(real["real_s0"]) >= 2 and len(real["real_0s"]) >= 2
    for kind, arm in (("real_s0", "lex_c0"), ("real_0s", "lex_c1")):
        paths = [e.branch for e in by[kind]]
        assert set(paths) == {f"{kind}/{arm}/neg", f"{kind}/{arm}/keep"}, paths
        for e in by[kind]:  # on the curve, outside G2, a zero component in y
            pt = g2_class(e.data, False)[1]
            assert g2_class(e.data, True)[0] == DEC_ERR_SUBGROUP and 0 in pt[1]
    for kind in ("delta_residue", "delta_nonresidue"):
        assert len(by[kind]) >= 8
        assert {e.branch for e in by[kind]} == {f"{kind}/lex_c1/neg", f"{kind}/lex_c1/keep"}
    assert len(by["norm_nonresidue"]) >= 4 and all(e.branch == "curve/norm_nonresidue" for e in by["norm_nonresidue"])
    for kind in ("sparse_pm1_pm1", "sparse_0_1", "sparse_2_0"):
        assert [g2_class(e.data, False)[0] for e in by[kind]] == [DEC_OK, DEC_OK], kind
    for kind in ("off_0_0", "off_1_0", "off_0_2"):
        assert all(e.branch.startswith("curve/") for e in by[kind]), kind
    for kind, es in by.items():
        if kind.startswith("field_"):
            comp = kind[6:8]
            below = kind.endswith("_below")
            for e in es:
                assert e.branch == "field_" + comp if not below else not e.branch.startswith("field"), e
        if kind.startswith("flags_inf"):
            assert all(e.branch == "flags_inf" for e in es), kind
        if kind in ("flags_c_cleared", "flags_all_zero"):
            assert all(e.branch == "flags_c" for e in es), kind
    assert len([k for k in by if k.startswith("field_c0")]) == 7 and len([k for k in by if k.startswith("field_c1")]) == 7
    assert all(e.branch == "identity" for e in by["identity"]) and len(by["flags_c_cleared"]) >= 2
    for e in by["valid"]:
        assert g2_class(e.data, True)[0] == DEC_OK
    for name in ("t13", "t23", "tor", "ns"):
        for e in by["sub_" + name]:
            assert g2_class(e.data, False)[0] == DEC_OK and g2_class(e.data, True)[0] == DEC_ERR_SUBGROUP
            # the bare order-13 point: [12] a == -a at the second addition, infinity from there to the fourth.  `exc` itself needs
            # [k] a == a for k in 2, 12, 104, 53760, ...: an order dividing 11, 103, 53759, ..., all
            # coprime to #E2(Fp2) (tests/test_h2c_edges_host.py proves it), so no decoded point sets it
            assert subgroup_events(g2_class(e.data, False)[1]) == ({"cancel", "inf"} if name == "tor" else set()), name
    assert not any("exc" in subgroup_events(g2_class(e.data, False)[1]) for e in ents if g2_class(e.data, False)[1])
    # neighbouring lanes take different branches
    assert sum(a.branch != b.branch for a, b in zip(ents, ents[1:])) >= len(ents) * 3 // 4

    g1 = g1_entries()
    k1 = {}
    for e in g1:
        k1.setdefault(e.kind, []).append(e)
        dec = g1_class(e.data)[0]
        if e.branch.startswith("ladder"):
            assert dec in (DEC_OK, DEC_ERR_SUBGROUP), e
        else:
            assert dec == {"flags_c": DEC_ERR_FLAGS, "flags_inf": DEC_ERR_FLAGS, "identity": DEC_IDENTITY,
                           "field": DEC_ERR_FIELD, "curve": DEC_ERR_NOT_ON_CURVE}[e.branch], e
    xs = {}
    for e in k1["valid"] + k1["valid_neg"]:
        assert g1_class(e.data)[0] == DEC_OK and e.branch == "ladder"
        xs.setdefault(e.data[1:], set()).add(e.data[0] & 0x20)
    assert sum(v == {0, 0x20} for v in xs.values()) >= 3  # the same x under both sign flags
    low = k1["low3_plus"] + k1["low3_minus"] + k1["low11"]
    assert all(g1_class(e.data)[0] == DEC_ERR_SUBGROUP for e in low + k1["non_subgroup"])
    assert k1["non_subgroup"][0].branch == "ladder"
    reached = set()
    for e in low:
        reached |= set(e.branch.split("/")[1:])
    assert {"dbl", "inf"} <= reached, reached  # jac_add's P == Q case, and infinity in mid-ladder
    # (p - 2^376 + 1 lies below p: whatever the oracle says of it, it is no field error)
    assert all((e.branch == "field") != k.endswith("_below") for k, es in k1.items() if k.startswith("field_") for e in es)
    assert len([k for k in k1 if k.startswith("field_")]) == 6
    assert k1["off_pm1"][0].branch == "curve"
    assert [e.branch for e in k1["flags_inf_x_p"] + k1["flags_inf_x"] + k1["flags_inf_sign"]] == ["flags_inf"] * 3
    assert k1["flags_c_cleared"][0].branch == "flags_c" and k1["flags_all_zero"][0].branch == "flags_c"


_prove()
