"""The lane-cooperative field arithmetic on real gfx950 lanes (tests/devcheck:
thin kernels around the product headers' device functions) with the directed
operands of tests/edge_operands.py, against Python integers and the oracle.

The device bodies of the cross-lane exchanges (ds_swizzle, DPP, shuffles, LDS)
otherwise run only inside whole VerifyAndAggregate launches on hash and
pairing outputs; here every primitive sees limbs at 0 and 2^28 - 1, lazy limbs
at 2^31 - 1, signed limbs at +-2^29, quotient estimates on a multiple of p,
and partly filled rows / hexads / workgroups.  All assertions are exact.

Every row, hexad and pair of a launch holds a different tuple and is checked
on its own; output past the last slot is pre-filled with a sentinel and must
come back untouched.  After a non-zero HIP status no further GPU work is
started in this module."""
import ctypes

import pytest

from oracle import bls12_381 as bls
from tests import edge_operands as eo
from tests import devcheck
from tests.devcheck import FP_OPS, HEX_OPS, PAIR_OPS, R12_OPS, ROW_OPS

pytestmark = pytest.mark.gpu

P = eo.P
NL = 14
SENT = eo.SENTINEL
_STATE = {"rc": 0}


def call(fn, *args):
    """Run one devcheck entry; its return code is asserted first."""
    if _STATE["rc"]:
        pytest.fail(f"an earlier devcheck entry returned HIP status {_STATE['rc']}: no further GPU work here")
    rc = getattr(devcheck.lib(), fn)(*args)
    if rc:
        _STATE["rc"] = rc
    assert rc == 0, f"{fn} returned {rc}"


def u32(words):
    return (ctypes.c_uint32 * len(words))(*[int(w) & 0xFFFFFFFF for w in words])


def i32(words):
    return (ctypes.c_int32 * len(words))(*[int(w) for w in words])


def sentinel(n, signed=False):
    t = ctypes.c_int32 if signed else ctypes.c_uint32
    v = SENT - (1 << 32) if signed else SENT
    return (t * n)(*([v] * n))


def untouched(buf, start):
    """Every word from `start` on still holds the sentinel."""
    s = SENT if buf._type_ is ctypes.c_uint32 else SENT - (1 << 32)
    return all(x == s for x in buf[start:])


def flat(vectors):
    return [w for v in vectors for w in v]


def chunks(xs, n):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


# ---------------------------------------------------------------------------
# lane-private Fp
@pytest.mark.parametrize("op", FP_OPS)
def test_fp_lane_private(op):
    cases = eo.fp_cases()[op]
    groups = {}
    for t in cases:  # one launch per small constant (fp_mul_small), 512 tuples at most each
        k = next((x for x in t if isinstance(x, int)), 0)
        groups.setdefault(k, []).append(t)
    for k, group in groups.items():
        for part in chunks(group, 512):
            ops = list(zip(*[[x for x in t if isinstance(x, list)] for t in part]))
            args = [(i32 if op == "from_signed" else u32)(flat(col)) for col in ops] + [None] * (4 - len(ops))
            if op == "from_signed":
                args[0] = ctypes.cast(args[0], ctypes.POINTER(ctypes.c_uint32))
            n = len(part)
            out = sentinel(n * NL)
            call("dc_fp", FP_OPS.index(op), *args, k, out, n)
            for i, t in enumerate(part):
                err = eo.check_plain(out[i * NL:(i + 1) * NL], eo.fp_expect(op, t))
                assert err is None, (op, i, t, err)


# ---------------------------------------------------------------------------
# row Fp
def _row_launch(op, part, threads):
    cols = list(zip(*part))
    args = [i32(flat(col)) for col in cols] + [None] * (4 - len(cols))
    n = len(part)
    out = sentinel(n * 16, signed=True)
    call("dc_row", ROW_OPS.index(op), *args, out, n, threads)
    for i, t in enumerate(part):
        err = eo.check_row(out[i * 16:(i + 1) * 16], eo.row_expect(op, t))
        assert err is None, (op, threads, i, t, err)


@pytest.mark.parametrize("op", ROW_OPS)
def test_row_fp_four_rows_a_wave(op):
    """64-thread workgroups: the four rows of every wave hold different
    tuples; the last launch of a list ends in a partly filled wave."""
    cases = eo.row_cases()[op]
    for part in chunks(cases, eo.ROW_CHUNK):
        _row_launch(op, part, 64)
    _row_launch(op, cases[:5], 64)  # one full wave and one row of the next
    _row_launch(op, cases[-3:], 64)  # a lone wave with its last row empty


@pytest.mark.parametrize("op", ROW_OPS)
def test_row_fp_one_workgroup_of_36_rows(op):
    """One 576-thread workgroup (the final exponentiation's shape): rows in
    waves 1..8 run; then the same workgroup partly filled."""
    cases = eo.row_cases()[op]
    step = max(1, len(cases) // 101)
    pick = cases[::step][:101]
    for part in chunks(pick, eo.ROW_BLOCK_ROWS):  # 36, 36, 29 rows
        _row_launch(op, part, 16 * eo.ROW_BLOCK_ROWS)


# ---------------------------------------------------------------------------
# Fp12 helpers
def f12_words(f, bump=()):
    """168 words: the 12 Fp in quad / row order as Montgomery limbs; `bump`
    names coefficients stored as value + p (still below 2p)."""
    return flat(eo.limbs(v * eo.R % P + (P if i in bump else 0)) for i, v in enumerate(eo.f12_to_quad(f)))


def f12_from_plain(words):
    """168 plain words back to an oracle element, limbs checked below 2^28."""
    ls = chunks([int(w) for w in words], NL)
    assert all(0 <= w <= eo.M28 for l in ls for w in l), "limbs not below 2^28"
    return [eo.unmont(l) for l in ls]


def f12_from_rows(words):
    """12 x 16 signed row words: lanes 14, 15 zero, then residues."""
    rows = chunks([int(w) for w in words], 16)
    assert all(r[14] == 0 and r[15] == 0 for r in rows), "lanes 14, 15 not zero"
    return [eo.unmont(r) for r in rows]


def cyclotomic(n):
    import random
    rng = random.Random(0xC7C10)
    out = [bls.F12_ONE, eo.f12_values()["cyclo"]]
    while len(out) < n:
        out.append(eo.easy_part(tuple(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3))
                                      for _ in range(2))))
    return out[:n]


_FE = {}


def final_exp_of(name):
    """The oracle's final exponentiation, computed once per element."""
    if name not in _FE:
        _FE[name] = bls.final_exp(eo.f12_values()[name])
    return _FE[name]


def fe_names():
    return [n for n in eo.f12_values() if n != "zero"]


# ---------------------------------------------------------------------------
# row Fp12 (one 576-thread workgroup, slots in LDS)
def _row12(op, x, y=None):
    out = sentinel(12 * 16, signed=True)
    flag = sentinel(1)
    call("dc_row12", R12_OPS.index(op), u32(x), u32(y) if y is not None else None, out, flag)
    return f12_from_rows(out), flag[0]


def test_row_fp12_ops():
    V = eo.f12_values()
    names = list(V)
    for i, n in enumerate(names):
        a, b = V[n], V[names[(i + 5) % len(names)]]
        bump = (i % 12, (i + 7) % 12)
        got, _ = _row12("mul", f12_words(a, bump), f12_words(b))
        assert eo.check_f12(got, bls.f12_mul(a, b)) is None, ("mul", n)
        got, _ = _row12("frob", f12_words(a, bump))
        assert eo.check_f12(got, bls.f12_frob(a)) is None, ("frob", n)
        got, _ = _row12("conj", f12_words(a, bump))
        assert eo.check_f12(got, bls.f12_conj(a)) is None, ("conj", n)
        got, flag = _row12("isone", f12_words(a, bump))
        assert eo.check_flag(flag, bls.f12_is_one(a)) is None, ("isone", n)
        assert eo.check_f12(got, a) is None
    for k, a in enumerate(cyclotomic(4)):
        got, _ = _row12("cyc", f12_words(a))
        assert eo.check_f12(got, bls.f12_sqr(a)) is None, ("cyc", k)


def test_row_final_exp():
    """row_final_exp_inv given f and the oracle's f^-1 (as k_l0_inv supplies
    it): the oracle's value, and row_is_one exactly when it is 1."""
    V = eo.f12_values()
    for n in fe_names():
        want = final_exp_of(n)
        got, flag = _row12("fe", f12_words(V[n]), f12_words(bls.f12_inv(V[n])))
        assert eo.check_f12(got, want) is None, n
        assert eo.check_flag(flag, bls.f12_is_one(want)) is None, n
    assert bls.f12_is_one(final_exp_of("cancel")) and not bls.f12_is_one(final_exp_of("pairing"))


def _host_lines(q):
    from tests.hostcheck import lib as hc
    out = (ctypes.c_uint32 * (68 * 6 * NL))()
    hc().hc_g2_lines_raw(u32(eo.g2_raw(q)), out)
    return list(out)


def test_row_lines():
    """The 68 S lines on rows (one 192-thread workgroup, rl_line_out on
    threads 128..133) equal the host g2_lines Fp for Fp modulo p (the lines
    carry arbitrary scale factors: g2_lines is the pinned form)."""
    for q in eo.g2_points():
        out = sentinel(68 * 6 * NL)
        call("dc_row_lines", u32(eo.g2_raw(q)), out)
        err = eo.check_lines(list(out), _host_lines(q))
        assert err is None, err


# ---------------------------------------------------------------------------
# hexad
def _hex_elements(n, shift=0, nonzero=False):
    vals = [v for k, v in eo.f12_values().items() if not (nonzero and k == "zero")]
    return [vals[(i + shift) % len(vals)] for i in range(n)]


def _hex_launch(op, A, B=None, lines=None, pts=None, want_flags=False):
    n = len(A)
    cap = n + 3
    out = sentinel(cap * 168)
    flags = sentinel(cap * 6)
    call("dc_hex", HEX_OPS.index(op), u32(flat(A)), u32(flat(B)) if B else None,
         u32(flat(lines)) if lines else None, u32(flat(pts)) if pts else None, out, flags, n, cap)
    if op == "isone":
        assert untouched(out, 0)
    else:
        assert untouched(out, n * 168), (op, n, "wrote past the last slot")
    assert untouched(flags, n * 6 if op in ("isone", "fe") else 0), (op, n, "flags past the last slot")
    return out, flags


@pytest.mark.parametrize("n", eo.HEX_COUNTS)
def test_hex_ops(n):
    """hex_mul / sqr / cyc_sqr / frob / conj / line_at / inv / is_one with n
    slots: partly filled rows (neighbouring trios gone), the second row pair
    of a wave, up to three waves."""
    import random
    rng = random.Random(0x4E8 + n)
    A, B = _hex_elements(n, n), _hex_elements(n, n + 5)
    bump = lambda i: (i % 12, (3 * i + 1) % 12)  # noqa: E731
    Aw = [f12_words(a, bump(i)) for i, a in enumerate(A)]
    unary = {"sqr": bls.f12_sqr, "frob": bls.f12_frob, "conj": bls.f12_conj}
    for op, ref in unary.items():
        out, _ = _hex_launch(op, Aw)
        for s in range(n):
            assert eo.check_f12(f12_from_plain(out[s * 168:(s + 1) * 168]), ref(A[s])) is None, (op, n, s)
    out, _ = _hex_launch("mul", Aw, [f12_words(b) for b in B])
    for s in range(n):
        assert eo.check_f12(f12_from_plain(out[s * 168:(s + 1) * 168]), bls.f12_mul(A[s], B[s])) is None, ("mul", n, s)
    C = cyclotomic(n)
    out, _ = _hex_launch("cyc", [f12_words(c) for c in C])
    for s in range(n):
        assert eo.check_f12(f12_from_plain(out[s * 168:(s + 1) * 168]), bls.f12_sqr(C[s])) is None, ("cyc", n, s)
    Z = _hex_elements(n, n, nonzero=True)
    out, _ = _hex_launch("inv", [f12_words(z, bump(i)) for i, z in enumerate(Z)])
    for s in range(n):
        assert eo.check_f12(f12_from_plain(out[s * 168:(s + 1) * 168]), bls.f12_inv(Z[s])) is None, ("inv", n, s)
    # stored lines (l0, l1', l4') evaluated at (-x, y) per slot, edge coefficients on some
    edge = [0, 1, P - 1, (P - 1) // 2]
    lines, pts, want = [], [], []
    for s in range(n):
        fp = lambda: edge[rng.randrange(4)] if (s + rng.randrange(3)) % 3 == 0 else rng.randrange(P)  # noqa: E731
        l0, l1, l4 = [(fp(), fp()) for _ in range(3)]
        nx, y = fp(), fp()
        lines.append(flat(eo.mont(c) for f2 in (l0, l1, l4) for c in f2))
        pts.append(eo.mont(nx) + eo.mont(y))
        want.append(bls.f12_mul(A[s], eo.line_f12(l0, bls.f2_muls(l1, nx), bls.f2_muls(l4, y))))
    out, _ = _hex_launch("line", Aw, lines=lines, pts=pts)
    for s in range(n):
        assert eo.check_f12(f12_from_plain(out[s * 168:(s + 1) * 168]), want[s]) is None, ("line", n, s)
    # is_one: ones among the others, a one stored as 1 + p, a one with a single coefficient off
    ones = [bls.F12_ONE if s % 2 == 0 else A[s] for s in range(n)]
    words = [f12_words(f, (0,) if s % 4 == 0 else bump(s)) for s, f in enumerate(ones)]
    if n > 2:
        words[2] = list(words[2])
        words[2][11 * NL] ^= 1  # the last Fp of a one: no longer one
        ones[2] = None
    _, flags = _hex_launch("isone", words)
    for s in range(n):
        is1 = ones[s] is not None and bls.f12_is_one(ones[s])
        assert [eo.check_flag(f, is1) for f in flags[6 * s:6 * s + 6]] == [None] * 6, ("isone", n, s)


def test_hex_final_exp():
    """hex_final_exp_in (hex_inv_ni and the out-of-line products inside) and
    hex_is_one of its result, one final exponentiation per element."""
    V = eo.f12_values()
    out, flags = _hex_launch("fe", [f12_words(V[n]) for n in fe_names()])
    for s, n in enumerate(fe_names()):
        want = final_exp_of(n)
        assert eo.check_f12(f12_from_plain(out[s * 168:(s + 1) * 168]), want) is None, n
        assert [eo.check_flag(f, bls.f12_is_one(want)) for f in flags[6 * s:6 * s + 6]] == [None] * 6, n


# ---------------------------------------------------------------------------
# lane pair
def _fp2_list():
    import random
    rng = random.Random(0x9A12)
    e = eo.CANON_EDGES
    vs = [(a, b) for a in e[:6] for b in e[:6]]
    vs += [(e[i], rng.randrange(P)) for i in range(len(e))] + [(rng.randrange(P), e[i]) for i in range(len(e))]
    vs += [(rng.randrange(P), rng.randrange(P)) for _ in range(19)]
    return [(a % P, b % P) for a, b in vs]


def _fp2_words(x, bump=False):
    return eo.limbs(x[0] * eo.R % P + (P if bump else 0)) + eo.mont(x[1])


def _fp2_from(words):
    w = [int(v) for v in words]
    assert all(0 <= v <= eo.M28 for v in w), "limbs not below 2^28"
    return (eo.unmont(w[:NL]), eo.unmont(w[NL:2 * NL]))


def test_pair_ops():
    A = _fp2_list()
    n = len(A)
    assert n % 32 != 0  # the last wave is partly filled
    B = [A[(i * 7 + 3) % n] for i in range(n)]
    cap = n + 2
    psi_x = bls.f2_inv(bls.f2_pow((1, 1), (P - 1) // 3))
    refs = {"mul": lambda a, b: bls.f2_mul(a, b), "sqr": lambda a, b: bls.f2_sqr(a),
            "inv": lambda a, b: bls.f2_inv(a) if a != (0, 0) else (0, 0), "conj": lambda a, b: bls.f2_conj(a),
            "mul_xi": lambda a, b: bls.f2_mul_xi(a), "mul_const": lambda a, b: bls.f2_mul(a, psi_x)}
    aw = u32(flat(_fp2_words(a, i % 3 == 0) for i, a in enumerate(A)))
    bw = u32(flat(_fp2_words(b) for b in B))
    for op, ref in refs.items():
        out = sentinel(cap * 2 * NL)
        call("dc_pair", PAIR_OPS.index(op), aw, bw, out, None, n, cap)
        assert untouched(out, n * 2 * NL), op
        for i in range(n):
            assert _fp2_from(out[i * 28:(i + 1) * 28]) == ref(A[i], B[i]), (op, i, A[i], B[i])
    # gather: the whole Fp2, limb for limb, on both lanes
    out = sentinel(cap * 4 * NL)
    call("dc_pair", PAIR_OPS.index("gather"), aw, None, out, None, n, cap)
    assert untouched(out, n * 4 * NL)
    for i in range(n):
        want = [int(w) for w in aw[i * 28:(i + 1) * 28]]
        assert list(out[i * 56:i * 56 + 28]) == want and list(out[i * 56 + 28:i * 56 + 56]) == want, ("gather", i)
    # f_eq / f_is_zero: equal in another representation, one component off, zero as p
    E = []
    for i, a in enumerate(A):
        k = i % 4
        E.append(a if k == 0 else ((a[0], (a[1] + 1) % P) if k == 1 else (((a[0] + 1) % P, a[1]) if k == 2 else B[i])))
    ew = u32(flat(_fp2_words(b, i % 3 != 0) for i, b in enumerate(E)))
    flags = sentinel(cap * 2)
    call("dc_pair", PAIR_OPS.index("eq"), aw, ew, None, flags, n, cap)
    assert untouched(flags, 2 * n)
    for i in range(n):
        want = (1 if A[i] == E[i] else 0) | (2 if A[i] == (0, 0) else 0)
        assert list(flags[2 * i:2 * i + 2]) == [want, want], ("eq", i, A[i], E[i])
    assert sum(1 for a in A if a == (0, 0)) >= 1 and sum(1 for a in A if 0 in a and a != (0, 0)) >= 2


def test_pair_lines():
    """px_g2_lines<true>, one lane pair per point, against the host g2_lines."""
    pts = eo.g2_points()
    n, cap = len(pts), len(pts) + 1
    out = sentinel(cap * 68 * 6 * NL)
    call("dc_pair_lines", u32(flat(eo.g2_raw(q) for q in pts)), out, n, cap)
    assert untouched(out, n * 68 * 6 * NL)
    for i, q in enumerate(pts):
        err = eo.check_lines(list(out[i * 5712:(i + 1) * 5712]), _host_lines(q))
        assert err is None, (i, err)


# ---------------------------------------------------------------------------
# workgroup batch inversion
def _waves():
    return sorted({devcheck.lib().dc_binv_waves(), 4})


ONE_M = eo.mont(1)


@pytest.mark.parametrize("n", eo.BATCH_INV_SIZES)
def test_block_batch_inv(n):
    vals, present = eo.batch_inv_case(n)
    for waves in _waves():
        cap = n + 5
        out = sentinel(cap * NL)
        call("dc_batch_inv", waves, u32(flat(eo.mont(v) for v in vals)), u32(present), out, n, cap)
        assert untouched(out, n * NL), (waves, n)
        for i, (v, pz) in enumerate(zip(vals, present)):
            got = list(out[i * NL:(i + 1) * NL])
            if pz:
                err = eo.check_plain(got, ("mod", pow(v, P - 2, P) * eo.R, 2 * P))
                assert err is None, (waves, n, i, err)
            else:
                assert got == ONE_M, (waves, n, i, "an absent value must come back as 1")


@pytest.mark.parametrize("g", [1, 2])
def test_block_jac_to_aff(g):
    """block_jac_to_aff: x = X / Z^2, y = Y / Z^3 with the inversion batched;
    infinity (Z = 0) and unwanted points report false and leave `out` alone."""
    import random
    for n in (1, 65, 300):
        rng = random.Random(0x7A + 16 * g + n)
        fe = lambda: tuple(rng.randrange(1, P) for _ in range(g))  # noqa: E731
        pts = [(fe(), fe(), fe()) for _ in range(n)]
        _, want = eo.batch_inv_case(n)
        if n > 8:
            pts[5] = (pts[5][0], pts[5][1], (0,) * g)  # infinity, wanted
            want[5] = 1
            if g == 2:
                pts[6] = (pts[6][0], pts[6][1], (0, pts[6][2][1]))  # Z = z1 u: not infinity
                want[6] = 1
        words = flat(eo.mont(c) for p in pts for f in p for c in f)
        for waves in _waves():
            cap = n + 2
            out = sentinel(cap * 2 * g * NL)
            ok = sentinel(cap)
            call("dc_jac_to_aff", g, waves, u32(words), u32(want), out, ok, n, cap)
            assert untouched(out, n * 2 * g * NL) and untouched(ok, n)
            for i, (X, Y, Z) in enumerate(pts):
                got = out[i * 2 * g * NL:(i + 1) * 2 * g * NL]
                present = bool(want[i]) and any(Z)
                assert ok[i] == int(present), (g, waves, n, i)
                if not present:
                    assert all(w == SENT for w in got), (g, waves, n, i, "out written for an absent point")
                    continue
                if g == 1:
                    zi = pow(Z[0], P - 2, P)
                    ref = [X[0] * zi * zi % P, Y[0] * zi * zi * zi % P]
                else:
                    zi = bls.f2_inv(Z)
                    zi2 = bls.f2_sqr(zi)
                    ref = list(bls.f2_mul(X, zi2)) + list(bls.f2_mul(Y, bls.f2_mul(zi2, zi)))
                for k in range(2 * g):
                    err = eo.check_plain(list(got[k * NL:(k + 1) * NL]), ("mod", ref[k] * eo.R, 2 * P))
                    assert err is None, (g, waves, n, i, k, err)
