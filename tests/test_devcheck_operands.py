"""The directed operand lists of tests/edge_operands.py through the HOST build
of the device math (tests/hostcheck, TBG_BOUNDS_CHECK on) against Python
integers and the oracle.

A violated precondition aborts the process: passing here is what licenses
sending the same lists to the GPU (tests/test_gpu_devcheck.py).  Also the
tests of the result checkers themselves: a correct result passes, the same
result with one limb off by one does not."""
import ctypes

import pytest

from oracle import bls12_381 as bls
from tests import edge_operands as eo
from tests.devcheck import FP_OPS, ROW_OPS
from tests.hostcheck import lib

P = eo.P
U32x14 = ctypes.c_uint32 * 14
I32x14 = ctypes.c_int32 * 14


def _u(l):
    return U32x14(*[int(v) & 0xFFFFFFFF for v in l])


def host_fp(op, t):
    ops = [x for x in t if isinstance(x, list)]
    k = next((x for x in t if isinstance(x, int)), 0)
    args = [_u(x) for x in ops] + [None] * (4 - len(ops))
    out = U32x14()
    assert lib().hc_fp_op_raw(FP_OPS.index(op), *args, ctypes.c_uint32(k), out) == 0
    return list(out)


def host_row(op, t):
    args = [I32x14(*x) for x in t] + [None] * (4 - len(t))
    out = (ctypes.c_int32 * 16)()
    assert lib().hc_row_op_raw(ROW_OPS.index(op), *args, out) == 0
    return list(out)


@pytest.mark.parametrize("op", FP_OPS)
def test_fp_lists_on_host(op):
    cases = eo.fp_cases()[op]
    assert len(cases) >= 20
    for t in cases:
        err = eo.check_plain(host_fp(op, t), eo.fp_expect(op, t))
        assert err is None, (op, t, err)


@pytest.mark.parametrize("op", ROW_OPS)
def test_row_lists_on_host(op):
    cases = eo.row_cases()[op]
    assert len(cases) >= (6400 if op == "mul2" else 100)
    for t in cases:
        err = eo.check_row(host_row(op, t), eo.row_expect(op, t))
        assert err is None, (op, t, err)


def test_lists_hold_the_directed_edges():
    """The lists reach what they are for: limbs at 2^31 - 1 into a product,
    a reduction on each side of the largest multiple of p, row limbs at
    +-2^29."""
    c = eo.fp_cases()
    assert any(max(a) == (1 << 31) - 1 for a, _ in c["mul"])
    assert any(max(a) == (1 << 31) - 1 for a, _, _, _ in c["mul2"])
    vals = {eo.val(a) for (a,) in c["reduce"]}
    assert {eo.Q_MAX * P - 1, eo.Q_MAX * P, eo.Q_MAX * P + 1} <= vals
    assert any(max(a) >= (1 << 30) and eo.val(a) % P == 0 for (a,) in c["reduce"])
    assert (1 << 390) - 1 >= max(vals) > (1 << 389)
    r = eo.row_cases()
    assert any(max(a[:13]) == (1 << 29) and min(b[:13]) == -(1 << 29) for a, b, _, _ in r["mul2"])
    assert len({tuple(a) for a, _, _, _ in r["mul2"]}) >= 80


# ---------------------------------------------------------------------------
def be(x):
    return x.to_bytes(48, "big")


def f12b(f):
    return b"".join(be(c[0]) + be(c[1]) for h in f for c in h)


def b2f12(bb):
    xs = [(int.from_bytes(bb[96 * i:96 * i + 48], "big"), int.from_bytes(bb[96 * i + 48:96 * i + 96], "big"))
          for i in range(6)]
    return (tuple(xs[:3]), tuple(xs[3:]))


def call12(fn, *args):
    ob = ctypes.create_string_buffer(576)
    rc = getattr(lib(), fn)(*args, ob)
    return b2f12(ob.raw), rc


def test_fp12_lists_on_host():
    V = eo.f12_values()
    names = list(V)
    for i, n in enumerate(names):
        a, b = V[n], V[names[(i + 5) % len(names)]]
        for fn in ("hc_row_fp12_mul", "hc_hex_mul"):
            assert call12(fn, f12b(a), f12b(b))[0] == bls.f12_mul(a, b), (fn, n)
        for fn in ("hc_row_fp12_frob", "hc_hex_frob"):
            assert call12(fn, f12b(a))[0] == bls.f12_frob(a), (fn, n)
        assert call12("hc_hex_conj", f12b(a))[0] == bls.f12_conj(a), n
        assert call12("hc_hex_sqr", f12b(a))[0] == bls.f12_sqr(a), n
        if n in ("one", "cyclo"):
            for fn in ("hc_row_fp12_cyc", "hc_hex_cyc_sqr"):
                assert call12(fn, f12b(a))[0] == bls.f12_sqr(a), (fn, n)
        if n != "zero":
            want = bls.final_exp(a)
            got, one = call12("hc_row_final_exp", f12b(a))
            assert got == want and one == int(bls.f12_is_one(want)), n
            assert call12("hc_hex_final_exp", f12b(a))[0] == want, n
    assert bls.f12_is_one(bls.final_exp(V["cancel"])) and not bls.f12_is_one(bls.final_exp(V["pairing"]))


def test_batch_inverse_cases_on_host():
    for n in eo.BATCH_INV_SIZES:
        vals, present = eo.batch_inv_case(n)
        for waves in (1, 4):
            out = ctypes.create_string_buffer(48 * n)
            lib().hc_batch_inv(b"".join(be(v) for v in vals), bytes(present), n, waves, out)
            for i, (v, pz) in enumerate(zip(vals, present)):
                assert int.from_bytes(out.raw[48 * i:48 * i + 48], "big") == (pow(v, P - 2, P) if pz else 1)


def host_lines(q):
    out = (ctypes.c_uint32 * (68 * 6 * 14))()
    lib().hc_g2_lines_raw((ctypes.c_uint32 * 56)(*eo.g2_raw(q)), out)
    return list(out)


def test_line_points_on_host():
    for q in eo.g2_points():
        aff = be(q[0][0]) + be(q[0][1]) + be(q[1][0]) + be(q[1][1])
        assert lib().hc_row_lines(aff) == 0
        ref = host_lines(q)
        assert eo.check_lines(ref, ref) is None
        # the first line's l0 is 3 x^3 - 2 y^2 up to the Montgomery factor
        x, y = q
        l0 = bls.f2_sub(bls.f2_muls(bls.f2_mul(bls.f2_sqr(x), x), 3), bls.f2_muls(bls.f2_sqr(y), 2))
        assert (eo.unmont(ref[:14]), eo.unmont(ref[14:28])) == l0


# ---------------------------------------------------------------------------
# the checkers: a correct result passes, one limb off by one does not
def _perturbed(words, idxs):
    for j in idxs:
        for d in (1, -1):
            w = list(words)
            w[j] += d
            yield w


@pytest.mark.parametrize("op", ["mul", "add", "sub", "mul_small", "reduce", "canon", "inv", "from_signed"])
def test_plain_checker_rejects_one_limb_off(op):
    for t in eo.fp_cases()[op][:6] + eo.fp_cases()[op][-6:]:
        got, exp = host_fp(op, t), eo.fp_expect(op, t)
        assert eo.check_plain(got, exp) is None
        for w in _perturbed(got, range(14)):
            assert eo.check_plain(w, exp) is not None, (op, t, w)


def test_plain_checker_range_and_limb_bounds():
    exp = ("mod", 5, 2 * P)
    assert eo.check_plain(eo.limbs(5 + P), exp) is None
    assert eo.check_plain(eo.limbs(5 + 2 * P), exp) is not None      # right residue, outside [0, 2p)
    assert eo.check_plain(eo.limbs(5 + P), ("mod", 5, P)) is not None  # canonical wanted
    l = eo.limbs(5 + P)
    l[0] += 1 << 28
    l[1] -= 1
    assert eo.val(l) == 5 + P and eo.check_plain(l, exp) is not None  # right value, a limb at 2^28


@pytest.mark.parametrize("op", ROW_OPS)
def test_row_checker_rejects_one_limb_off(op):
    for t in eo.row_cases()[op][:5] + eo.row_cases()[op][-5:]:
        got, exp = host_row(op, t), eo.row_expect(op, t)
        assert eo.check_row(got, exp) is None
        for w in _perturbed(got, range(16)):
            assert eo.check_row(w, exp) is not None, (op, t, w)
    w = eo.signed_limbs(3) + [0, 0]
    assert eo.check_row(w, ("mod", 3)) is None
    assert eo.check_row(eo.signed_limbs(3 + 2 * P) + [0, 0], ("mod", 3)) is not None
    assert eo.check_row(eo.signed_limbs(3 - 2 * P) + [0, 0], ("mod", 3)) is not None
    w[0], w[1] = w[0] + (1 << 29), w[1] - 2
    assert eo.val(w) == 3 and eo.check_row(w, ("mod", 3)) is not None


def test_fp12_flag_and_line_checkers_reject_one_off():
    V = eo.f12_values()
    a = V["rand0"]
    quad = eo.f12_to_quad(a)
    assert eo.quad_to_f12(quad) == a
    assert eo.check_f12(quad, a) is None
    assert eo.check_f12([v + P for v in quad], a) is None  # reduced mod p first
    for w in _perturbed(quad, range(12)):
        assert eo.check_f12(w, a) is not None
    # through the limbs: one limb of one Montgomery coefficient off by one
    ls = [eo.mont(v) for v in quad]
    assert eo.check_f12([eo.unmont(l) for l in ls], a) is None
    ls[7][3] += 1
    assert eo.check_f12([eo.unmont(l) for l in ls], a) is not None
    assert eo.check_flag(1, True) is None and eo.check_flag(0, False) is None
    assert eo.check_flag(0, True) is not None and eo.check_flag(1, False) is not None
    ref = host_lines(eo.g2_points()[0])
    for j in (0, 13, 14 * 6 * 67 + 5, len(ref) - 1):
        for w in _perturbed(ref, [j]):
            assert eo.check_lines(w, ref) is not None


# ---------------------------------------------------------------------------
# the lane-pair G2 group law (tests/edge_points.py; the GPU run:
# test_gpu_devcheck_g2.py)
from tests import edge_points as ep  # noqa: E402


def host_g2(op, aw, bw):
    a = (ctypes.c_uint32 * len(aw))(*aw)
    b = (ctypes.c_uint32 * len(bw))(*bw) if bw is not None else None
    out = (ctypes.c_uint32 * 84)(*([eo.SENTINEL] * 84))
    flag = ctypes.c_uint32(eo.SENTINEL)
    assert lib().hc_g2_op_raw(ep.OPS.index(op), a, b, out, ctypes.byref(flag)) == 0
    return list(out), flag.value


@pytest.mark.parametrize("op", ep.OPS)
def test_g2_lists_on_host(op):
    cases = ep.cases()[op]
    assert len(cases) >= 8
    for i, (aw, bw, expect) in enumerate(cases):
        words, flag = host_g2(op, aw, bw)
        err = ep.check(op, words, flag, expect)
        assert err is None, (op, i, err)
        if op == "in_subgroup_aff":
            assert words == [eo.SENTINEL] * 84


def test_g2_lists_hold_the_directed_cases():
    """The lists reach what they are for, and the restated schedules agree
    with the oracle where it has the operation."""
    c, b = ep.cases(), ep.bank()
    for op in ("add_x", "add_aff_x"):
        excs = [e[1] for _, _, e in c[op]]
        infs = [e[0] is None and not e[1] for _, _, e in c[op]]
        assert sum(excs) >= 8 and sum(infs) >= 8 and len(excs) > 32 and len(excs) % 32 != 0
        # neighbouring pairs differ in kind: no run of three equal outcomes
        kinds = [(e[1], e[0] is None) for _, _, e in c[op]]
        assert all(len({kinds[i], kinds[i + 1], kinds[i + 2]}) > 1 for i in range(30))
    # every pattern of empty buckets; many of them add the running sum to itself
    sums = c["sgb_sums"]
    assert len(sums) >= 64 + 4
    n_exc = sum(e[1] for _, _, e in sums[:64])
    assert 20 <= n_exc < 64
    assert sums[0][2] == (None, False, False)                       # all empty
    assert sums[1][2] == (b["g"][0], False, False)                  # only bucket 1
    assert sums[2][2][1] is True                                    # only bucket 2: run + run
    assert sums[64][2][1] is True                                   # all buckets equal
    for (_, _, fast), (_, _, full) in zip(sums, c["sgb_sums_complete"]):
        assert fast[1] or fast[0] == full[0]                        # without exc the two agree
    assert any(e[1] for _, _, e in c["sgb_fold"]) and not all(e[1] for _, _, e in c["sgb_fold"])
    # the oracle's own decisions
    g0 = b["g"][0]
    assert ep.psi(g0) == bls.g2_mul(g0, bls.X % bls.R)              # psi acts as [x] on G2
    verdicts = [e[2] for _, _, e in c["in_subgroup_aff"]]
    pts = [g0, b["tor"], b["ns"], b["g"][1], b["t13"], b["t23"], b["g"][2], b["g"][3]]
    assert len(verdicts) == len(pts)
    for v, p, (_, _, e) in zip(verdicts, pts, c["in_subgroup_aff"]):
        assert e[1] or v == bls.g2_in_subgroup(p)
    assert verdicts.count(True) == 4
    for (_, _, e), p in zip(c["clear_cofactor"], [g0, b["tor"], b["ns"]]):
        if not e[1]:
            assert e[0] == bls.clear_cofactor_g2(p)
    assert c["clear_cofactor"][2][2][1] is False and c["clear_cofactor"][2][2][0] is not None  # E2 outside G2
    assert bls.g2_in_subgroup(c["clear_cofactor"][2][2][0])
    for (_, _, e), p in zip(c["mul_xabs_x"], pts[:3]):
        if not e[1]:
            assert e[0] == bls.g2_mul_raw(p, bls.X_ABS)


def test_g2_checker_rejects_one_limb_off():
    for op in ("add_x", "add_in", "dbl_lo", "psi", "sgb_sums_complete"):
        done = 0
        for aw, bw, expect in ep.cases()[op]:
            if expect[0] is None:
                continue
            words, flag = host_g2(op, aw, bw)
            assert ep.check(op, words, flag, expect) is None
            assert ep.check(op, words, flag ^ 1, expect) is not None
            for w in _perturbed(words, range(0, 84, 5)):
                assert ep.check(op, w, flag, expect) is not None, (op, w)
            done += 1
            if done == 3:
                break
        assert done == 3
    # infinity is Z == 0 mod p whatever X and Y hold; a non-zero Z is not infinity
    aw, bw, expect = next(c for c in ep.cases()["add_x"] if c[2][0] is None and not c[2][1])
    words, flag = host_g2("add_x", aw, bw)
    assert ep.check("add_x", words, flag, expect) is None
    words[5 * 14] += 1
    assert ep.check("add_x", words, flag, expect) is not None
    aw, bw, expect = ep.cases()["in_subgroup_aff"][0]
    words, flag = host_g2("in_subgroup_aff", aw, bw)
    assert ep.check("in_subgroup_aff", words, flag, expect) is None
    assert ep.check("in_subgroup_aff", words, flag ^ 2, expect) is not None
