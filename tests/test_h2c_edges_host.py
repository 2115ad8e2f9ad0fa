"""The directed inputs of tests/edge_h2c.py on the CPU: the (u0, u1) pairs and
the square-root values through the HOST build of the device math
(tests/hostcheck: hc_map_pair_u, hc_sqrt_or_z; TBG_BOUNDS_CHECK on, so a limb
form outside bls_field.h's documented ranges aborts the process), and the
lists' own claims -- which rare branch each item reaches, and that the
expected values agree with the oracle's independent forms -- in Python
integers.  Passing here is what licenses sending the same lists to the GPU
(tests/test_gpu_devcheck_h2c.py)."""
import ctypes
import math

from oracle import bls12_381 as bls
from tests import edge_h2c as eh
from tests import edge_operands as eo
from tests.edge_points import add, bank, mul, neg, psi
from tests.hostcheck import lib

P = bls.P


def _u(words):
    return (ctypes.c_uint32 * len(words))(*words)


def host_map_pair(u0, u1):
    q0, q1 = _u([eo.SENTINEL] * eh.JAC_W), _u([eo.SENTINEL] * eh.JAC_W)
    lib().hc_map_pair_u(_u(eh.fp2_words(u0)), _u(eh.fp2_words(u1)), q0, q1)
    return list(q0), list(q1)


def host_sqrt(a):
    root = _u([eo.SENTINEL] * eh.FP2_W)
    flags = lib().hc_sqrt_or_z(_u(eh.fp2_words(a)), root)
    return flags, list(root)


def _alternates(kinds, ordinary):
    """Rare and ordinary items side by side: no two rare neighbours, and a
    rare item at every other position while they last."""
    rare = [not k.startswith(ordinary) for k in kinds]
    assert not any(a and b for a, b in zip(rare, rare[1:]))
    last = max(i for i, r in enumerate(rare) if r)
    assert all(rare[i] for i in range(1, last + 1, 2))


def test_u_pairs_on_host():
    pairs = eh.u_pairs()
    for i, (kind, u0, u1) in enumerate(pairs):
        q0, q1 = host_map_pair(u0, u1)
        for q, u in ((q0, u0), (q1, u1)):
            err = eh.check_jac(q, eh.map_point(u))
            assert err is None, (i, kind, err)


def test_sqrt_values_on_host():
    for i, (kind, a) in enumerate(eh.sqrt_values()):
        flags, root = host_sqrt(a)
        err = eh.check_sqrt(a, flags, root)
        assert err is None, (i, kind, err)


def test_u_pair_list_holds_the_directed_cases():
    pairs = eh.u_pairs()
    kinds = [k for k, _, _ in pairs]
    assert len(pairs) > 64 and len(pairs) % 64 != 0
    _alternates(kinds, "sq")
    assert {"sq11", "sq10", "sq01", "sq00"} <= set(kinds)
    for kind, u0, u1 in pairs:
        q0, q1 = eh.map_point(u0), eh.map_point(u1)
        assert q0 is not None and q1 is not None and bls.g2_on_curve(q0) and bls.g2_on_curve(q1)
        if kind.startswith("sq"):
            assert kind == "sq%d%d" % (eh.gx1_is_square(u0), eh.gx1_is_square(u1))
        if kind.startswith("zero"):  # the denominator product is zero: no batched inverse for this message
            assert eh.sswu_x1(u0) is None or eh.sswu_x1(u1) is None
        else:
            assert eh.sswu_x1(u0) is not None and eh.sswu_x1(u1) is not None
        if kind in ("same", "zero_both"):  # Q0 == Q1: k_hash_clear_x1's first addition is a doubling
            assert "sum" in eh.clear_sites(q0, q1)
        if kind == "opposite":  # y takes u's sign: Q1 = -Q0, the identity runs through the clearing
            assert q1 == neg(q0) and eh.clear_steps(add(q0, q1)) == (None, None, None)
        assert "mul" not in eh.clear_sites(q0, q1)
    # the whole chain's value against the oracle's own composition
    for kind, u0, u1 in pairs[:8]:
        p = add(eh.map_point(u0), eh.map_point(u1))
        assert eh.clear_steps(p)[2] == bls.clear_cofactor_g2(p)


def test_sswu_slot_list_holds_the_directed_cases():
    slots = eh.sswu_slots()
    kinds = [s[0] for s in slots]
    assert len(slots) % 2 == 0 and len(slots) > 64 and len(slots) % 64 != 0
    _alternates(kinds, "ordinary")
    assert eh.sswu_gx(eh.X1_REAL_GX)[1] == 0  # the closed-form root refuses: g(x1) lies in Fp
    for kind, u, x1, flag in slots:
        assert flag == (0 if kind == "no_inverse" else 1)
        if kind == "ordinary":
            assert x1 == eh.sswu_x1(u)
            assert eh.sqrt_model(eh.sswu_gx(x1))[0]  # the closed form covers it
        if kind == "real_gx":
            assert x1 == eh.X1_REAL_GX and not eh.sqrt_model(eh.sswu_gx(x1))[0]
        assert eh.map_point(u) is not None


def test_sqrt_list_holds_the_directed_cases():
    vals = eh.sqrt_values()
    kinds = [k for k, _ in vals]
    assert len(vals) > 64 and len(vals) % 64 != 0
    _alternates(kinds, "sq")
    seen = set()
    for kind, a in vals:
        flag, sq, arm = eh.sqrt_model(a)
        assert sq == bls.f2_is_square(a)
        if kind.startswith("sq"):
            assert flag and kind == "sq%d_arm%d" % (sq, arm)
            seen.add((sq, arm))
        elif kind == "imaginary":  # c0 == 0: delta is gamma / 2 alone
            assert flag and a[0] == 0
        else:
            assert not flag, kind
            # the two exits: a in Fp (every element of Fp is a square in Fp2), or a non-square with Z a in Fp
            assert (sq and a[1] == 0) or (not sq and bls.f2_mul(eh.Z, a)[1] == 0)
        if kind == "over_z":
            assert not sq
        if kind in ("zero", "fp_square", "fp_nonresidue", "imaginary"):
            assert sq
    assert seen == {(True, True), (True, False), (False, True), (False, False)}  # both arms of the final select


def test_clear_lists_hold_the_directed_cases():
    pairs = eh.clear_pairs()
    kinds = [k for k, _, _ in pairs]
    assert len(pairs) > 32 and len(pairs) % 32 != 0
    _alternates(kinds, "generic")
    b = bank()
    assert psi(b["g"][0]) == eh.mul_x(b["g"][0])  # psi acts as [x] on G2
    reached = set()
    for kind, q0, q1 in pairs:
        p = add(q0, q1)
        sites = eh.clear_sites(q0, q1)
        assert "mul" not in sites  # px_mul_x_complete: not reachable (module docstring)
        if kind == "double":
            assert "sum" in sites
        elif kind == "g2_sum":
            assert "psi" in sites and (p is None or bls.g2_in_subgroup(p))
        else:
            assert kind in ("generic", "cancel", "inf_q0", "inf_q1", "inf_both")
            assert not sites
        reached |= sites
        h = eh.clear_steps(p)[2]
        assert h == eh.clear_formula(p)
        assert h == mul(p, bls.H_EFF_G2)
        assert h is None or bls.g2_in_subgroup(h)
    assert reached == {"sum", "psi"}
    # the order-dividing claim behind "mul": the running multiples of [|x|] P at its five additions
    acc, prefixes = 1, []
    for i in range(62, -1, -1):
        acc *= 2
        if (bls.X_ABS >> i) & 1:
            prefixes.append(acc - 1)
            acc += 1
    # (the first addition meets [2]P == P only at infinity, which jac_add_x handles)
    assert acc == bls.X_ABS and prefixes == [1, 11, 103, 53759, 230901736800255]
    x = bls.X
    h2 = (x**8 - 4 * x**7 + 5 * x**6 - 4 * x**4 + 6 * x**3 - 4 * x**2 - 4 * x + 13) // 9  # #E2(Fp2) = h2 r
    assert mul(b["ns"], h2 * bls.R) is None and mul(b["ns"], bls.R) is not None
    assert all(math.gcd(k, h2 * bls.R) == 1 for k in prefixes)


def test_fin_list_holds_the_directed_cases():
    triples = eh.fin_triples()
    kinds = [t[0] for t in triples]
    assert len(triples) > 32 and len(triples) % 32 != 0
    _alternates(kinds, "generic")
    for kind, p, t1, v in triples:
        sites = eh.fin_sites(p, t1, v)
        assert sites == ({int(kind[3])} if kind.startswith("add") else set()), (kind, sites)
    assert {k for k in kinds if k != "generic"} == {"add1", "add2", "add3", "add4"}


def test_message_list_holds_the_lengths():
    msgs = eh.messages()
    assert len(msgs) == max(eh.MSG_BATCHES) and {len(m) for m in msgs} == set(eh.MSG_LENGTHS)
    # neighbouring lanes compress different numbers of SHA-256 blocks
    blocks = [(len(m) + 3 + 44 + 1 + 8 + 63) // 64 for m in msgs[:64]]
    assert sum(a != b for a, b in zip(blocks, blocks[1:])) >= 16
    u0, u1 = bls.hash_to_field_fp2(msgs[3], bls.DST_POP, 2)
    p = add(eh.map_point(u0), eh.map_point(u1))
    assert eh.clear_steps(p)[2] == eh.hash_point(msgs[3])


def test_checkers_reject_one_limb_off():
    _, u0, u1 = eh.u_pairs()[0]
    q0, _ = host_map_pair(u0, u1)
    assert eh.check_jac(q0, eh.map_point(u0)) is None
    for j in range(0, eh.JAC_W, 5):
        for d in (1, -1):
            w = list(q0)
            w[j] += d
            assert eh.check_jac(w, eh.map_point(u0)) is not None, j
    kind, a = next(v for v in eh.sqrt_values() if v[0].startswith("sq1"))
    flags, root = host_sqrt(a)
    assert eh.check_sqrt(a, flags, root) is None
    assert eh.check_sqrt(a, flags ^ 1, root) is not None and eh.check_sqrt(a, flags ^ 2, root) is not None
    for j in range(eh.FP2_W):
        w = list(root)
        w[j] ^= 1
        assert eh.check_sqrt(a, flags, w) is not None, j
    # a refused value must leave no root behind
    flags, root = host_sqrt((0, 0))
    assert eh.check_sqrt((0, 0), flags, root) is None
    assert eh.check_sqrt((0, 0), flags, [1] + root[1:]) is not None
    # k_hash_affine's output: the point, or status 1 and zeros
    g0 = bank()["g"][0]
    words = eh.fp2_words(g0[0]) + eh.fp2_words(g0[1])
    assert eh.check_affine(words, 0, g0) is None and eh.check_affine(words, 1, g0) is not None
    for j in range(0, eh.AFF_W, 3):
        w = list(words)
        w[j] ^= 1
        assert eh.check_affine(w, 0, g0) is not None, j
    assert eh.check_affine([0] * eh.AFF_W, 1, None) is None
    assert eh.check_affine([0] * eh.AFF_W, 0, None) is not None
    assert eh.check_affine([0] * 5 + [1] + [0] * (eh.AFF_W - 6), 1, None) is not None
