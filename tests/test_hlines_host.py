"""The H(m)-lines kernel's projective Miller steps (charon_amd/csrc/bls_pair.h
hline_dbl_s / hline_add_s, k_lines_h through px_h_lines) on the host: a twin
built from the same headers (tests/hlines, TBG_BOUNDS_CHECK on, so a violated
value or limb bound of the lazy sums aborts the process), in the single-lane
Fp2 form and with the lane pair emulated.

The new steps give each of the 68 lines as the pinned Jacobian form's
(g2_lines, P left out) times one non-zero Fp2 factor.  That is checked step by
step with the oracle's integers (cross products), then where it matters: the
Miller values agree after the final exponentiation, with each other and with
the oracle's pairing, and a signature verifies with H(m)'s lines from the new
steps beside the signature's lines from the pinned ones.
"""
import ctypes
import json
import os
import random

import pytest

from oracle import bls12_381 as bls
from tests import hlines

P = bls.P
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = hlines.N_LINES


def gold(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)["vectors"]


@pytest.fixture(scope="module")
def hl():
    return hlines.lib()


@pytest.fixture(scope="module")
def points(hl):
    """H(m) of fixture messages, G2's generator, 16 seeded random multiples."""
    msgs = [gold("cfg1_3of4_single.json")[0]["msg"]] + [v["msg"] for v in gold("cfg2_3of4_sample.json")[:3]] + \
        [v["msg"] for v in gold("kat_verify.json")[:2]]
    rng = random.Random(0x41A5)
    pts = [("H(%s..)" % m[:8], hlines.h_of(bytes.fromhex(m))) for m in msgs]
    pts.append(("generator", bls.G2_GEN))
    pts += [("multiple %d" % k, bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))) for k in range(16)]
    return pts


def steps(hl, q, form):
    new, ref, end = (ctypes.create_string_buffer(288 * N), ctypes.create_string_buffer(288 * N),
                     ctypes.create_string_buffer(192))
    assert hl.hl_steps(hlines.aff192(q), form, new, ref, end) == 0

    def triples(buf):
        return [tuple(hlines.b2f(buf.raw[288 * i + 96 * k:288 * i + 96 * k + 96]) for k in range(3)) for i in range(N)]
    return triples(new), triples(ref), (hlines.b2f(end.raw[:96]), hlines.b2f(end.raw[96:]))


@pytest.mark.parametrize("form", [0, 1], ids=["Fp2", "pair"])
def test_every_step_is_the_pinned_line_up_to_one_factor(hl, points, form):
    for name, q in points:
        assert bls.g2_on_curve(q)
        new, ref, end = steps(hl, q, form)
        for i, ((n0, n1, n4), (r0, r1, r4)) in enumerate(zip(new, ref)):
            assert n4 != (0, 0), (name, i)
            assert bls.f2_mul(n0, r1) == bls.f2_mul(n1, r0), (name, i)
            assert bls.f2_mul(n0, r4) == bls.f2_mul(n4, r0), (name, i)
            assert bls.f2_mul(n1, r4) == bls.f2_mul(n4, r1), (name, i)
        assert end == bls.g2_mul_raw(q, bls.X_ABS), name


def test_both_forms_give_the_same_lines(hl, points):
    for name, q in points[:3] + points[-2:]:
        assert steps(hl, q, 0)[0] == steps(hl, q, 1)[0], name


def pairing_bytes(hl, p, q, which):
    out = ctypes.create_string_buffer(576)
    assert hl.hl_pairing(p[0].to_bytes(48, "big") + p[1].to_bytes(48, "big"), hlines.aff192(q), which, out) == 0
    return out.raw


@pytest.fixture(scope="module")
def pairs(points):
    rng = random.Random(0x9A17)
    qs = [points[0][1], points[6][1], points[7][1], points[-1][1]]  # an H(m), the generator, two multiples
    return [(bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R)), q) for q in qs]


def f12_bytes(f):
    return b"".join(v.to_bytes(48, "big") for six in f for c in six for v in c)


def test_pairing_agrees_after_the_final_exponentiation(hl, pairs):
    for p, q in pairs:
        new = pairing_bytes(hl, p, q, 0)
        assert new == pairing_bytes(hl, p, q, 1)
        assert new == f12_bytes(bls.pairing(p, q))


def test_a_negated_l1_is_seen(hl, pairs):
    """The control: a sign slip in one coefficient changes the pairing value."""
    for p, q in pairs:
        assert pairing_bytes(hl, p, q, 2) != pairing_bytes(hl, p, q, 1)


def test_signature_verifies_with_mixed_line_forms(hl):
    v = gold("cfg1_3of4_single.json")[0]
    pk, msg, sig = bytes.fromhex(v["tss"]["public_key"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["expect"]["agg"])
    assert hl.hl_verify(pk, msg, len(msg), sig) == 1
    bad = bytearray(msg)
    bad[-1] ^= 1
    assert hl.hl_verify(pk, bytes(bad), len(bad), sig) == 0
    for k in gold("kat_verify.json"):
        if k["expect"] == "valid":
            m = bytes.fromhex(k["msg"])
            assert hl.hl_verify(bytes.fromhex(k["pk"]), m, len(m), bytes.fromhex(k["sig"])) == 1
            break
