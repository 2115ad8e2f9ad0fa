"""Directed operands for the hexad's direct line product, shared by
tests/test_hex_line_direct_host.py and tests/test_gpu_hex_line_direct.py.

Every Fp is given as its STORED integer x (Montgomery domain, 0 <= x < 2p,
written out as 14 limbs of 28 bits): what a lane holds.  Its field value is
x / R mod p.
"""
import random

from oracle import bls12_381 as bls
from tests import edge_operands as eo

P = eo.P
NL = eo.NL
M28 = (1 << 28) - 1


def max_limbs_below(bound):
    """The largest value below `bound` whose limbs 0 .. 12 are all 2^28 - 1."""
    low = (1 << 364) - 1
    top = (bound - 1) >> 364
    if (top << 364) | low >= bound:
        top -= 1
    assert top >= 0
    return (top << 364) | low


ONE = eo.R % P            # the field's 1
MAXL = max_limbs_below(2 * P)
# what one component of f is set to: 0, the field's 1, the word 1, p - 1, the
# non-canonical 2p - 1, every limb but the top one at 2^28 - 1
F_EDGES = [0, ONE, 1, P - 1, 2 * P - 1, MAXL]
LINE_EDGES = [0, P - 1, MAXL]


def _rnd(rng):
    return rng.randrange(2 * P)


def case(name, f, line, pt):
    assert len(f) == 12 and len(line) == 6 and (pt is None or len(pt) == 2)
    assert all(0 <= x < 2 * P for x in list(f) + list(line) + list(pt or ()))
    return {"name": name, "f": list(f), "line": list(line), "pt": None if pt is None else list(pt)}


def cases():
    """Every directed case once with an unevaluated line and a point
    (hex_line_at_v) and once with the line taken as evaluated
    (hex_line_folded)."""
    rng = random.Random(0x11E)
    base = []

    def add(name, f=None, line=None, pt=None):
        base.append((name, f or [_rnd(rng) for _ in range(12)], line or [_rnd(rng) for _ in range(6)],
                     pt or [_rnd(rng), _rnd(rng)]))

    for i in range(6):
        add(f"random{i}")
    add("f_is_one", f=[ONE] + [0] * 11)
    for e, x in enumerate(F_EDGES):
        add(f"f_all_edge{e}", f=[x] * 12)
        for i in range(12):
            f = [_rnd(rng) for _ in range(12)]
            f[i] = x
            add(f"f{i}_edge{e}", f=f)
    for e, x in enumerate(LINE_EDGES):
        add(f"line_all_edge{e}", line=[x] * 6)
        add(f"point_edge{e}", pt=[x, x])
        for i in range(6):
            line = [_rnd(rng) for _ in range(6)]
            line[i] = x
            add(f"line{i}_edge{e}", line=line)
    add("all_max_limbs", f=[MAXL] * 12, line=[MAXL] * 6, pt=[MAXL, MAXL])
    # l0 = l4 as coefficients, and l1, l4 with equal components: D = y0 - y1 = 0
    l = [_rnd(rng) for _ in range(6)]
    add("l0_eq_l4", line=[l[0], l[1], l[2], l[3], l[0], l[1]])
    add("d4_zero", line=[l[0], l[1], l[2], l[3], l[4], l[4]])
    add("d1_zero", line=[l[0], l[1], l[2], l[2], l[4], l[5]])
    add("d_all_zero", line=[l[0], l[0], l[2], l[2], l[4], l[4]], pt=[l[5], l[5]])
    out = []
    for name, f, line, pt in base:
        out.append(case(name + "/at", f, line, pt))
        out.append(case(name + "/folded", f, line, None))
    return out


def words(xs):
    return [w for x in xs for w in eo.limbs(x)]


def expect(c):
    """f * line in the oracle's tower."""
    v = [x * eo.RINV % P for x in c["f"]]
    l = [x * eo.RINV % P for x in c["line"]]
    l0, l1, l4 = (l[0], l[1]), (l[2], l[3]), (l[4], l[5])
    if c["pt"] is not None:
        nx, y = [x * eo.RINV % P for x in c["pt"]]
        l1, l4 = bls.f2_muls(l1, nx), bls.f2_muls(l4, y)
    return bls.f12_mul(eo.quad_to_f12(v), eo.line_f12(l0, l1, l4))
