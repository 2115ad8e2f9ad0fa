"""The hexad's direct line product (charon_amd/csrc/bls_hex.h hx_line_cb /
hx_line_ca) on the host.

A lane of a hexad forms each component of f * line as ONE reduced sum of six
Fp products, where the Karatsuba form (hx_line_u / hx_line_t / hx_line2,
retained as the reference) reduces five sums of two.  tests/hexline compiles
the per-lane pieces for the CPU with the value bound checks on
(TBG_BOUNDS_CHECK aborts the process on a violated bound) and runs the six
lanes of a hexad in a loop, for both line sources: stored lines evaluated at
a point (hex_line_at_v) and lines evaluated already (hex_line_folded).

Each directed case (tests/hexline/operands.py) is checked three ways, on
canonical values: against fp12_mul by the sparse element in the device
tower, against the Karatsuba form, and against the oracle's tower.  That
every case returns at all is the bound checks not firing.
"""
import ctypes
import subprocess
import sys

import pytest

from tests import edge_operands as eo
from tests.hexline import operands as ops

P = eo.P
NL = eo.NL


def u32(words):
    return (ctypes.c_uint32 * len(words))(*[int(w) for w in words])


@pytest.fixture(scope="module")
def hc():
    from tests.hexline import lib
    h = lib()
    h.hxl_hc_line.restype = ctypes.c_int
    h.hxl_hc_sum6.restype = ctypes.c_int
    h.hxl_hc_neg_l.restype = ctypes.c_int
    h.hxl_hc_columns_fit.restype = ctypes.c_int
    h.hxl_hc_columns_fit.argtypes = [ctypes.c_double]
    return h


def run_line(hc, c):
    outs = [(ctypes.c_uint32 * 168)() for _ in range(4)]
    pt = u32(ops.words(c["pt"])) if c["pt"] is not None else None
    assert hc.hxl_hc_line(u32(ops.words(c["f"])), u32(ops.words(c["line"])), pt, *outs) == 0
    return [list(o) for o in outs]


def chunks(xs, n):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


def test_directed_cases(hc):
    cases = ops.cases()
    assert len(cases) > 200
    for c in cases:
        direct, kara, tower, raw = run_line(hc, c)
        assert direct == tower, (c["name"], "direct form differs from fp12_mul by the sparse element")
        assert direct == kara, (c["name"], "direct form differs from the Karatsuba form")
        # the lanes leave REDC outputs: normalised limbs, below 2p
        for l in chunks(raw, NL):
            assert max(l) <= eo.M28 and eo.val(l) < 2 * P, c["name"]
        assert eo.check_f12([eo.unmont(l) for l in chunks(direct, NL)], ops.expect(c)) is None, c["name"]


def test_columns_fit_at_worst_case_limbs(hc):
    """Three of the six left operands are fp_neg_l values (limbs < 2^29), the
    other nine operands normalised: the column fits.  Six lazy operands on
    each side would not."""
    m28, m29, m31 = (1 << 28) - 1, (1 << 29) - 1, (1 << 31) - 1
    assert hc.hxl_hc_columns_fit(float(14 * m28 * (3 * m29 + 3 * m28))) == 1
    assert hc.hxl_hc_columns_fit(float(14 * 6 * m31 * m31)) == 0
    # the lazy negation's limbs stay below 2^29, and 16p - 0 is the largest of them
    out = (ctypes.c_uint32 * NL)()
    for x in (0, 1, P - 1, ops.MAXL):
        assert hc.hxl_hc_neg_l(u32(eo.limbs(x)), out) == 0
        assert max(out) <= m29 and eo.val(list(out)) == 16 * P - x
    assert hc.hxl_hc_neg_l(u32(eo.limbs(0)), out) == 0
    assert min(out[:NL - 1]) >= m28  # every limb of 16p - 0 below the top one at or above 2^28 - 1: the worst case


def sum6_operands():
    """One sum at the bounds' edge: own views just below 2p with limbs 0 .. 12
    at 2^28 - 1, partner views 16p - 0 (the largest lazy negation, every limb
    below the top one >= 2^28 - 1); against them a D just below 18p and an S just below 4p."""
    own = ops.MAXL
    d, s = ops.max_limbs_below(18 * P), ops.max_limbs_below(4 * P)
    left = [eo.limbs(own), "neg0"] * 3
    right = [eo.limbs(d), eo.limbs(s)] * 3
    return left, right, [(own, d), (16 * P, s)] * 3


def test_sum_at_the_edge_of_its_bounds(hc):
    left, right, pairs = sum6_operands()
    neg0 = (ctypes.c_uint32 * NL)()
    assert hc.hxl_hc_neg_l(u32(eo.limbs(0)), neg0) == 0
    left = [list(neg0) if l == "neg0" else l for l in left]
    out = (ctypes.c_uint32 * NL)()
    assert hc.hxl_hc_sum6(u32([w for l in left for w in l]), u32([w for l in right for w in l]), out) == 0
    got = list(out)
    assert max(got) <= eo.M28 and eo.val(got) < 2 * P
    assert eo.val(got) % P == sum(a * b for a, b in pairs) * eo.RINV % P


CHILD = """
import ctypes, sys
from tests.hexline import lib
from tests import edge_operands as eo
from tests.hexline import operands as ops
P = eo.P
u32 = lambda ws: (ctypes.c_uint32 * len(ws))(*ws)
h = lib()
out = (ctypes.c_uint32 * 14)()
kind = sys.argv[1]
if kind == "value":      # 6 * 20p * 18p = 2160 p^2, over the 2048 p^2 a reduction takes
    l, r = eo.limbs(20 * P), eo.limbs(ops.max_limbs_below(18 * P))
elif kind == "columns":  # values below 2p, but every limb lazy, towards 2^31: 84 products of 2^62 in a column
    l = r = eo.lazy(ops.MAXL)
elif kind == "within":   # the same call inside its bounds returns
    l = r = eo.limbs(ops.MAXL)
h.hxl_hc_sum6(u32(l * 6), u32(r * 6), out)
print("returned")
"""


@pytest.mark.parametrize("kind,message", [("value", "hx_line_sum6 bound"), ("columns", "fp_mul_sum columns fit"),
                                          ("within", None)])
def test_bound_checks_are_live(kind, message):
    """An operand set over the value bound and one over the column bound abort
    the process with the bound's name; the same call within bounds returns."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from tests.hexline import build
    build()
    r = subprocess.run([sys.executable, "-c", CHILD, kind], cwd=root, capture_output=True, text=True)
    if message is None:
        assert r.returncode == 0 and "returned" in r.stdout, r.stderr
    else:
        assert r.returncode == -6 and "returned" not in r.stdout, (r.returncode, r.stderr)
        assert "bound violated: " + message in r.stderr, r.stderr
