"""px_h_lines (charon_amd/csrc/bls_pair.h: the body of k_lines_h, projective
Miller steps on lane pairs) on real gfx950 lanes, one lane pair per point
(tests/devcheck_hlines), against the host twin of the same steps
(tests/hlines, itself checked against the pinned line forms and the oracle by
tests/test_hlines_host.py).

70 points: two full waves of 32 pairs and a third with 6, so a partly filled
wave and the `pr >= n` guard both run.  Every output word is compared modulo
p, the limbs must be normalised, and everything past the 70th point's last
line -- two more rows and canary words -- must come back as it went in."""
import ctypes
import random

import pytest

from oracle import bls12_381 as bls
from tests import edge_operands as eo
from tests import hlines

pytestmark = pytest.mark.gpu

N_POINTS = 70
ROWS = 72      # rows 70 and 71 stay unwritten
CANARY = 64    # words after the last row
W = hlines.LINES_WORDS


def points():
    """70 distinct points of G2: runs of consecutive multiples of seeded random ones."""
    rng = random.Random(0x70C5)
    out = []
    for _ in range(7):
        base = bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))
        p = base
        for _ in range(10):
            out.append(p)
            p = bls.g2_add(p, base)
    assert len(set(out)) == N_POINTS
    return out


def host_words(q):
    out = (ctypes.c_uint32 * W)()
    hlines.lib().hl_words(hlines.aff192(q), out)
    return list(out)


def test_lines_of_70_points_match_the_host_twin():
    from tests import devcheck_hlines
    pts = points()
    q = (ctypes.c_uint32 * (N_POINTS * 4 * eo.NL))(*[w for p in pts for w in eo.g2_raw(p)])
    total = ROWS * W + CANARY
    out = (ctypes.c_uint32 * total)(*([eo.SENTINEL] * total))
    rc = devcheck_hlines.lib().dch_lines(q, out, N_POINTS, total)
    assert rc == 0, f"dch_lines returned HIP status {rc}"
    assert all(x == eo.SENTINEL for x in out[N_POINTS * W:]), "words past the last point's lines were written"
    for i, p in enumerate(pts):
        got = list(out[i * W:(i + 1) * W])
        assert eo.SENTINEL not in got, (i, "a word of the table was not written")
        err = eo.check_lines(got, host_words(p))
        assert err is None, (i, err)
