"""The lane-pair G2 group law on real gfx950 lanes (tests/devcheck,
devcheck_g2.hip: thin kernels around bls_pair.h / bls_sgb.h, compiled as
k_sgb.hip compiles them) with the directed operands of tests/edge_points.py,
against Python integers and the oracle.

The additions without a doubling branch, the complete ones, psi, [|x|] P, the
subgroup test, cofactor clearing and the batched subgroup test's fold and
running sums otherwise run only inside whole launches, on operands that never
meet their exceptional branches.  Their cross-lane exchanges sit inside
branches, so every list is laid out with neighbouring pairs of a wave taking
different branches (generic, `exc`, cancellation, infinity), run once more
rotated by one pair, and ends in a partly filled wave.  Every item is
normalised (X / Z^2, Y / Z^3, infinity as Z == 0) and compared exactly, the
`exc` flag included, on both lanes of its pair.

The same lists pass tests/hostcheck under TBG_BOUNDS_CHECK first
(test_devcheck_operands.py).  After a non-zero HIP status no further GPU work
is started by the devcheck modules."""
import pytest

from tests import edge_points as ep
from tests.devcheck import G2_OPS
from tests.test_gpu_devcheck import SENT, call, flat, sentinel, u32, untouched

pytestmark = pytest.mark.gpu

JAC_W = 84


def launch(op, cases, cap_extra=3):
    n, cap = len(cases), len(cases) + cap_extra
    aw = u32(flat(c[0] for c in cases))
    bw = u32(flat(c[1] for c in cases)) if cases[0][1] is not None else None
    out, flags = sentinel(cap * JAC_W), sentinel(cap * 2)
    call("dc_g2", G2_OPS.index(op), aw, bw, out, flags, n, cap)
    assert untouched(out, n * JAC_W) and untouched(flags, 2 * n), op
    for i, (_, _, expect) in enumerate(cases):
        f0, f1 = flags[2 * i], flags[2 * i + 1]
        assert f0 == f1, (op, i, "the lanes of a pair disagree", f0, f1)
        words = list(out[i * JAC_W:(i + 1) * JAC_W])
        if op == "in_subgroup_aff":
            assert all(w == SENT for w in words), (op, i, "out written")
        err = ep.check(op, words, f0, expect)
        assert err is None, (op, i, err)


def test_op_codes_match():
    assert G2_OPS == ep.OPS


@pytest.mark.parametrize("op", ["add_x", "add_aff_x", "add_in", "add_aff_in"])
def test_additions_with_interleaved_branches(op):
    cases = ep.cases()[op]
    assert len(cases) > 32 and len(cases) % 32 != 0  # more than one wave, the last partly filled
    launch(op, cases)
    launch(op, cases[1:] + cases[:1])  # every pair position sees the other branch


@pytest.mark.parametrize("op", ["dbl_lo", "psi"])
def test_doubling_and_psi(op):
    cases = ep.cases()[op]
    assert len(cases) > 32 and len(cases) % 32 != 0
    launch(op, cases)
    launch(op, cases[1:] + cases[:1])


@pytest.mark.parametrize("op", ["mul_xabs_x", "mul_xabs_aff_x", "in_subgroup_aff", "clear_cofactor"])
def test_x_chains_on_g2_torsion_and_non_subgroup_points(op):
    cases = ep.cases()[op]
    assert 8 <= len(cases) < 32  # a partly filled wave; G2, torsion and non-subgroup points side by side
    launch(op, cases)
    launch(op, cases[1:] + cases[:1])


@pytest.mark.parametrize("op", ["sgb_sums", "sgb_sums_complete", "sgb_fold", "sgb_fold_complete"])
def test_subgroup_batch_sums(op):
    cases = ep.cases()[op]
    if op.startswith("sgb_sums"):
        assert len(cases) >= 64 + 4 and len(cases) % 32 != 0  # every pattern of empty buckets among six, and more
    launch(op, cases)
    launch(op, cases[1:] + cases[:1])


def test_checker_sees_a_wrong_lane_word():
    """The comparison reaches every word a kernel wrote: one limb of one
    result off by one is rejected."""
    cases = ep.cases()["add_in"][:5]
    n = len(cases)
    aw, bw = u32(flat(c[0] for c in cases)), u32(flat(c[1] for c in cases))
    out, flags = sentinel(n * JAC_W), sentinel(n * 2)
    call("dc_g2", G2_OPS.index("add_in"), aw, bw, out, flags, n, n)
    i = next(k for k, c in enumerate(cases) if c[2][0] is not None)
    words = list(out[i * JAC_W:(i + 1) * JAC_W])
    assert ep.check("add_in", words, flags[2 * i], cases[i][2]) is None
    for j in (0, 13, 14, 41, 83):
        w = list(words)
        w[j] += 1
        assert ep.check("add_in", w, flags[2 * i], cases[i][2]) is not None
