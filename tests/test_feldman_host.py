"""The Feldman commitment evaluation (charon_amd/csrc/bls_feldman.h) on the CPU,
through the host twin tests/feldman with TBG_BOUNDS_CHECK on (a violated value
bound aborts the process).

1. Every directed polynomial and identifier of tests/edge_feldman.py, in the
   layout the GPU test launches: outputs and both status arrays equal the
   integers' [f(id) mod r] G1 exactly.
2. 200 random polynomials with t in 1..8 at identifiers 1..10, exactly.
3. A commitment that does not decode fails every evaluation of its polynomial
   (TBG_FV_COMMIT, zero bytes) and no other polynomial's.
4. fv_mul_u32 alone on the directed identifiers.
"""
import numpy as np

from tests import edge_feldman as ef
from tests.feldman import lib


def run(commit48, poly_first, eval_poly, eval_id):
    c = np.frombuffer(commit48, dtype=np.uint8).copy()
    pf = np.ascontiguousarray(poly_first, dtype=np.uint32)
    ep = np.ascontiguousarray(eval_poly, dtype=np.uint32)
    ei = np.ascontiguousarray(eval_id, dtype=np.uint32)
    out = np.full((len(ep), 48), 0xAA, dtype=np.uint8)
    st = np.full(len(ep), 99, dtype=np.int32)
    cst = np.full(len(c) // 48, 99, dtype=np.int32)
    rc = lib().fvh_eval(c.ctypes.data, pf.ctypes.data, len(pf) - 1, ep.ctypes.data, ei.ctypes.data, len(ep), out.ctypes.data,
                        st.ctypes.data, cst.ctypes.data)
    assert rc == 0
    return [bytes(o) for o in out], st.tolist(), cst.tolist()


def test_directed_cases_equal_the_integers():
    L = ef.launch()
    out, st, cst = run(L.commit48, L.poly_first, L.eval_poly, L.eval_id)
    for k, (p, i) in enumerate(zip(L.eval_poly, L.eval_id)):
        assert st[k] == L.want_status[k], (L.case_of_poly[p], i, st[k])
        assert out[k] == L.want_out[k], (L.case_of_poly[p], i)
    want_c = [1 if L.commit48[48 * j:48 * j + 48] == ef.IDENT48 else 0 for j in range(len(L.commit48) // 48)]
    assert cst == want_c and sum(want_c) == 3


def test_random_polynomials_equal_the_integers():
    polys = ef.random_polys(200, list(range(1, 9)), seed=0xFE1D2)
    assert {len(p) for p in polys} == set(range(1, 9))
    first = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
    ev = [(p, i) for p in range(len(polys)) for i in range(1, 11)]
    out, st, cst = run(b"".join(b for p in polys for b in ef.commits(p)), first, [p for p, _ in ev], [i for _, i in ev])
    assert cst == [0] * int(first[-1])
    for k, (p, i) in enumerate(ev):
        assert (st[k], out[k]) == ef.expected(polys[p], i), (p, i)


def test_bad_commitment_fails_its_polynomial_only():
    good = ef.BY_NAME["generic_t3"].coeffs
    bad = bytes(48)  # the compression flag is missing: DEC_ERR_FLAGS
    cs = ef.commits(good)
    blob = b"".join(cs + [bad] + cs[1:] + cs[:1] + [bad] + cs[2:] + cs)
    out, st, cst = run(blob, [0, 3, 6, 9, 12], [0, 1, 2, 3, 1, 2, 1], [2, 2, 2, 2, 0, 5, 1])
    ok = ef.expected(good, 2)
    assert (st[0], out[0]) == ok and (st[3], out[3]) == ok
    assert st[1] == st[2] == st[5] == st[6] == ef.FV_COMMIT and out[1] == out[2] == out[5] == ef.ZERO48
    assert st[4] == ef.FV_ID  # the identifier's check comes first
    assert cst == [0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 0]


def test_small_multiples():
    h = lib()
    base = ef.BY_NAME["t1"].coeffs[0]
    for k in [i for i in ef.IDS if i] + [5, 7, 0x55555555, 0xAAAAAAAA]:
        out = np.zeros(48, dtype=np.uint8)
        assert h.fvh_mul(ef.commit(base), k, out.ctypes.data) == 0
        assert bytes(out) == ef.commit(base * k), k
        assert h.fvh_mul(ef.IDENT48, k, out.ctypes.data) == 0 and bytes(out) == ef.IDENT48
