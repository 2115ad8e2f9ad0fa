"""The fused level 0's S role (charon_amd/csrc/bls_l0tail.h) on the host.

In a fused launch the first workgroups of k_rlc_g1_l0's grid form
S = sum_j psi^j(2 A_j + T) from the batched subgroup test's sums: a block
sums one chunk of 128 points of a column, the last block to arrive at a
column's counter sums the column, the last column to arrive runs the Horner
steps.  tests/l0tail compiles that block function for the CPU (the 32 lane
pairs of a block in a loop, the hand-off counters plain words, value bounds
checked) and runs the blocks in an order the test chooses.

Every input point is a small multiple of the G2 generator, so S is checked
twice: against the same form with every column summed point by point (as
tests/l0fused forms it), and against oracle/bls12_381.py through the scalars
(psi acts on G2 as multiplication by x).
"""
import ctypes
import random

import numpy as np
import pytest

from oracle import bls12_381 as bls

FIRST = [0, 5, 10, 14, 18]
COLS = 19

# (n_sg, n_t): groups, slices of T per group
ONE_CHUNK = (2, 32)       # one chunk per column: 18 + 1 blocks
SHORT_LAST = (9, 32)      # T: 288 slices = 3 chunks, the last of 32 points
TWO_Q_CHUNKS = (130, 2)   # Q columns: 128 + 2 points; T: 260 slices = 3 chunks, the last of 4


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def hc():
    from tests.l0tail import lib
    h = lib()
    h.l0t_hc_blocks.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    h.l0t_hc_blocks.restype = ctypes.c_uint32
    h.l0t_hc_chunks.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    h.l0t_hc_chunks.restype = ctypes.c_uint32
    h.l0t_hc_run.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3 + \
        [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    h.l0t_hc_run.restype = ctypes.c_int
    return h


def expected_scalar(qk, tk):
    """S's multiple of the base point: sum_j x^j (2 sum_e 13^e Qbar_(first_j + e) + T)."""
    qbar = [int(v) for v in qk.astype(np.int64).sum(axis=0)]
    t = int(tk.astype(np.int64).sum())
    s = 0
    for j in range(4):
        a = sum(13 ** e * qbar[FIRST[j] + e] for e in range(FIRST[j + 1] - FIRST[j]))
        s += bls.X ** j * (2 * a + t)
    return s % bls.R


def orders(n):
    fwd = np.arange(n, dtype=np.uint32)
    sh = fwd.copy()
    np.random.default_rng(0x5EED).shuffle(sh)
    return {"forward": fwd, "reverse": fwd[::-1].copy(), "shuffled": sh}


def run_role(hc, shape, qk, tk, order):
    n_sg, n_t = shape
    qk = np.ascontiguousarray(qk, dtype=np.uint32)
    tk = np.ascontiguousarray(tk, dtype=np.uint32)
    assert qk.shape == (n_sg, 18) and tk.shape == (n_sg * n_t,)
    role, ref = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    stats, counters = np.zeros(4, dtype=np.uint32), np.zeros(COLS + 1, dtype=np.uint32)
    rc = hc.l0t_hc_run(bls.g2_compress(bls.G2_GEN), n_sg, n_t, vp(qk), vp(tk), vp(order), role, ref, vp(stats),
                       vp(counters))
    assert rc == 0
    return role.raw, ref.raw, stats, counters


def check(hc, shape, qk, tk):
    n_sg, n_t = shape
    blocks = hc.l0t_hc_blocks(n_sg, n_t)
    chunks = [hc.l0t_hc_chunks(n_sg, n_t, c) for c in range(COLS)]
    assert blocks == sum(chunks)
    k = expected_scalar(qk, tk)
    want = bls.g2_compress(bls.g2_mul(bls.G2_GEN, k)) if k else None
    for name, order in orders(blocks).items():
        role, ref, stats, counters = run_role(hc, shape, qk, tk, order)
        assert role == ref, name
        if want is not None:
            assert role == want and stats[1] == 0, name
        else:
            assert stats[1] == 1, name  # S = 0: the flag, no point
        # one block ran the Horner steps, and it was the last to run; every
        # column was summed once, behind an acquire each, as was the last step
        assert stats[0] == 1 and stats[3] == blocks - 1, (name, stats)
        assert stats[2] == COLS + 1, (name, stats)
        assert counters[:COLS].tolist() == chunks and counters[COLS] == COLS, (name, counters)
    return blocks, chunks


def random_inputs(shape, seed):
    n_sg, n_t = shape
    rng = np.random.default_rng(seed)
    return rng.integers(1, 1 << 16, size=(n_sg, 18), dtype=np.uint32), \
        rng.integers(1, 1 << 16, size=n_sg * n_t, dtype=np.uint32)


def test_one_chunk_per_column(hc):
    qk, tk = random_inputs(ONE_CHUNK, 1)
    blocks, chunks = check(hc, ONE_CHUNK, qk, tk)
    assert blocks == 19 and chunks == [1] * 19


def test_three_t_chunks_with_a_short_last_one(hc):
    qk, tk = random_inputs(SHORT_LAST, 2)
    blocks, chunks = check(hc, SHORT_LAST, qk, tk)
    assert blocks == 18 + 3 and chunks == [1] * 18 + [3]


def test_two_chunks_per_q_column(hc):
    qk, tk = random_inputs(TWO_Q_CHUNKS, 3)
    blocks, chunks = check(hc, TWO_Q_CHUNKS, qk, tk)
    assert blocks == 18 * 2 + 3 and chunks == [2] * 18 + [3]


@pytest.mark.parametrize("shape", [ONE_CHUNK, SHORT_LAST], ids=["one_chunk", "short_last"])
def test_equal_points_meet_the_doubling_case(hc, shape):
    """Equal points inside a pair's chain, equal pair sums in the tree (a whole
    column of one point), equal chunk sums in a column's fold, and points at
    infinity among them."""
    n_sg, n_t = shape
    qk, tk = random_inputs(shape, 4)
    tk[:] = 7                 # every slice of T the same point: every level of the tree doubles
    tk[5] = 0                 # ... but for an infinity in one pair's chain
    qk[:, 0] = 3              # a column of equal points
    qk[:, 1] = 0              # a column of infinities
    qk[:, 17] = qk[0, 17]     # the top coefficient of A_3 equal over the groups
    check(hc, shape, qk, tk)


def test_s_at_infinity_sets_the_flag(hc):
    n_sg, n_t = ONE_CHUNK
    qk = np.zeros((n_sg, 18), dtype=np.uint32)
    tk = np.zeros(n_sg * n_t, dtype=np.uint32)
    check(hc, ONE_CHUNK, qk, tk)
