"""The hash-to-G2 kernel chain on real gfx950 lanes, stage by stage
(tests/devcheck, devcheck_h2c.hip / devcheck_h2c_clear.hip: the product's own
k_hash.hip and k_hash_clear.hip, included and compiled as the product compiles
them) with the directed inputs of tests/edge_h2c.py, against Python integers
and the oracle.

H(m) otherwise runs only inside whole launches, from message bytes, and a
wrong point shows only as a failed verification.  Here the chain is entered
from messages of every block-boundary length, from injected (u0, u1), from
preloaded SSWU slots and from preloaded points, so the branches it takes on
exceptional values run with ordinary items on the neighbouring lanes
(edge_h2c's docstring lists the branches and what stays unreachable).  Every
result is compared exactly as an affine point; every word a stage should not
have written -- h_jac slots, h_aff, h_status, the words past item n -- must
still hold what was copied in.

The (u0, u1) and square-root lists pass tests/hostcheck under
TBG_BOUNDS_CHECK first (test_h2c_edges_host.py).  After a non-zero HIP status
no further GPU work is started by the devcheck modules."""
import ctypes
import random

import pytest

from oracle import bls12_381 as bls
from tests import devcheck
from tests import edge_h2c as eh
from tests.edge_points import add, psi
from tests.test_gpu_devcheck import _STATE, SENT, call, flat, sentinel, u32, untouched

pytestmark = pytest.mark.gpu

JAC_W, AFF_W, FP2_W = eh.JAC_W, eh.AFF_W, eh.FP2_W
S = {name: i for i, name in enumerate(eh.STAGES)}
SSENT = SENT - (1 << 32)


def run(first, last, n, msgs=None, u=None, preload=(), cap_extra=3):
    """One dc_h2c call.  preload: {h_jac slot: 84 words}; every other word of
    every buffer holds the sentinel.  Returns (h_jac words before, after,
    h_aff, h_status)."""
    cap = n + cap_extra
    hjac = sentinel((3 * n + cap_extra) * JAC_W)
    for slot, words in dict(preload).items():
        assert 0 <= slot < 3 * n and len(words) == JAC_W
        hjac[slot * JAC_W:(slot + 1) * JAC_W] = words
    before = list(hjac)
    haff, hst = sentinel(cap * AFF_W), sentinel(cap, signed=True)
    mb = moff = uw = None
    if msgs is not None:
        mb = b"".join(msgs)
        off = [0]
        for m in msgs:
            off.append(off[-1] + len(m))
        moff = u32(off)
    if u is not None:
        uw = u32(u)
    call("dc_h2c", S[first], S[last], n, mb, moff, uw, hjac, haff, hst, cap)
    assert untouched(hjac, 3 * n * JAC_W), "h_jac past the 3 n slots"
    assert untouched(haff, n * AFF_W) and untouched(hst, n), "h_aff / h_status past item n"
    return before, list(hjac), list(haff), list(hst)


def slot(words, k):
    return words[k * JAC_W:(k + 1) * JAC_W]


def check_slots(tag, before, after, n, expect):
    """expect: {slot: point}; every slot not named there must hold exactly
    the words copied in."""
    for k in range(3 * n):
        if k in expect:
            err = eh.check_jac(slot(after, k), expect[k])
            assert err is None, (tag, "slot", k, err)
        else:
            assert slot(after, k) == slot(before, k), (tag, "slot", k, "written")


def check_affine_out(tag, haff, hst, n, points):
    """points: the n expected H, or None: k_hash_affine did not run."""
    if points is None:
        assert all(w == SENT for w in haff[:n * AFF_W]) and all(s == SSENT for s in hst[:n]), (tag, "h_aff written")
        return
    for i, h in enumerate(points):
        err = eh.check_affine(haff[i * AFF_W:(i + 1) * AFF_W], hst[i], h)
        assert err is None, (tag, "h_aff", i, err)


def chain_expect(n, q_pairs, last):
    """Slots and affine output after the chain ran from the mapped points
    (Q0, Q1 per message) up to `last`."""
    expect, points = {}, None
    for i, (q0, q1) in enumerate(q_pairs):
        if last == "SSWU":
            expect[i], expect[n + i] = q0, q1
            continue
        p = add(q0, q1)
        t1, v, h = eh.clear_steps(p)
        if last == "CLEAR_X1":
            expect[i], expect[n + i], expect[2 * n + i] = p, t1, add(t1, psi(p))
        else:
            expect[i], expect[n + i], expect[2 * n + i] = h, t1, v
    if last == "AFFINE":
        points = [expect[i] for i in range(n)]
    return expect, points


def rotations(items):
    """The list, and the list rotated by one: every lane (pair) position
    sees the other kind of item."""
    return [items, items[1:] + items[:1]]


def test_stage_codes_and_workgroup_size():
    assert devcheck.H2C_STAGES == eh.STAGES
    blk = devcheck.lib().dc_h2c_binv_block()
    for n in (len(eh.u_pairs()), max(eh.MSG_BATCHES)):
        assert n > blk and n % blk != 0  # more than one workgroup of the batched inversions, the last partly filled
    assert {blk - 1, blk, blk + 1} <= set(eh.MSG_BATCHES)


@pytest.mark.parametrize("n", eh.MSG_BATCHES)
def test_messages_through_the_whole_chain(n):
    """MAP_MSG .. AFFINE is launch_hash_msgs itself: messages of every
    block-boundary length, batches around the batched inversion's workgroup."""
    msgs = eh.messages()[:n]
    before, after, haff, hst = run("MAP_MSG", "AFFINE", n, msgs=msgs)
    q_pairs = []
    for m in msgs:
        u0, u1 = bls.hash_to_field_fp2(m, bls.DST_POP, 2)
        q_pairs.append((eh.map_point(u0), eh.map_point(u1)))
    expect, points = chain_expect(n, q_pairs, "AFFINE")
    assert points == [eh.hash_point(m) for m in msgs]
    check_slots(n, before, after, n, expect)
    check_affine_out(n, haff, hst, n, points)


@pytest.mark.parametrize("last", ["SSWU", "AFFINE"])
def test_injected_field_elements(last):
    """MAP_U: zero denominators (no batched inverse: both maps of the message
    take the reference map, the workgroup's other lanes undisturbed), u in Fp,
    purely imaginary, +-1, Q0 == Q1 and Q1 == -Q0."""
    for pairs in rotations(eh.u_pairs()):
        n = len(pairs)
        before, after, haff, hst = run("MAP_U", last, n, u=eh.u_words(pairs))
        expect, points = chain_expect(n, [(eh.map_point(u0), eh.map_point(u1)) for _, u0, u1 in pairs], last)
        if last == "AFFINE":
            for (kind, _, _), h in zip(pairs, points):
                assert (h is None) == (kind == "opposite")
        check_slots(last, before, after, n, expect)
        check_affine_out(last, haff, hst, n, points)


def test_sswu_from_preloaded_slots():
    """k_hash_sswu alone: slots without an inverse, slots whose g(x1) the
    closed-form root refuses (u must still be intact for the reference map),
    ordinary slots in between."""
    for slots in rotations(eh.sswu_slots()):
        n = len(slots) // 2
        before, after, haff, hst = run("SSWU", "SSWU", n,
                                       preload={k: eh.sswu_slot_words(s) for k, s in enumerate(slots)})
        check_slots("sswu", before, after, n, {k: eh.map_point(s[1]) for k, s in enumerate(slots)})
        check_affine_out("sswu", haff, hst, n, None)


def test_square_root_or_z():
    """fp2_sqrt_or_z_in with its input waiting in a memory slot: both
    refusals, both arms of the final select, squares and non-squares."""
    for vals in rotations(eh.sqrt_values()):
        n, cap = len(vals), len(vals) + 3
        root, flags = sentinel(cap * FP2_W), sentinel(cap)
        call("dc_h2c_sqrt", u32(flat(eh.fp2_words(a) for _, a in vals)), root, flags, n, cap)
        assert untouched(root, n * FP2_W) and untouched(flags, n)
        for i, (kind, a) in enumerate(vals):
            err = eh.check_sqrt(a, flags[i], list(root[i * FP2_W:(i + 1) * FP2_W]))
            assert err is None, (i, kind, err)


@pytest.mark.parametrize("last", ["CLEAR_X1", "AFFINE"])
def test_clearing_from_injected_points(last):
    """CLEAR_X1 on: Q0 == Q1 and sums in G2 (the two calls of
    px_add_complete_at), cancellation, infinities, torsion and non-subgroup
    points, each beside a generic pair."""
    rng = random.Random(0xC1EA2)
    for pairs in rotations(eh.clear_pairs()):
        n = len(pairs)
        preload = {}
        for i, (_, q0, q1) in enumerate(pairs):
            preload[i], preload[n + i] = eh.point_words(rng, q0), eh.point_words(rng, q1)
        before, after, haff, hst = run("CLEAR_X1", last, n, preload=preload)
        expect, points = chain_expect(n, [(q0, q1) for _, q0, q1 in pairs], last)
        check_slots(last, before, after, n, expect)
        check_affine_out(last, haff, hst, n, points)


def test_last_clearing_kernel_from_injected_points():
    """k_hash_clear_fin alone: each of its four additions meets its doubling
    case in some item (clear_fin_complete), generic triples in between."""
    rng = random.Random(0xF1A)
    for triples in rotations(eh.fin_triples()):
        n = len(triples)
        preload = {}
        for i, (_, p, t1, v) in enumerate(triples):
            preload[i], preload[n + i], preload[2 * n + i] = (eh.point_words(rng, q) for q in (p, t1, v))
        before, after, haff, hst = run("CLEAR_FIN", "CLEAR_FIN", n, preload=preload)
        check_slots("fin", before, after, n, {i: eh.fin_value(p, t1, v) for i, (_, p, t1, v) in enumerate(triples)})
        check_affine_out("fin", haff, hst, n, None)


def test_checker_sees_a_wrong_word():
    """The comparison reaches every word the chain wrote: one limb of one
    result off by one, a written slot that should have been left alone and a
    wrong status are all rejected."""
    pairs = eh.clear_pairs()[:5]
    n = len(pairs)
    rng = random.Random(5)
    preload = {}
    for i, (_, q0, q1) in enumerate(pairs):
        preload[i], preload[n + i] = eh.point_words(rng, q0), eh.point_words(rng, q1)
    before, after, haff, hst = run("CLEAR_X1", "AFFINE", n, preload=preload, cap_extra=0)
    expect, points = chain_expect(n, [(q0, q1) for _, q0, q1 in pairs], "AFFINE")
    check_slots("ok", before, after, n, expect)
    check_affine_out("ok", haff, hst, n, points)
    i = next(k for k, h in enumerate(points) if h is not None)
    for k in (i, n + i, 2 * n + i):
        for j in (0, 13, 14, 41, 83):
            bad = list(after)
            bad[k * JAC_W + j] += 1
            with pytest.raises(AssertionError):
                check_slots("bad", before, bad, n, expect)
    for j in (0, 13, 14, 55):
        bad = list(haff)
        bad[i * AFF_W + j] += 1
        with pytest.raises(AssertionError):
            check_affine_out("bad", bad, hst, n, points)
    bad = list(hst)
    bad[i] = 1
    with pytest.raises(AssertionError):
        check_affine_out("bad", haff, bad, n, points)
    # one limb of one EXPECTED value flipped
    x, y = points[i]
    with pytest.raises(AssertionError):
        check_affine_out("bad", haff, hst, n, points[:i] + [((x[0] ^ 1, x[1]), y)] + points[i + 1:])
    # a slot the stage must not write
    del expect[2 * n + i]
    with pytest.raises(AssertionError):
        check_slots("bad", before, after, n, expect)


def test_both_libraries_run_their_own_kernels_in_one_process():
    """libdevcheck.so holds a second copy of the hash and decode kernels and
    of launch_hash_msgs / launch_decode_sigs under the product's names: with the engine library
    loaded and used before and after, each still runs its own code."""
    import __graft_entry__ as entry
    if _STATE["rc"]:
        pytest.fail(f"an earlier devcheck entry returned HIP status {_STATE['rc']}: no further GPU work here")
    entry.smoke()
    msgs = eh.messages()[:2]
    before, after, haff, hst = run("MAP_MSG", "AFFINE", 2, msgs=msgs)
    check_affine_out("both", haff, hst, 2, [eh.hash_point(m) for m in msgs])
    # ... and of the decode kernels and their launchers (devcheck_decode.hip)
    from tests import edge_decode as ed
    from tests.test_gpu_devcheck_decode import check_keys, check_sigs, run_keys, run_sigs
    keys = ed.g1_entries()[:3]
    check_keys("both", *run_keys(keys), keys)
    sigs = ed.g2_entries()[:5]
    aff, st, _, _ = run_sigs("DECODE", "SUBGROUP", len(sigs), sigs=[e.data for e in sigs])
    check_sigs("both", aff, st, sigs, True)
    entry.smoke()
