"""The hexad's direct line product on the GPU (charon_amd/csrc/bls_hex.h
hex_line_mul: each output component one reduced sum of six products).

Unit level: tests/devcheck/devcheck_hexline.hip runs hex_line_at_v and
hex_line_folded on real lanes, one hexad per slot, on the host test's
directed operands (tests/hexline/operands.py; distinct values per hexad):
  n = 10  one full wave, lane 15 of each row idle
  n = 13  a partial second wave
  n = 1
Output slots past n must keep the caller's sentinel; results are compared as
canonical values with the oracle's tower.

End to end, against oracle/c as the level-0 tests do, each at the smallest
batch that reaches the path (level 0 forced on, one slot, (G, C) = (16, 8)
unless stated); each test names the kernels whose line steps it reaches.
Verdicts and aggregates must match the oracle bit for bit.
"""
import copy
import ctypes

import numpy as np
import pytest

from tests import edge_operands as eo

pytestmark = pytest.mark.gpu

P = eo.P
NL = eo.NL
SENT = eo.SENTINEL
T, N = 3, 4
_STATE = {"rc": 0}


# ---------------------------------------------------------------------------
# the line steps on real lanes
@pytest.fixture(scope="module")
def directed():
    from tests.hexline import operands as ops
    cs = ops.cases()
    at = [c for c in cs if c["pt"] is not None]
    folded = [c for c in cs if c["pt"] is None]
    return {"at": at, "folded": folded, "want": {id(c): ops.expect(c) for c in cs}}


def u32(words):
    return (ctypes.c_uint32 * len(words))(*[int(w) for w in words])


def launch(folded, cases):
    from tests import devcheck_hexline
    from tests.hexline import operands as ops
    if _STATE["rc"]:
        pytest.fail(f"an earlier launch returned HIP status {_STATE['rc']}: no further GPU work here")
    n, cap = len(cases), len(cases) + 3
    out = (ctypes.c_uint32 * (cap * 168))(*([SENT] * (cap * 168)))
    f = u32([w for c in cases for w in ops.words(c["f"])])
    lines = u32([w for c in cases for w in ops.words(c["line"])])
    pts = None if folded else u32([w for c in cases for w in ops.words(c["pt"])])
    rc = devcheck_hexline.lib().dcx_hex_line(1 if folded else 0, f, lines, pts, out, n, cap)
    if rc:
        _STATE["rc"] = rc
    assert rc == 0, f"dcx_hex_line returned {rc}"
    assert all(w == SENT for w in out[n * 168:]), "wrote past the last slot"
    return [list(out[s * 168:(s + 1) * 168]) for s in range(n)]


@pytest.mark.parametrize("kind", ["at", "folded"])
@pytest.mark.parametrize("n", [10, 13, 1])
def test_line_steps_on_lanes(directed, kind, n):
    """Every directed case once per shape and source, n hexads at a time (the
    last launch of a shape wraps round to the first cases, so every launch
    has exactly n slots)."""
    cases = directed[kind]
    per_shape = {10: range(0, len(cases), 10), 13: range(0, len(cases), 13), 1: range(0, len(cases), 29)}[n]
    for start in per_shape:
        batch = [cases[(start + i) % len(cases)] for i in range(n)]
        got = launch(kind == "folded", batch)
        for s, c in enumerate(batch):
            words = got[s]
            assert max(words) <= eo.M28, (c["name"], "limbs not below 2^28")
            ls = [words[i:i + NL] for i in range(0, 168, NL)]
            assert all(eo.val(l) < 2 * P for l in ls), (c["name"], "not below 2p")
            assert eo.check_f12([eo.unmont(l) for l in ls], directed["want"][id(c)]) is None, (kind, n, s, c["name"])


# ---------------------------------------------------------------------------
# end to end
N_SHARED, N_PER = 48, 43  # 48 duties of 43 partials = 2,064 partials: the smallest fused launch has 2,048


@pytest.fixture(scope="module")
def ctx():
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_shared_batch
    base = dict(slots=1, rlc_batch=eng.RLC_L0_ON)
    es = dict(classic=eng.Engine(0, rlc_group=16, rlc_chunk=8, **base),
              fused=eng.Engine(0, subgroup_batch=eng.SGB_ON, l0_msg_share=eng.L0_MSG_ALWAYS, **base),
              long=eng.Engine(0, rlc_group=40, rlc_chunk=20, **base))
    shared = make_shared_batch(es["fused"], N_SHARED, T, N_PER, (np.arange(N_SHARED) % 3).astype(np.uint32), seed=1706)
    assert len(shared.sigs) == 2064
    yield dict(es=es, shared=shared, shared_ref=oracle_run(shared))
    for e in es.values():
        e.close()


def run(e, b):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs, b.identifiers, msgs=(b.msg_data, b.msg_off),
                 duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids, duty_threshold=b.threshold)
    return e.collect(t), t


def check(e, b, want_level0, ref=None):
    """Per-partial verdicts, per-duty verdicts and every aggregate bit for bit
    with oracle/c; level 0's outcome as named."""
    from tests.test_gpu_fullsize import assert_same, oracle_run
    res, t = run(e, b)
    assert_same(res, oracle_run(b) if ref is None else ref)
    assert e.level0(t) == want_level0
    return res, t


def variant(b, **kw):
    v = copy.copy(b)
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def test_one_duty(ctx):
    """k_miller_hex<MILLER_L0>: one chunk with one live line per step, and the
    S hexad beside it."""
    from charon_amd import engine as eng
    from tools.workload import make_batch
    e = ctx["es"]["classic"]
    b = make_batch(e, 1, T, N, seed=1701)
    res, _ = check(e, b, eng.L0_PASSED)
    assert (res.duty_status == 0).all() and np.array_equal(res.agg, b.group_sig)


def test_nine_duties_second_chunk_of_one(ctx):
    from charon_amd import engine as eng
    from tools.workload import make_batch
    e = ctx["es"]["classic"]
    b = make_batch(e, 9, T, N, seed=1702)
    res, t = check(e, b, eng.L0_PASSED)
    s = e.shape(t)
    assert (s["group"], s["chunk"], s["chunks"]) == (16, 8, 2), s
    assert (res.duty_status == 0).all() and np.array_equal(res.agg, b.group_sig)


def test_one_invalid_partial_runs_the_group_and_fallback_checks(ctx):
    """Level 0 fails: the groups' S hexads (k_miller_hex<MILLER_GROUP_S> after
    a classic level 0, whose P chunks serve as they are) and the hexad
    fallback checks of the failing group (k_rlc.hip) find the partial."""
    from charon_amd import engine as eng
    from tools.workload import make_batch
    e = ctx["es"]["classic"]
    b = make_batch(e, 20, T, N, seed=1703)
    bad = 4 * 17 + 1
    sigs = np.array(b.sigs, copy=True)
    sigs[bad] = b.sigs[4 * 3 + 1]  # a valid point, another duty's partial
    res, t = check(e, variant(b, sigs=sigs), eng.L0_FAILED)
    assert res.partial_status[bad] != eng.PS_VALID
    assert (np.delete(res.partial_status, bad) == eng.PS_VALID).all()
    assert (res.duty_status == 0).all()  # three valid partials are left in duty 17


def test_a_duty_that_is_not_combined_is_skipped_in_the_hoisted_list(ctx):
    """Two of a duty's four partials do not decode: below the threshold, the
    duty is not combined and its bit stays out of its chunk's run list, while
    the chunk's other duties run."""
    from charon_amd import engine as eng
    from tools.workload import make_batch
    e = ctx["es"]["classic"]
    b = make_batch(e, 9, T, N, seed=1705)
    sigs = np.array(b.sigs, copy=True)
    sigs[4 * 2] = 0xFF       # not an encoding of a point
    sigs[4 * 2 + 3] = 0xFF
    res, _ = check(e, variant(b, sigs=sigs), eng.L0_PASSED)
    assert res.duty_status[2] != 0 and (np.delete(res.duty_status, 2) == 0).all()


def test_shared_messages_pair_one_key_sum_per_message(ctx):
    """48 duties on 3 messages in a fused launch: k_l0m_miller."""
    from charon_amd import engine as eng
    e, b = ctx["es"]["fused"], ctx["shared"]
    res, t = check(e, b, eng.L0_PASSED, ref=ctx["shared_ref"])
    assert e.level0_msgs(t)["merged"] is True
    assert "k_l0m_miller" in {name for name, _ in e.replay_profile(t)}
    assert (res.duty_status == 0).all() and np.array_equal(res.agg, b.group_sig)


def test_groups_after_a_fused_level0_failure(ctx):
    """A failed FUSED level 0 keeps nothing: k_miller_hex<MILLER_GROUPS> forms
    the P chunks again with the groups' S hexads, and the fallback checks
    find the partial."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    e, b = ctx["es"]["fused"], ctx["shared"]
    duty, bad = 5, N_PER * 5 + 2
    sigs = np.array(b.sigs, copy=True)
    sigs[bad] = b.sigs[N_PER * 9 + 2]
    v = variant(b, sigs=sigs)
    ps, ds, agg = (np.array(x, copy=True) for x in ctx["shared_ref"])
    p, d, a = oracle_run(v, duty, duty + 1)  # every other duty's inputs are the clean ones
    ps[N_PER * duty:N_PER * (duty + 1)] = p
    ds[duty] = d[0]
    agg[duty] = a[0]
    res, _ = check(e, v, eng.L0_FAILED, ref=(ps, ds, agg))
    assert res.partial_status[bad] != eng.PS_VALID


def test_chunks_longer_than_the_hoisted_list(ctx):
    """rlc_chunk = 20 > HEX_HOIST_MAX = 16 (the engine accepts it): the
    un-hoisted loop of k_miller_hex decides every duty at every step."""
    from charon_amd import engine as eng
    from tools.workload import make_batch
    e = ctx["es"]["long"]
    b = make_batch(e, 23, T, N, seed=1707)
    res, t = check(e, b, eng.L0_PASSED)
    s = e.shape(t)
    assert (s["group"], s["chunk"], s["chunks"]) == (40, 20, 2), s
    assert (res.duty_status == 0).all() and np.array_equal(res.agg, b.group_sig)
