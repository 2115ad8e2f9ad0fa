"""The fused level 0 on the GPU against oracle/c.

While the batched subgroup test runs, level 0 takes S from that test's sums
(bls_rlc.h top; k_sgb.hip, k_msm.hip k_l0f_*) instead of a bucket MSM over
the signatures.  Settings: 3-of-4, subgroup_batch = SGB_ON, level 0 forced
on, 600 DVs = 2,400 partials -- two full subgroup groups and a short one of
352, the smallest shape with the batched test on.  Every result (per-partial
status, per-duty status, every aggregate) is compared with oracle/c's
restatement of the per-item schedule (tbls/tss.go:153-197,
tblsconv/tblsconv.go:125-132) through the helpers of test_gpu_fullsize.py.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_DV, T, N = 600, 3, 4
FUSED_KERNELS = {"k_l0f_reduce", "k_l0f_fold", "k_l0f_horner"}
MSM_KERNELS = {"k_msm_scan", "k_msm_scatter", "k_msm_bucket_part", "k_msm_bucket", "k_msm_tree", "k_msm_tree_final"}


@pytest.fixture(scope="module")
def ctx():
    """The two contexts (batched test on / off, level 0 on in both), the clean
    batch with its keys resident under the same ids in both, and its oracle
    results."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_batch
    on = eng.Engine(0, slots=1, subgroup_batch=eng.SGB_ON, rlc_batch=eng.RLC_L0_ON)
    off = eng.Engine(0, slots=1, subgroup_batch=eng.SGB_OFF, rlc_batch=eng.RLC_L0_ON)
    b = make_batch(on, N_DV, T, N, seed=7070)
    first, st = off.load_pubkeys(b.pubshares)
    assert first == b.pk_first and (st == 0).all()
    assert len(b.sigs) == 2400
    yield dict(on=on, off=off, b=b, ref=oracle_run(b))
    on.close()
    off.close()


def run(e, b, sigs=None, pubkey_ids=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg,
                 pubkey_ids=b.pubkey_ids if pubkey_ids is None else pubkey_ids, duty_threshold=b.threshold)
    return e.collect(t), t


def variant(b, sigs=None, pubkey_ids=None):
    """The batch with some inputs replaced (for oracle_run)."""
    import copy
    v = copy.copy(b)
    if sigs is not None:
        v.sigs = sigs
    if pubkey_ids is not None:
        v.pubkey_ids = pubkey_ids
    return v


def kernels(e, t):
    return {name for name, _ in e.replay_profile(t)}


def test_clean_batch_passes_on_the_fused_path(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    e, b = ctx["on"], ctx["b"]
    res, t = run(e, b)
    assert_same(res, ctx["ref"])
    assert e.level0(t) == eng.L0_PASSED
    assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == 0).all()
    assert np.array_equal(res.agg, b.group_sig)
    assert e.subgroup(t) == {"groups": 3, "failed": 0, "group_size": 1024}
    ks = kernels(e, t)
    assert FUSED_KERNELS <= ks and not (MSM_KERNELS & ks), sorted(ks)
    # the profiled replay left the same outputs
    again = e.fetch(t, N_DV, len(b.sigs))
    assert np.array_equal(again.partial_status, res.partial_status) and np.array_equal(again.agg, res.agg)
    assert e.level0(t) == eng.L0_PASSED


def test_same_batch_without_the_batched_test_runs_the_bucket_msm(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    b = ctx["b"]
    res_on, _ = run(ctx["on"], b)
    res, t = run(ctx["off"], b)
    assert_same(res, ctx["ref"])
    assert ctx["off"].level0(t) == eng.L0_PASSED
    ks = kernels(ctx["off"], t)
    assert MSM_KERNELS <= ks and not (FUSED_KERNELS & ks), sorted(ks)
    assert np.array_equal(res.partial_status, res_on.partial_status)
    assert np.array_equal(res.duty_status, res_on.duty_status) and np.array_equal(res.agg, res_on.agg)


@pytest.mark.parametrize("pos", [0, 2399], ids=["first", "last_of_short_group"])
def test_one_wrong_share_partial_fails_level0(ctx, pos):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e, b = ctx["on"], ctx["b"]
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = b.sigs[pos + 1 if pos % N == 0 else pos - 1]  # another share of its DV signed it
    res, t = run(e, b, sigs=sigs)
    assert e.level0(t) == eng.L0_FAILED
    assert_same(res, oracle_run(variant(b, sigs=sigs)))
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert res.partial_status[pos] == eng.PS_INVALID
    assert FUSED_KERNELS <= kernels(e, t)


def test_one_torsion_point_voids_level0(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e, b = ctx["on"], ctx["b"]
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        t13 = bytes.fromhex(json.load(f)["points"]["t13"][0])
    pos = 1024 + 77
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = np.frombuffer(t13, dtype=np.uint8)
    res, t = run(e, b, sigs=sigs)
    assert e.subgroup(t) == {"groups": 3, "failed": 1, "group_size": 1024}
    assert e.level0(t) == eng.L0_FAILED
    assert_same(res, oracle_run(variant(b, sigs=sigs)))
    assert res.partial_status[pos] == eng.PS_ERR_SUBGROUP
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]


def test_one_unknown_pubkey_id_voids_level0(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    from tools.workload import NO_PUBKEY
    e, b = ctx["on"], ctx["b"]
    pos = 2048 + 5
    ids = np.array(b.pubkey_ids, copy=True)
    ids[pos] = NO_PUBKEY
    res, t = run(e, b, pubkey_ids=ids)
    assert e.level0(t) == eng.L0_FAILED
    assert_same(res, oracle_run(variant(b, pubkey_ids=ids)))
    assert res.partial_status[pos] == eng.PS_ERR_PUBKEY
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]


@pytest.mark.parametrize("pa,pb", [(10, 501), (10, 1501)], ids=["one_group", "two_groups"])
def test_cancelling_errors_are_both_rejected(ctx, pa, pb):
    """s_a + delta and s_b - delta: the plain sum T cancels them, so only the
    weighted part of S separates the batch from a valid one."""
    from charon_amd import engine as eng
    from oracle import bls12_381 as bls
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e, b = ctx["on"], ctx["b"]
    delta = bls.g2_mul(bls.G2_GEN, 0x1234567)
    sigs = np.array(b.sigs, copy=True)
    sa, sb = bls.g2_decompress(bytes(b.sigs[pa])), bls.g2_decompress(bytes(b.sigs[pb]))
    sigs[pa] = np.frombuffer(bls.g2_compress(bls.g2_add(sa, delta)), dtype=np.uint8)
    sigs[pb] = np.frombuffer(bls.g2_compress(bls.g2_add(sb, bls.g2_neg(delta))), dtype=np.uint8)
    res, t = run(e, b, sigs=sigs)
    assert e.level0(t) == eng.L0_FAILED
    assert_same(res, oracle_run(variant(b, sigs=sigs)))
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pa, pb]
    assert (res.partial_status[[pa, pb]] == eng.PS_INVALID).all()


def test_packed_batches_and_prefix_replay(ctx):
    """Three caller batches of 300 DVs in one device batch (3,600 partials:
    the subgroup groups straddle the callers), then a replayed prefix of two."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    from tools.workload import make_batch
    e = ctx["on"]
    parts = [make_batch(e, 300, T, N, seed=7171 + k) for k in range(3)]
    refs = [oracle_run(p) for p in parts]
    args = [dict(duty_first=p.duty_first, sigs=p.sigs, identifiers=p.identifiers, msgs=(p.msg_data, p.msg_off),
                 duty_msg=p.duty_msg, pubkey_ids=p.pubkey_ids, duty_threshold=p.threshold) for p in parts]
    tickets = e.submit_group(eng.OP_VERIFY_AGGREGATE, args)
    for p, ref, t in zip(parts, refs, tickets):
        res = e.collect(t)
        assert_same(res, ref)
        assert np.array_equal(res.agg, p.group_sig)
    assert e.level0(tickets[0]) == eng.L0_PASSED
    assert e.subgroup(tickets[0]) == {"groups": 4, "failed": 0, "group_size": 1024}
    assert FUSED_KERNELS <= kernels(e, tickets[0])
    e.replay_plan([tickets[0]], [2])  # 2,400 partials of the resident batch
    e.synchronize()
    assert e.level0(tickets[0]) == eng.L0_PASSED
    for p, ref, t in zip(parts[:2], refs[:2], tickets[:2]):
        assert_same(e.fetch(t, p.n_dv, len(p.sigs)), ref)


def test_smaller_groups_after_non_subgroup_history():
    """A context that has just collected 8 non-subgroup partials in 6,000 runs
    subgroup groups below 1,024; a clean batch passes level 0 on the fused path."""
    from charon_amd import engine as eng
    from tests.test_gpu_sgb import crafted_batch
    from tools.workload import make_batch
    e = eng.Engine(0, slots=1, subgroup_batch=eng.SGB_AUTO, rlc_batch=eng.RLC_L0_ON)
    try:
        b, bad = crafted_batch(e)
        res, _ = run(e, b)
        assert np.flatnonzero(res.partial_status == eng.PS_ERR_SUBGROUP).tolist() == bad
        clean = make_batch(e, N_DV, T, N, seed=7272)
        res, t = run(e, clean)
        sg = e.subgroup(t)
        assert 64 <= sg["group_size"] < 1024 and sg["failed"] == 0 and sg["groups"] == -(-2400 // sg["group_size"]), sg
        assert e.level0(t) == eng.L0_PASSED
        assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, clean.group_sig)
        ks = kernels(e, t)
        assert FUSED_KERNELS <= ks and "k_msm_bucket_part" not in ks
    finally:
        e.close()


# ---- the group law's exceptional cases inside the batched test's sums ------
# k_sgb_fold / k_sgb_combine add without a doubling branch and redo a sum that
# met two equal operands with the complete formulas (bls_sgb.h).  Equal
# operands are certain in a short last group (an empty bucket below the
# highest non-empty one adds run to q == run) and in groups of replayed
# signatures (equal slice and bucket sums); neither may fail a group or void
# level 0.  2,049 .. 2,056 partials: two full groups and a tail of 1, 4, 8,
# the smallest batches that run the batched test.

@pytest.fixture(scope="module")
def sums_engine():
    """A context of its own with ctx's settings: the group size follows the
    non-subgroup share of the batches a context has collected, and these tests
    state it (1,024: a clean history)."""
    from charon_amd import engine as eng
    e = eng.Engine(0, slots=1, subgroup_batch=eng.SGB_ON, rlc_batch=eng.RLC_L0_ON)
    yield e
    e.close()


def short_tail_batch(e, n_dv, t, n, seed):
    from tools.workload import make_batch
    b = make_batch(e, n_dv, t, n, seed=seed)
    assert 2048 < len(b.sigs) <= 2048 + 16
    return b


@pytest.mark.parametrize("n_dv,t,n,tail", [(683, 2, 3, 1), (513, 3, 4, 4), (514, 3, 4, 8)],
                         ids=["tail1", "tail4", "tail8"])
def test_clean_short_tail_group_passes(sums_engine, n_dv, t, n, tail):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e = sums_engine
    b = short_tail_batch(e, n_dv, t, n, seed=7300 + tail)
    assert len(b.sigs) == 2048 + tail
    res, tk = run(e, b)
    print("short tail", tail, "subgroup", e.subgroup(tk), "level0", e.level0(tk))
    assert_same(res, oracle_run(b))
    assert e.level0(tk) == eng.L0_PASSED
    assert e.subgroup(tk) == {"groups": 3, "failed": 0, "group_size": 1024}
    assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, b.group_sig)


def test_replayed_duties_pass(sums_engine):
    """8 distinct 3-of-4 duties tiled 64 times: 2,048 partials, every group
    full of duplicates (32 signatures, 32 copies of each in a group of 1,024;
    the context's history of non-subgroup partials may pick a smaller group
    size, a multiple of 32 too)."""
    import dataclasses
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    from tools.workload import make_batch
    e = sums_engine
    base = make_batch(e, 8, T, N, seed=7373)
    reps = 64
    b = dataclasses.replace(
        base, n_dv=8 * reps, duty_first=np.arange(8 * reps + 1, dtype=np.uint32) * N,
        sigs=np.tile(base.sigs, (reps, 1)), identifiers=np.tile(base.identifiers, reps),
        pubkey_ids=np.tile(base.pubkey_ids, reps), duty_msg=np.tile(base.duty_msg, reps),
        threshold=np.tile(base.threshold, reps), group_sig=np.tile(base.group_sig, (reps, 1)))
    assert len(b.sigs) == 2048
    res, tk = run(e, b)
    print("replayed subgroup", e.subgroup(tk), "level0", e.level0(tk))
    assert_same(res, oracle_run(b))
    sg = e.subgroup(tk)
    assert sg["failed"] == 0 and sg["group_size"] % 32 == 0 and sg["groups"] == -(-2048 // sg["group_size"]), sg
    assert e.level0(tk) == eng.L0_PASSED
    assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, b.group_sig)


def test_crafted_point_alone_in_the_tail_group_is_caught(sums_engine):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e = sums_engine
    b = short_tail_batch(e, 683, 2, 3, seed=7301)
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        t13 = bytes.fromhex(json.load(f)["points"]["t13"][0])
    pos = len(b.sigs) - 1
    assert pos == 2048  # the sole member of the third group
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = np.frombuffer(t13, dtype=np.uint8)
    res, tk = run(e, b, sigs=sigs)
    print("crafted tail subgroup", e.subgroup(tk), "level0", e.level0(tk))
    assert_same(res, oracle_run(variant(b, sigs=sigs)))
    assert res.partial_status[pos] == eng.PS_ERR_SUBGROUP
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert e.subgroup(tk) == {"groups": 3, "failed": 1, "group_size": 1024}
    assert e.level0(tk) == eng.L0_FAILED
