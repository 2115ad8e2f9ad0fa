"""The fused level 0's S role inside the key-side kernel's grid, on the GPU
against oracle/c.

In a fused launch of at least tbg_config.l0_tail_partials partials the first
workgroups of k_rlc_g1_l0's grid form S from the batched subgroup test's sums
(bls_l0tail.h; k_msm.hip "the S role"): one wave per chunk of 128 points of a
column, the columns and then the Horner steps handed over to the last
workgroup to arrive at a counter, while every other workgroup runs the key
side; k_l0f_reduce, k_l0f_fold and k_l0f_horner do not run then.  Smaller
launches keep those three kernels.

Settings: 3-of-4, subgroup_batch = SGB_ON, level 0 forced on, one slot,
l0_tail_partials = L0_TAIL_ALWAYS but for the threshold test at the end.
  small   512 DVs = 2,048 partials, the smallest fused launch: 2 subgroup
          groups of 1,024, 64 slices of T -- one chunk per column, 19 S
          workgroups; one lane per partial on the key side.
  large   4,104 DVs = 16,416 partials, one lane per duty on the key side:
          17 groups (the last of 32 partials), 544 slices of T = 4 chunks of
          128 and one of 32 -- 23 S workgroups, more than the 8 XCDs; on the
          triple schedule in groups of 2,048: 9 groups, 576 slices, 5 chunks.
Every result (per-partial status, per-duty status, every aggregate) is
compared bit for bit with oracle/c through the helpers of
test_gpu_fullsize.py; the references are computed once per module.
"""
import copy
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T, N = 3, 4
N_SMALL, N_LARGE, N_SETS, N_PART = 512, 4104, 2048, 600
TRI_M = 2048
DUTY_SUM = "k_rlc_duty_sum<DSUM_L0_P>"
GONE = {"k_l0f_reduce", "k_l0f_fold", "k_l0f_horner"}
MSM_KERNELS = {"k_msm_scan", "k_msm_scatter", "k_msm_bucket_part", "k_msm_bucket", "k_msm_tree", "k_msm_tree_final"}


@pytest.fixture(scope="module")
def ctx():
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_batch
    base = dict(slots=1, subgroup_batch=eng.SGB_ON, rlc_batch=eng.RLC_L0_ON)
    kw = dict(l0_tail_partials=eng.L0_TAIL_ALWAYS, **base)
    es = dict(thr=eng.Engine(0, l0_duty_partials=eng.L0_DUTY_ALWAYS, l0_tail_partials=N_LARGE * N, **base),
              dflt=eng.Engine(0, l0_duty_partials=eng.L0_DUTY_ALWAYS, **base),
              duty=eng.Engine(0, l0_duty_partials=eng.L0_DUTY_ALWAYS, **kw),
              partial=eng.Engine(0, l0_duty_partials=eng.L0_DUTY_NEVER, **kw),
              tri=eng.Engine(0, l0_duty_partials=eng.L0_DUTY_ALWAYS, sgb_tri_partials=N_LARGE * N, sgb_tri_m=TRI_M,
                             **kw))
    e = es["duty"]
    bs = dict(small=make_batch(e, N_SMALL, T, N, seed=1601), large=make_batch(e, N_LARGE, T, N, seed=1602),
              sets=make_batch(e, N_SETS, T, N, seed=1603), p0=make_batch(e, N_PART, T, N, seed=1604),
              p1=make_batch(e, N_PART, T, N, seed=1605))
    assert len(bs["small"].sigs) == 2048 and len(bs["large"].sigs) == 16416
    for other in (es["partial"], es["tri"], es["thr"], es["dflt"]):
        for b in bs.values():  # (the order make_batch loaded them in)
            first, st = other.load_pubkeys(b.pubshares)
            assert first == b.pk_first and (st == 0).all()
    yield dict(es=es, bs=bs, ref={k: oracle_run(b) for k, b in bs.items()})
    for x in es.values():
        x.close()


def run(e, b, sigs=None, pubkey_ids=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg,
                 pubkey_ids=b.pubkey_ids if pubkey_ids is None else pubkey_ids, duty_threshold=b.threshold)
    return e.collect(t), t


def kernels(e, t):
    return {name for name, _ in e.replay_profile(t)}


def ref_with(b, clean_ref, duty, **changed):
    """The clean batch's oracle results with duty `duty` taken from oracle/c
    on the changed inputs (every other duty's inputs are the clean ones)."""
    from tests.test_gpu_fullsize import oracle_run
    v = copy.copy(b)
    for k, x in changed.items():
        setattr(v, k, x)
    ps, ds, agg = (np.array(x, copy=True) for x in clean_ref)
    p, d, a = oracle_run(v, duty, duty + 1)
    ps[int(b.duty_first[duty]):int(b.duty_first[duty + 1])] = p
    ds[duty] = d[0]
    agg[duty] = a[0]
    return ps, ds, agg


def assert_clean_pass(e, b, ref, res, t):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    assert_same(res, ref)
    assert e.level0(t) == eng.L0_PASSED
    assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == 0).all()
    assert np.array_equal(res.agg, b.group_sig)


# ---- (a) one chunk per column, one lane per partial on the key side ----------
def test_one_chunk_per_column(ctx):
    from charon_amd import engine as eng
    e, b = ctx["es"]["partial"], ctx["bs"]["small"]
    res, t = run(e, b)
    assert_clean_pass(e, b, ctx["ref"]["small"], res, t)
    assert e.subgroup(t) == {"groups": 2, "failed": 0, "group_size": 1024}
    ks = kernels(e, t)
    assert "k_rlc_g1_l0" in ks and DUTY_SUM in ks and not (GONE & ks) and not (MSM_KERNELS & ks), sorted(ks)
    assert e.level0(t) == eng.L0_PASSED  # (the profiled replay too)


# ---- (b) several chunks per column, one lane per duty ------------------------
def test_several_chunks_with_a_short_last_one(ctx):
    from charon_amd import engine as eng
    e, b = ctx["es"]["duty"], ctx["bs"]["large"]
    res, t = run(e, b)
    assert_clean_pass(e, b, ctx["ref"]["large"], res, t)
    sg = e.subgroup(t)
    assert sg == {"groups": 17, "failed": 0, "group_size": 1024}
    assert sg["groups"] * (sg["group_size"] // 32) == 544 > 512  # slices of T: chunks of 128, 128, 128, 128, 32
    ks = kernels(e, t)
    assert "k_rlc_g1_l0" in ks and DUTY_SUM not in ks and not (GONE & ks) and not (MSM_KERNELS & ks), sorted(ks)
    assert e.level0(t) == eng.L0_PASSED


# ---- (c) the triple schedule at small size ----------------------------------
def test_triple_schedule(ctx):
    e, b = ctx["es"]["tri"], ctx["bs"]["large"]
    res, t = run(e, b)
    sg = e.subgroup(t, schedule=True)
    assert sg == {"groups": 9, "failed": 0, "group_size": TRI_M, "schedule": "triple"}, sg
    assert e.subgroup(t, schedule=True)["schedule"] == "triple"
    assert_clean_pass(e, b, ctx["ref"]["large"], res, t)


# ---- (d) void paths: the group levels' exact verdicts -----------------------
def test_missing_pubshare_voids_level0_while_the_s_role_runs(ctx):
    """The key role marks the partial and sets CNT_L0_BAD in the same kernel
    in which the S role runs (and no longer looks at the flag)."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    from tools.workload import NO_PUBKEY
    e, b = ctx["es"]["duty"], ctx["bs"]["large"]
    pos = 9002
    ids = np.array(b.pubkey_ids, copy=True)
    ids[pos] = NO_PUBKEY
    res, t = run(e, b, pubkey_ids=ids)
    assert e.level0(t) == eng.L0_FAILED
    assert res.partial_status[pos] == eng.PS_ERR_PUBKEY
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert_same(res, ref_with(b, ctx["ref"]["large"], pos // N, pubkey_ids=ids))


def test_wrong_share_partial_fails_level0(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    e, b = ctx["es"]["duty"], ctx["bs"]["large"]
    pos = 16415  # the last partial, in the short last subgroup group
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = b.sigs[pos - 1]  # another share of its DV signed it
    res, t = run(e, b, sigs=sigs)
    assert e.level0(t) == eng.L0_FAILED  # level 0 ran and failed
    assert res.partial_status[pos] == eng.PS_INVALID
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert_same(res, ref_with(b, ctx["ref"]["large"], pos // N, sigs=sigs))


def test_non_subgroup_signature_voids_level0(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    e, b = ctx["es"]["duty"], ctx["bs"]["large"]
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        t13 = bytes.fromhex(json.load(f)["points"]["t13"][0])
    pos = 5 * 1024 + 77
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = np.frombuffer(t13, dtype=np.uint8)
    res, t = run(e, b, sigs=sigs)
    assert e.subgroup(t)["failed"] == 1
    assert e.level0(t) == eng.L0_FAILED
    assert res.partial_status[pos] == eng.PS_ERR_SUBGROUP
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert_same(res, ref_with(b, ctx["ref"]["large"], pos // N, sigs=sigs))


# ---- (e) replays: k_decode_sigs zeroes the role's counters every time --------
def test_replays_give_identical_outputs(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    e, b = ctx["es"]["duty"], ctx["bs"]["large"]
    res, t = run(e, b)
    assert_clean_pass(e, b, ctx["ref"]["large"], res, t)
    for _ in range(3):
        e.replay_plan([t], [0])
        e.synchronize()
        again = e.fetch(t, b.n_dv, len(b.sigs))
        assert np.array_equal(again.partial_status, res.partial_status)
        assert np.array_equal(again.duty_status, res.duty_status) and np.array_equal(again.agg, res.agg)
        assert e.level0(t) == eng.L0_PASSED
    # a prefix of a two-batch device batch: 2,400 of its 4,800 partials
    parts = [ctx["bs"]["p0"], ctx["bs"]["p1"]]
    refs = [ctx["ref"]["p0"], ctx["ref"]["p1"]]
    args = [dict(duty_first=p.duty_first, sigs=p.sigs, identifiers=p.identifiers, msgs=(p.msg_data, p.msg_off),
                 duty_msg=p.duty_msg, pubkey_ids=p.pubkey_ids, duty_threshold=p.threshold) for p in parts]
    tickets = e.submit_group(eng.OP_VERIFY_AGGREGATE, args)
    first = [e.collect(tk) for tk in tickets]
    for r, ref in zip(first, refs):
        assert_same(r, ref)
    assert e.level0(tickets[0]) == eng.L0_PASSED
    for _ in range(3):
        e.replay_plan([tickets[0]], [1])
        e.synchronize()
        assert e.level0(tickets[0]) == eng.L0_PASSED
        again = e.fetch(tickets[0], parts[0].n_dv, len(parts[0].sigs))
        assert np.array_equal(again.partial_status, first[0].partial_status)
        assert np.array_equal(again.duty_status, first[0].duty_status) and np.array_equal(again.agg, first[0].agg)


# ---- (f) a set launch -------------------------------------------------------
def test_set_launch_passes_level0(ctx):
    from charon_amd import engine as eng
    e, b = ctx["es"]["duty"], ctx["bs"]["sets"]
    set_first = np.arange(0, N_SETS + 1, 4, dtype=np.uint32)  # 512 sets of four duties
    t = e.submit_sets(set_first, duty_first=b.duty_first, sigs=b.sigs, identifiers=b.identifiers,
                      msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids)
    res = e.collect_sets(t)
    assert len(res.set_status) == 512 and (res.set_status == eng.SS_VALID).all()
    ps, ds, _ = ctx["ref"]["sets"]
    assert (ds == 0).all() and np.array_equal(res.partial_status, ps)  # every partial valid, as oracle/c finds
    assert e.level0(t) == eng.L0_PASSED


# ---- the threshold: the same bytes from either form --------------------------
def test_threshold_between_the_role_and_the_three_kernels(ctx):
    """l0_tail_partials = 16,416: the 16,416-partial batch forms S in the key
    kernel's grid, the 8,192-partial one by k_l0f_reduce / _fold / _horner; the
    default (131,072) keeps the three kernels for both.  Each gives the bytes of
    the context forced to the role."""
    from charon_amd import engine as eng
    es = ctx["es"]
    for which, role_at_thr in (("large", True), ("sets", False)):
        b, out = ctx["bs"][which], {}
        for name, role in (("duty", True), ("thr", role_at_thr), ("dflt", False)):
            res, t = run(es[name], b)
            assert_clean_pass(es[name], b, ctx["ref"][which], res, t)
            ks = kernels(es[name], t)
            assert "k_rlc_g1_l0" in ks and not (MSM_KERNELS & ks), sorted(ks)
            assert (not (GONE & ks)) if role else GONE <= ks, (which, name, sorted(ks))
            assert es[name].level0(t) == eng.L0_PASSED
            out[name] = res
        for name in ("thr", "dflt"):
            assert np.array_equal(out[name].partial_status, out["duty"].partial_status)
            assert np.array_equal(out[name].duty_status, out["duty"].duty_status)
            assert np.array_equal(out[name].agg, out["duty"].agg)
