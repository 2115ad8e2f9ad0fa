"""The fused level 0's per-duty key side on the GPU against oracle/c.

In fused launches of at least tbg_config.l0_duty_partials partials k_rlc_g1_l0 runs
one lane per duty: P_d = sum_i [r_i] pk_i in Straus' joint form (bls_rlc.h
rlc_duty_keys_l0f), its affine form and dv_state written by the same kernel,
k_rlc_duty_sum<DSUM_L0_P> not launched.  Settings: subgroup_batch = SGB_ON,
level 0 forced on, l0_duty_partials = 1 (always per duty), 512 DVs x 4 = 2,048
partials -- the smallest fused launch -- and 2,052 partials for the mixed
thresholds.  Every result (per-partial status, per-duty status, every
aggregate) is compared with oracle/c through the helpers of
test_gpu_fullsize.py, and with a context that runs no level 0.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_DV, T, N = 512, 3, 4
DUTY_SUM = "k_rlc_duty_sum<DSUM_L0_P>"


def merged(parts, order):
    """One batch of the duties of `parts` (keys loaded back to back) in the
    order [(part, duty), ...]."""
    first = parts[0].pk_first
    at = first
    for p in parts:
        assert p.pk_first == at
        at += len(p.pubshares)
    m0 = np.cumsum([0] + [p.n_dv for p in parts])
    sl = [slice(int(parts[k].duty_first[d]), int(parts[k].duty_first[d + 1])) for k, d in order]
    cat = lambda name: np.concatenate([getattr(parts[k], name)[s] for (k, _), s in zip(order, sl)])  # noqa: E731
    pick = lambda name: np.array([getattr(parts[k], name)[d] for k, d in order])  # noqa: E731
    msgs = [m for p in parts for m in p.msgs]
    sizes = np.array([s.stop - s.start for s in sl], dtype=np.uint32)
    return dataclasses.replace(
        parts[0], n_dv=len(order), t=0, n=0, duty_first=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32),
        sigs=cat("sigs"), identifiers=cat("identifiers"), pubkey_ids=cat("pubkey_ids"),
        pubshares=np.concatenate([p.pubshares for p in parts]),
        msg_data=np.frombuffer(b"".join(msgs), dtype=np.uint8), msg_off=np.arange(len(msgs) + 1, dtype=np.uint32) * 32,
        duty_msg=np.array([m0[k] + parts[k].duty_msg[d] for k, d in order], dtype=np.uint32),
        threshold=pick("threshold").astype(np.uint32), group_sig=pick("group_sig"), injected=cat("injected"),
        expect_ok=pick("expect_ok"), secrets=[parts[k].secrets[d] for k, d in order], shares=[], msgs=msgs, pk_first=first)


@pytest.fixture(scope="module")
def ctx():
    """Contexts: per duty always / never / from 2,049 partials, and one without
    level 0; the batches with their keys resident under the same ids in all,
    and their oracle results (computed once)."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_batch
    kw = dict(slots=1, subgroup_batch=eng.SGB_ON)
    es = dict(duty=eng.Engine(0, rlc_batch=eng.RLC_L0_ON, l0_duty_partials=eng.L0_DUTY_ALWAYS, **kw),
              partial=eng.Engine(0, rlc_batch=eng.RLC_L0_ON, l0_duty_partials=eng.L0_DUTY_NEVER, **kw),
              thr=eng.Engine(0, rlc_batch=eng.RLC_L0_ON, l0_duty_partials=N_DV * N + 1, **kw),
              off=eng.Engine(0, rlc_batch=eng.RLC_L0_OFF, **kw))
    e = es["duty"]
    clean = make_batch(e, N_DV, T, N, seed=8080)
    # 175 x 4 + 96 x 7 + 68 x 10 = 2,052 partials, the three kinds interleaved
    parts = [make_batch(e, 175, 3, 4, seed=8181), make_batch(e, 96, 5, 7, seed=8182),
             make_batch(e, 68, 7, 10, seed=8183)]
    order, left = [], [0, 0, 0]
    while any(left[k] < parts[k].n_dv for k in range(3)):
        for k in range(3):
            if left[k] < parts[k].n_dv:
                order.append((k, left[k]))
                left[k] += 1
    mixed = merged(parts, order)
    over = make_batch(e, N_DV + 1, T, N, seed=8284)
    assert len(clean.sigs) == 2048 and len(mixed.sigs) == 2052 and len(over.sigs) == 2052
    for name, other in es.items():
        if other is not e:
            at = clean.pk_first
            for b in [clean] + parts + [over]:
                first, st = other.load_pubkeys(b.pubshares)
                assert first == at == b.pk_first and (st == 0).all()
                at += len(b.pubshares)
    yield dict(es=es, clean=clean, mixed=mixed, over=over,
               ref=dict(clean=oracle_run(clean), mixed=oracle_run(mixed), over=oracle_run(over)))
    for x in es.values():
        x.close()


def run(e, b, sigs=None, pubkey_ids=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg,
                 pubkey_ids=b.pubkey_ids if pubkey_ids is None else pubkey_ids, duty_threshold=b.threshold)
    return e.collect(t), t


def variant(b, **kw):
    import copy
    v = copy.copy(b)
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def kernels(e, t):
    return {name for name, _ in e.replay_profile(t)}


def same_bytes(a, b):
    return (np.array_equal(a.partial_status, b.partial_status) and np.array_equal(a.duty_status, b.duty_status) and
            np.array_equal(a.agg, b.agg))


@pytest.mark.parametrize("which", ["clean", "mixed"])
def test_clean_batch_passes_per_duty(ctx, which):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    e, b = ctx["es"]["duty"], ctx[which]
    res, t = run(e, b)
    assert_same(res, ctx["ref"][which])
    assert e.level0(t) == eng.L0_PASSED
    assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == 0).all()
    assert np.array_equal(res.agg, b.group_sig)
    ks = kernels(e, t)
    assert "k_rlc_g1_l0" in ks and DUTY_SUM not in ks and "k_l0f_horner" in ks, sorted(ks)
    assert e.level0(t) == eng.L0_PASSED  # (the profiled replay too)
    res_off, t_off = run(ctx["es"]["off"], b)
    assert ctx["es"]["off"].level0(t_off) == eng.L0_NOT_RUN
    assert same_bytes(res, res_off)


def test_duplicate_pubkey_id_inside_a_duty(ctx):
    """Partial 1 of a duty replays partial 0's key and signature (its own
    identifier): both verify, and the duty's P_d adds two multiples of one key."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e, b = ctx["es"]["duty"], ctx["clean"]
    ids, sigs = np.array(b.pubkey_ids, copy=True), np.array(b.sigs, copy=True)
    for d in (0, 200, N_DV - 1):
        ids[N * d + 1], sigs[N * d + 1] = ids[N * d], sigs[N * d]
    res, t = run(e, b, sigs=sigs, pubkey_ids=ids)
    assert_same(res, oracle_run(variant(b, sigs=sigs, pubkey_ids=ids)))
    assert (res.partial_status == eng.PS_VALID).all()
    assert e.level0(t) == eng.L0_PASSED


def test_one_missing_pubshare_voids_level0(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    from tools.workload import NO_PUBKEY
    e, b = ctx["es"]["duty"], ctx["clean"]
    pos = 1024 + 6
    ids = np.array(b.pubkey_ids, copy=True)
    ids[pos] = NO_PUBKEY
    res, t = run(e, b, pubkey_ids=ids)
    assert res.partial_status[pos] == eng.PS_ERR_PUBKEY
    assert e.level0(t) == eng.L0_FAILED
    assert_same(res, oracle_run(variant(b, pubkey_ids=ids)))
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]


def test_duty_whose_partials_all_fail_decode(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e, b = ctx["es"]["duty"], ctx["clean"]
    d = 301
    sigs = np.array(b.sigs, copy=True)
    sigs[N * d:N * d + N, 0] &= 0x7F  # no compression flag: a decode error, no candidate
    res, t = run(e, b, sigs=sigs)
    assert_same(res, oracle_run(variant(b, sigs=sigs)))
    assert (res.partial_status[N * d:N * d + N] < 0).all()
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == list(range(N * d, N * d + N))
    assert e.level0(t) == eng.L0_PASSED  # the duty is RLC_NONE: the rest passes as one check


@pytest.mark.parametrize("pos", [0, 2047], ids=["first", "last"])
def test_one_wrong_share_partial_fails_level0(ctx, pos):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    e, b = ctx["es"]["duty"], ctx["clean"]
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = b.sigs[pos + 1 if pos % N == 0 else pos - 1]  # another share of its DV signed it
    res, t = run(e, b, sigs=sigs)
    assert e.level0(t) == eng.L0_FAILED
    assert_same(res, oracle_run(variant(b, sigs=sigs)))
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert res.partial_status[pos] == eng.PS_INVALID


@pytest.mark.parametrize("which", ["clean", "over"], ids=["just_under", "just_over"])
def test_both_forms_give_identical_bytes_around_the_threshold(ctx, which):
    """l0_duty_partials = 2,049: the 2,048-partial batch keeps one lane per partial and
    k_rlc_duty_sum<DSUM_L0_P>, the 2,052-partial batch runs one lane per duty; each
    gives the bytes of the contexts forced to either form."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    es, b = ctx["es"], ctx[which]
    out = {}
    for name in ("thr", "duty", "partial"):
        res, t = run(es[name], b)
        assert es[name].level0(t) == eng.L0_PASSED
        out[name] = (res, DUTY_SUM in kernels(es[name], t))
    assert_same(out["thr"][0], ctx["ref"][which])
    assert same_bytes(out["thr"][0], out["duty"][0]) and same_bytes(out["thr"][0], out["partial"][0])
    assert out["duty"][1] is False and out["partial"][1] is True
    assert out["thr"][1] is (which == "clean")
