"""The decode kernels on real gfx950 lanes, stage by stage (tests/devcheck,
devcheck_decode.hip: the product's own k_decode.hip, included and compiled as
the product compiles it) with the directed encodings of tests/edge_decode.py,
against the oracle.

k_decode_sigs, k_subgroup_sigs and k_decode_pubkeys otherwise run only inside
whole launches on honest signatures and a handful of injected ones.  Here
every lane of a wave takes a different branch of the decoder -- real
right-hand sides, coordinates on and beside p, every bad infinity encoding,
both arms of the root -- failures and good keys share a workgroup of the
batched inversion, and the subgroup kernel is entered alone behind a
preloaded gate (edge_decode's docstring lists the branches and what stays
unreachable).  Every comparison is exact: the status, the stored point as
values mod p with every limb below 2^28 and every value below 2p, all-zero
words for a failed partial, and the sentinel in every word a kernel should
not have written.

The lists pass tests/hostcheck under TBG_BOUNDS_CHECK first
(test_decode_edges_host.py).  After a non-zero HIP status no further GPU work
is started by the devcheck modules."""
import pytest

from oracle import bls12_381 as bls
from tests import devcheck
from tests import edge_decode as ed
from tests.edge_points import aff_words
from tests.test_gpu_devcheck import SENT, call, sentinel, u32, untouched

pytestmark = pytest.mark.gpu

AFF_W, G1A_W = ed.AFF_W, ed.G1A_W
S = {name: i for i, name in enumerate(devcheck.DECODE_STAGES)}
SSENT = SENT - (1 << 32)


def consts():
    L = devcheck.lib()
    return L.dc_decode_cnt_words(), L.dc_decode_msm_buckets(), L.dc_decode_binv_block()


def run_sigs(first, last, n, sigs=None, preload=None, rlc_batch=0, sgb=0, sgb_m=0, sgb_bad=None, cap_extra=3):
    """One dc_decode_sigs call.  preload: n pairs (56 words, status) for a
    run that enters at SUBGROUP; every other word of every buffer holds the
    sentinel.  -> (sig_aff words, statuses, counters, msm_off) of the n
    partials, the tails checked here."""
    cnt, msm, _ = consts()
    cap = n + cap_extra
    aff, st = sentinel(cap * AFF_W), sentinel(cap, signed=True)
    for i, (words, status) in enumerate(preload or ()):
        assert len(words) == AFF_W
        aff[i * AFF_W:(i + 1) * AFF_W] = words
        st[i] = status
    counters, msm_off = sentinel(cnt + 1), sentinel(msm + 2)
    data = b"".join(sigs) if sigs else None
    assert data is None or len(data) == 96 * n
    call("dc_decode_sigs", S[first], S[last], n, data, aff, st, counters, msm_off, rlc_batch, sgb, sgb_m,
         u32(sgb_bad) if sgb_bad is not None else None, cap)
    assert untouched(aff, n * AFF_W) and untouched(st, n), "sig_aff / partial_status past partial n"
    return list(aff), list(st), list(counters), list(msm_off)


def check_first_kernel(counters, msm_off, rlc_batch):
    """k_decode_sigs' duties as the chain's first kernel."""
    cnt, msm, _ = consts()
    assert counters[:cnt] == [0] * cnt, "counters not zeroed"
    assert counters[cnt] == SENT, "the word past the counters"
    if rlc_batch:
        bad = [i for i in range(msm + 1) if msm_off[i] != 0]
        assert not bad, ("msm_off not zeroed", bad[:5])
        assert msm_off[msm + 1] == SENT, "the word past msm_off"
    else:
        assert all(w == SENT for w in msm_off), "msm_off written without level 0"


def check_sigs(tag, aff, st, entries, subgroup):
    for i, e in enumerate(entries):
        dec, pt = ed.g2_class(e.data, subgroup)
        err = ed.check_g2_slot(aff[i * AFF_W:(i + 1) * AFF_W], st[i], ed.ps_of(dec), pt)
        assert err is None, (tag, i, e.kind, e.branch, err)


def rotations(items):
    """The list, and the list rotated by one: every lane (pair) position
    sees the other kind of item."""
    return [items, items[1:] + items[:1]]


def test_stage_codes_and_constants():
    assert devcheck.DECODE_STAGES == ["DECODE", "SUBGROUP"]
    cnt, msm, blk = consts()
    assert 0 < cnt < 64 and msm > 64 and blk % 64 == 0
    n = len(ed.g2_entries())
    assert n > 64 and n % 64 != 0  # more than one wave of k_decode_sigs, the last partly filled


def test_whole_g2_list_through_decode():
    """k_decode_sigs alone: status, x and y per lane against the oracle's
    decode without the subgroup check; the first-kernel duties on the way."""
    for entries in rotations(ed.g2_entries()):
        aff, st, counters, msm_off = run_sigs("DECODE", "DECODE", len(entries), sigs=[e.data for e in entries])
        check_sigs("decode", aff, st, entries, False)
        check_first_kernel(counters, msm_off, 0)


def test_decode_then_subgroup():
    """launch_decode_sigs itself with every signature tested alone (sgb = 0):
    the final status is the oracle's full class.  The order-13 point runs to
    infinity in mid-ladder in the same wave as valid signatures."""
    base = ed.g2_entries()
    tor = [i for i, e in enumerate(base) if e.kind == "sub_tor"]
    # k_subgroup_sigs: one lane pair per partial, 32 partials a wave
    assert tor and all(any(e.kind == "valid" for e in base[i // 32 * 32:i // 32 * 32 + 32]) for i in tor)
    for entries in rotations(base):
        aff, st, counters, msm_off = run_sigs("DECODE", "SUBGROUP", len(entries), sigs=[e.data for e in entries])
        check_sigs("full", aff, st, entries, True)
        check_first_kernel(counters, msm_off, 0)
    classes = {ed.g2_class(e.data, True)[0] for e in base}
    assert classes == {ed.DEC_OK, ed.DEC_IDENTITY, ed.DEC_ERR_FLAGS, ed.DEC_ERR_FIELD, ed.DEC_ERR_NOT_ON_CURVE,
                       ed.DEC_ERR_SUBGROUP}


def subgroup_preload(n):
    """n lanes for k_subgroup_sigs alone: the points of subgroup_points() in
    the limb forms of SUBGROUP_FORMS, and every 11th lane an error status (or
    a verified one) over sentinel words."""
    pts, forms = ed.subgroup_points(), ed.SUBGROUP_FORMS
    lanes = []
    for i in range(n):
        if i % 11 == 5:
            lanes.append(("left_alone", None, [SENT] * AFF_W, (-3, -5, 1, 0, -1)[(i // 11) % 5]))
        else:
            name, p = pts[i % len(pts)]
            lanes.append((name, p, aff_words(p, forms[(i // len(pts) + i) % len(forms)]), ed.PS_NOT_VERIFIED))
    return lanes


def test_subgroup_alone_behind_the_batched_tests_gate():
    """sgb = 1, groups of 64, only group 1 marked bad: its points outside G2
    are rejected and zeroed, its G2 points stay; groups 0 and 2 and every lane
    with another status come back bit-identical."""
    n, m, bad = 130, 64, [0, 1, 0]
    lanes = subgroup_preload(n)
    for g in range(3):  # points outside G2 in all three groups
        assert any(p is not None and not bls.g2_in_subgroup(p) for _, p, _, _ in lanes[g * m:(g + 1) * m])
    assert any(name == "left_alone" for name, _, _, _ in lanes[m:2 * m])
    aff, st, counters, msm_off = run_sigs("SUBGROUP", "SUBGROUP", n, preload=[(w, s) for _, _, w, s in lanes], sgb=1,
                                          sgb_m=m, sgb_bad=bad)
    cnt, _, _ = consts()
    assert counters == [SENT] * (cnt + 1) and all(w == SENT for w in msm_off)  # not the first kernel
    rejected = 0
    for i, (name, p, words, status) in enumerate(lanes):
        got = aff[i * AFF_W:(i + 1) * AFF_W]
        if bad[i // m] and p is not None and not bls.g2_in_subgroup(p):
            assert st[i] == ed.DEC_ERR_SUBGROUP and got == [0] * AFF_W, (i, name)
            rejected += 1
        else:
            assert st[i] == status and got == [w & 0xFFFFFFFF for w in words], (i, name)
    assert rejected >= 16


def test_subgroup_alone_every_lane_tested():
    """The same lanes with sgb = 0: every point outside G2 is rejected."""
    n = 130
    lanes = subgroup_preload(n)
    aff, st, _, _ = run_sigs("SUBGROUP", "SUBGROUP", n, preload=[(w, s) for _, _, w, s in lanes])
    for i, (name, p, words, status) in enumerate(lanes):
        got = aff[i * AFF_W:(i + 1) * AFF_W]
        if p is not None and not bls.g2_in_subgroup(p):
            assert st[i] == ed.DEC_ERR_SUBGROUP and got == [0] * AFF_W, (i, name)
        else:
            assert st[i] == status and got == [w & 0xFFFFFFFF for w in words], (i, name)


def test_first_kernel_duties():
    """launch_decode_sigs sizes the grid for the zeroing: one partial and no
    partial at all still clear every counter, and an unfused level 0 clears
    msm_off[0 .. MSM_BUCKETS] and not the word behind it."""
    one = [next(e for e in ed.g2_entries() if e.kind == "valid")]
    aff, st, counters, msm_off = run_sigs("DECODE", "SUBGROUP", 1, sigs=[one[0].data])
    check_sigs("n1", aff, st, one, True)
    check_first_kernel(counters, msm_off, 0)
    aff, st, counters, msm_off = run_sigs("DECODE", "SUBGROUP", 1, sigs=[one[0].data], rlc_batch=1)
    check_sigs("n1 rlc", aff, st, one, True)
    check_first_kernel(counters, msm_off, 1)
    aff, st, counters, msm_off = run_sigs("DECODE", "SUBGROUP", 0)
    check_first_kernel(counters, msm_off, 0)


def run_keys(entries, cap_extra=3):
    n = len(entries)
    cap = n + cap_extra
    out, outx, st = sentinel(cap * G1A_W), sentinel(cap * G1A_W), sentinel(cap, signed=True)
    call("dc_decode_pubkeys", n, b"".join(e.data for e in entries), out, outx, st, cap)
    assert untouched(out, n * G1A_W) and untouched(outx, n * G1A_W) and untouched(st, n), "past key n"
    return list(out), list(outx), list(st)


def check_keys(tag, out, outx, st, entries):
    for i, e in enumerate(entries):
        dec, pt = ed.g1_class(e.data)
        err = ed.check_g1_slot(out[i * G1A_W:(i + 1) * G1A_W], outx[i * G1A_W:(i + 1) * G1A_W], st[i], dec, pt)
        assert err is None, (tag, i, e.kind, e.branch, err)


def test_whole_g1_list_in_a_mixed_workgroup():
    """n = BINV_BLOCK + 3: failures at lanes 0, BINV_BLOCK - 1, BINV_BLOCK and
    n - 1 with valid keys around them, so block_jac_to_aff inverts for a
    workgroup of present and absent lanes and for a partly filled last one
    with a failure in it; then a lone valid key and a lone point of order 3."""
    blk = consts()[2]
    entries = ed.g1_layout(blk)
    assert len(entries) == blk + 3
    check_keys("mixed", *run_keys(entries), entries)
    for kind in ("valid", "low3_plus"):
        one = [next(e for e in ed.g1_entries() if e.kind == kind)]
        check_keys(kind, *run_keys(one), one)


def test_checker_sees_a_wrong_word():
    """The comparison reaches every word the kernels wrote: one limb off by
    one, one status, one expected limb and one expected status are rejected."""
    entries = ed.g2_entries()[:20]
    n = len(entries)
    aff, st, counters, msm_off = run_sigs("DECODE", "DECODE", n, sigs=[e.data for e in entries], cap_extra=0)
    check_sigs("ok", aff, st, entries, False)
    ok = next(i for i, e in enumerate(entries) if ed.g2_class(e.data, False)[0] == ed.DEC_OK)
    failed = next(i for i, e in enumerate(entries) if ed.g2_class(e.data, False)[0] < 0)
    for j in (0, 13, 14, 41, 55):
        bad = list(aff)
        bad[ok * AFF_W + j] += 1
        with pytest.raises(AssertionError):
            check_sigs("bad", bad, st, entries, False)
    bad = list(aff)
    bad[failed * AFF_W + 7] = 1
    with pytest.raises(AssertionError):
        check_sigs("bad", bad, st, entries, False)
    for i, v in ((ok, ed.DEC_ERR_FLAGS), (failed, ed.PS_NOT_VERIFIED), (failed, st[failed] - 1)):
        bad = list(st)
        bad[i] = v
        with pytest.raises(AssertionError):
            check_sigs("bad", aff, bad, entries, False)
    # one EXPECTED limb and one EXPECTED status, in the test's own copy
    dec, pt = ed.g2_class(entries[ok].data, False)
    words = aff[ok * AFF_W:(ok + 1) * AFF_W]
    assert ed.check_g2_slot(words, st[ok], ed.ps_of(dec), pt) is None
    assert ed.check_g2_slot(words, st[ok], ed.ps_of(dec), (pt[0], (pt[1][0], pt[1][1] ^ 1))) is not None
    assert ed.check_g2_slot(words, st[ok], ed.PS_ERR_IDENTITY, pt) is not None
    bad = list(counters)
    bad[3] = 1
    with pytest.raises(AssertionError):
        check_first_kernel(bad, msm_off, 0)
    bad = list(msm_off)
    bad[-1] = 0
    with pytest.raises(AssertionError):
        check_first_kernel(counters, bad, 0)
