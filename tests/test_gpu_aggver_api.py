"""GPU tests of the Python layers over TBG_OP_AGGREGATE_VERIFY:
tbls.aggregate_and_verify_batch / aggregate_and_verify (strings and types),
parsig.Aggregator.aggregate_verified_batch over the duty types of
tests/golden/parsig_sets.json (a tampered item dropped, subscribers not called
for it), and dkg.agg_and_verify_deposit_data against the existing pair
agg_deposit_data_sigs + verify_deposit_aggregates."""
import json
import os

import pytest

from charon_amd import dkg, parsig, tbls
from charon_amd import engine as eng
from charon_amd.parsig import ParSignedData
from tests.test_gpu_dkg import _deposit_inputs
from tests.test_gpu_parsig import _sets, _spec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(HERE, "golden", "parsig_sets.json")) as f:
        return json.load(f)


def _deposit_duties():
    data, _, msgs = _deposit_inputs()
    return [{"partials": [tbls.PartialSignature(p.share_idx, tbls.Signature(p.signature)) for p in data[dv]],
             "msg": msgs[dv], "public_key": tbls.PublicKey(dv)} for dv in data], data, msgs


def test_tbls_batch_strings_and_types(engine):
    duties, data, msgs = _deposit_duties()
    want = dkg.agg_deposit_data_sigs(*_deposit_inputs(), engine)
    dvs = list(data)
    clean = tbls.aggregate_and_verify_batch(duties, engine)
    assert all(isinstance(r, tbls.Signature) for r in clean)
    assert [r.raw for r in clean] == [want[dv] for dv in dvs]
    p = duties[0]["partials"]
    undecodable = tbls.Signature(bytes([p[0].signature.raw[0] & 0x7F]) + p[0].signature.raw[1:])
    cases = [
        dict(duties[0], public_key=duties[1]["public_key"]),                      # another DV's key
        dict(duties[0], msg=msgs[dvs[1]]),                                         # another DV's message
        dict(duties[0], partials=[p[0], duties[1]["partials"][1]] + p[2:]),        # another DV's partial
        dict(duties[0], public_key=None),
        dict(duties[0], public_key=bytes([0x9F]) + bytes([0xFF]) * 47),            # x >= p
        dict(duties[0], public_key=bytes([0xC0]) + bytes(47)),                     # the identity
        dict(duties[0], partials=p[:1]),
        dict(duties[0], partials=[p[0], tbls.PartialSignature(p[0].identifier, p[1].signature)] + p[2:]),
        dict(duties[0], partials=[tbls.PartialSignature(1, undecodable)] + p[1:]),
        dict(duties[0], partials=p[1:], public_key=duties[0]["public_key"].raw),   # three of four, raw key bytes
    ]
    got = tbls.aggregate_and_verify_batch(cases + duties[1:], engine)
    assert all(isinstance(r, tbls.TblsError) for r in got[:9])
    assert [str(r) for r in got[:3]] == ["invalid aggregated signature"] * 3
    assert str(got[3]) == "verify aggregate: public key cannot be nil"
    assert str(got[4]) == "verify aggregate: public key invalid bytes - not in field"
    assert str(got[5]) == "verify aggregate: public key is the identity"
    assert str(got[6]) == "aggregate signatures: insufficient partial signatures"
    assert str(got[7]) == "aggregate signatures: duplicate identifier"
    assert str(got[8]) == "uncompress sig"
    assert [r.raw for r in got[9:]] == [want[dv] for dv in dvs]
    assert tbls.aggregate_and_verify_batch([], engine) == []
    # the single-duty form returns the signature or raises
    d = duties[2]
    assert tbls.aggregate_and_verify(d["partials"], d["msg"], d["public_key"], engine).raw == want[dvs[2]]
    with pytest.raises(tbls.TblsError, match="^invalid aggregated signature$"):
        tbls.aggregate_and_verify(d["partials"], d["msg"], duties[3]["public_key"], engine)
    # equal to the two calls it replaces
    for c, r in zip(cases, got):
        a = tbls.aggregate_batch([c["partials"]], engine)[0]
        if isinstance(a, tbls.Signature) and c["public_key"] is not None:
            try:
                ok = tbls.verify(c["public_key"] if isinstance(c["public_key"], tbls.PublicKey)
                                 else tbls.PublicKey(c["public_key"]), c["msg"], a, engine)
            except tbls.TblsError:
                ok = False
            assert ok == isinstance(r, tbls.Signature)
        elif not isinstance(a, tbls.Signature):
            assert str(a) == str(r)


def test_aggregator_verified_batch(fx, engine):
    """Every (duty, DV) of the fixture from its three honest peers; one item tampered."""
    spec = _spec(fx)
    sets = _sets(fx)
    clean_sets = [k for k, s in enumerate(fx["sets"]) if s["expect_error"] is None]
    by_duty = {}
    for k in clean_sets:
        duty, pset = sets[k]
        for pk, data in pset.items():
            by_duty.setdefault((duty, pk), []).append(data)
    t = fx["threshold"]
    items = [(duty, pk, parts[:t]) for (duty, pk), parts in by_duty.items() if len(parts) >= t]
    assert len({duty.type for duty, _, _ in items}) > 1, "the fixture's duty types"
    expect = {(fx["duties"][a["duty"]]["slot"], a["pubkey"]): a["agg"] for a in fx["aggregates"]}
    # tamper one item: its second partial comes from another DV's share (decodes, wrong aggregate)
    bad_k = 1
    duty, pk, parts = items[bad_k]
    other = next(p for d2, pk2, ps in items if pk2 != pk and d2 == duty for p in ps if p.share_idx == parts[1].share_idx)
    tampered = [parts[0], ParSignedData(parts[1].domain, parts[1].epoch, parts[1].message_root, other.signature,
                                        parts[1].share_idx)] + list(parts[2:])
    items[bad_k] = (duty, pk, tampered)
    items.append((duty, pk, parts[:t - 1]))  # below threshold: host-side refusal
    items.append((duty, pk, [ParSignedData("NO_SUCH_DOMAIN", p.epoch, p.message_root, p.signature, p.share_idx)
                             for p in parts]))
    agg = parsig.Aggregator(t, engine)
    seen = []
    agg.subscribe(lambda d, k, signed: seen.append((d.slot, k, signed.signature.hex())))
    out = agg.aggregate_verified_batch(items, spec)
    plain = parsig.Aggregator(t, engine).aggregate_batch(items[:-2])
    n = len(items) - 2
    for k in range(n):
        d, key, _ = items[k]
        if k == bad_k:
            assert isinstance(out[k], parsig.ParSigError) and str(out[k]) == "invalid aggregated signature"
            assert not isinstance(plain[k], Exception)  # (aggregate_batch alone hands the wrong aggregate on)
        else:
            assert out[k].signature.hex() == expect[(d.slot, key)] == plain[k].signature.hex()
            assert out[k].share_idx == 0
    assert str(out[n]) == "require threshold signatures"
    assert "domain type not found" in str(out[n + 1])
    assert sorted(seen) == sorted((items[k][0].slot, items[k][1], expect[(items[k][0].slot, items[k][1])])
                                  for k in range(n) if k != bad_k)


def test_dkg_agg_and_verify_deposit_data(engine):
    data, shares, msgs = _deposit_inputs()
    want = dkg.agg_deposit_data_sigs(data, shares, msgs, engine)
    dkg.verify_deposit_aggregates(want, msgs, engine)
    assert dkg.agg_and_verify_deposit_data(data, shares, msgs, engine) == want
    assert dkg.agg_and_verify_deposit_data({}, shares, msgs, engine) == {}
    k0, k1 = list(data)[:2]
    # a bad partial: the same error, raised before any aggregate is checked
    bad = dict(data)
    bad[k0] = [data[k0][0], dkg.DKGPartial(data[k0][1].share_idx, data[k1][1].signature)] + data[k0][2:]
    for fn in (dkg.agg_deposit_data_sigs, dkg.agg_and_verify_deposit_data):
        with pytest.raises(dkg.DKGError, match="^invalid deposit data partial signature from peer$"):
            fn(bad, shares, msgs, engine)
    # a bad aggregate: DV k0 handed DV k1's partials, pubshares and message -- every partial
    # verifies against its pubshare, the aggregate does not verify under k0
    data2, shares2, msgs2 = dict(data), dict(shares), dict(msgs)
    data2[k0], shares2[k0], msgs2[k0] = data[k1], shares[k1], msgs[k1]
    with pytest.raises(dkg.DKGError, match="^invalid deposit data aggregated signature$"):
        dkg.verify_deposit_aggregates(dkg.agg_deposit_data_sigs(data2, shares2, msgs2, engine), msgs2, engine)
    with pytest.raises(dkg.DKGError, match="^invalid deposit data aggregated signature$"):
        dkg.agg_and_verify_deposit_data(data2, shares2, msgs2, engine)
