"""The directed encodings of tests/edge_decode.py through the real engine (C
ABI, default configuration): every G2 encoding as one partial of its own
duty beside honest partials, once under TBG_OP_VERIFY and once under
TBG_OP_AGGREGATE, and the G1 list through the key upload; every status is the
oracle's.  The same lists run stage by stage in test_gpu_devcheck_decode.py
and on the CPU in test_decode_edges_host.py."""
import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import tbls_oracle as tb
from tests import edge_decode as ed
from tests.test_gpu_parity import DS_NAMES, PS_NAMES

pytestmark = pytest.mark.gpu

T, N = 3, 4
PS_OF_DEC = {ed.DEC_IDENTITY: "err_identity", ed.DEC_ERR_FLAGS: "err_flags", ed.DEC_ERR_FIELD: "err_field",
             ed.DEC_ERR_NOT_ON_CURVE: "err_curve", ed.DEC_ERR_SUBGROUP: "err_subgroup"}


@pytest.fixture(scope="module")
def engine():
    from charon_amd import engine as eng
    e = eng.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch(engine):
    """One honest 3-of-4 duty per G2 encoding; partial d % 4 of duty d is
    replaced by encoding d.  -> (ClusterBatch, sigs, entries, positions)."""
    from tools.workload import make_batch
    entries = ed.g2_entries()
    b = make_batch(engine, len(entries), T, N, seed=0xDEC0)
    sigs = np.array(b.sigs, dtype=np.uint8).reshape(-1, 96).copy()
    pos = [N * d + d % N for d in range(len(entries))]
    for k, e in zip(pos, entries):
        sigs[k] = np.frombuffer(e.data, dtype=np.uint8)
    return b, sigs, entries, pos


def test_every_g2_encoding_under_verify(engine, batch):
    from charon_amd import engine as eng
    b, sigs, entries, pos = batch
    res = engine.run(eng.OP_VERIFY, b.duty_first, sigs, b.identifiers, msgs=(b.msg_data, b.msg_off),
                     duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids)
    got = [PS_NAMES[int(s)] for s in res.partial_status]
    want = ["valid"] * len(got)
    for d, (k, e) in enumerate(zip(pos, entries)):
        dec, pt = ed.g2_class(e.data, True)
        if dec == ed.DEC_OK:  # a point of G2 that is no signature of this duty's message: the oracle's pairing check
            pk = bls.g1_decompress(bytes(b.pubshares[k]))
            want[k] = "valid" if tb.core_verify(pk, b.msgs[d], pt) else "invalid"
        else:
            want[k] = PS_OF_DEC[dec]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:8]
    assert {want[k] for k in pos} == {"invalid", "err_identity", "err_flags", "err_field", "err_curve", "err_subgroup"}


def test_every_g2_encoding_under_aggregate(engine, batch):
    from charon_amd import engine as eng
    b, sigs, entries, pos = batch
    res = engine.run(eng.OP_AGGREGATE, b.duty_first, sigs, b.identifiers)
    seen = set()
    for d, (k, e) in enumerate(zip(pos, entries)):
        dec, _ = ed.g2_class(e.data, True)
        got = DS_NAMES[int(res.duty_status[d])]
        if dec == ed.DEC_IDENTITY:
            want = "identity"
        elif dec != ed.DEC_OK:
            want = "decode"
        else:  # tbls.Aggregate over the four decoded points, whatever they sign
            parts = [(int(b.identifiers[N * d + j]), bls.g2_decompress(bytes(sigs[N * d + j]))) for j in range(N)]
            try:
                agg, want = bls.g2_compress(tb.combine_signatures(parts)), "ok"
            except tb.TblsError as err:
                want = "duplicate" if "duplicate" in str(err) else "too_few" if "insufficient" in str(err) else "identity"
            if want == "ok":
                assert bytes(res.agg[d]) == agg, (d, e.kind)
        assert got == want, (d, e.kind, e.branch, got, want)
        if want != "ok":
            assert not np.asarray(res.agg[d]).any(), (d, e.kind)
        seen.add(want)
    assert seen == {"ok", "identity", "decode"}


def test_g1_list_through_the_key_upload(engine):
    from charon_amd import tbls
    entries = ed.g1_entries()
    names = {0: "valid", 1: "identity", -1: "err_flags", -2: "err_field", -3: "err_curve", -4: "err_subgroup"}
    _, st = engine.load_pubkeys(b"".join(e.data for e in entries))
    want = [names[ed.g1_class(e.data)[0]] for e in entries]
    assert [names[s] for s in st.tolist()] == want
    assert set(want) == set(names.values())
    keys = tbls.key_from_bytes_batch([e.data for e in entries], engine)
    for k, w, e in zip(keys, want, entries):
        if w == "valid":
            assert isinstance(k, tbls.PublicKey), e.kind
        else:
            assert isinstance(k, tbls.TblsError) and str(k).startswith("unmarshal pubkey"), e.kind
