"""CPU tests of the Python layers over TBG_OP_AGGREGATE_VERIFY on a stub
engine: argument packing (one key id per duty, distinct messages sent once),
status-to-error mapping, that aggregate_batch / verify_deposit_aggregates
still make the calls they made before, and that the header stays plain C
with the codes Python mirrors."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from charon_amd import dkg, parsig, shard, signing, tbls
from charon_amd import engine as eng
from charon_amd.parsig import Duty, ParSignedData

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class StubEngine:
    """An engine that records its launches and returns canned duty statuses
    (queue of lists, one per run call; missing: every duty DS_OK)."""

    def __init__(self, duty_statuses=(), key_status=None):
        self.uid = -1000 - id(self) % 1000003  # (per-instance key cache)
        self.queue = [list(x) for x in duty_statuses]
        self.key_status = key_status or {}
        self.keys = []
        self.calls = []

    def load_pubkeys(self, pk48):
        raw = bytes(pk48)
        first = len(self.keys)
        new = [raw[i:i + 48] for i in range(0, len(raw), 48)]
        self.keys += new
        return first, np.array([self.key_status.get(k, 0) for k in new], dtype=np.int32)

    def run(self, op, duty_first, sigs, identifiers, **kw):
        duty_first = [int(x) for x in duty_first]
        nd, np_ = len(duty_first) - 1, duty_first[-1]
        assert len(bytes(sigs)) == 96 * np_ and len(identifiers) == np_
        self.calls.append(dict(op=op, duty_first=duty_first, identifiers=[int(i) for i in identifiers], sigs=bytes(sigs),
                               **{k: (v if k == "msgs" else [int(x) for x in v]) for k, v in kw.items()}))
        ds = self.queue.pop(0) if self.queue else [eng.DS_OK] * nd
        assert len(ds) == nd
        agg = np.zeros((nd, 96), dtype=np.uint8)
        for d in range(nd):
            agg[d] = 0xA0 + d if ds[d] == eng.DS_OK else 0
        ps = np.full(np_, eng.PS_VALID if op in (eng.OP_VERIFY, eng.OP_VERIFY_AGGREGATE) else eng.PS_NOT_VERIFIED,
                     dtype=np.int32)
        return eng.BatchResult(ps, np.array(ds, dtype=np.int32), agg)


def _ps(i, fill):
    return tbls.PartialSignature(i, tbls.Signature(bytes([fill]) * 96))


K1, K2, KBAD = bytes([1]) * 48, bytes([2]) * 48, bytes([3]) * 48


def test_packing_one_key_per_duty_and_distinct_messages():
    stub = StubEngine()
    duties = [dict(partials=[_ps(1, 0x11), _ps(2, 0x12), _ps(3, 0x13)], msg=b"m" * 32, public_key=tbls.PublicKey(K1)),
              dict(partials=[_ps(2, 0x21), _ps(4, 0x22)], msg=b"n" * 32, public_key=K2),
              dict(partials=[], msg=b"m" * 32, public_key=None),
              dict(partials=[_ps(1, 0x31), _ps(2, 0x32)], msg=b"m" * 32, public_key=K1)]
    out = tbls.aggregate_and_verify_batch(duties, stub)
    assert len(stub.calls) == 1
    c = stub.calls[0]
    assert c["op"] == eng.OP_AGGREGATE_VERIFY == 4
    assert c["duty_first"] == [0, 3, 5, 5, 7] and c["identifiers"] == [1, 2, 3, 2, 4, 1, 2]
    assert c["sigs"] == b"".join(bytes([f]) * 96 for f in (0x11, 0x12, 0x13, 0x21, 0x22, 0x31, 0x32))
    assert c["msgs"] == [b"m" * 32, b"n" * 32] and c["duty_msg"] == [0, 1, 0, 0]  # equal roots are sent once
    assert c["pubkey_ids"] == [0, 1, eng.NO_PUBKEY, 0] and stub.keys == [K1, K2]  # per DUTY; a key is resident once
    assert "duty_threshold" not in c
    assert [r.raw[0] for r in out] == [0xA0, 0xA1, 0xA2, 0xA3] and all(isinstance(r, tbls.Signature) for r in out)
    # the keys stay resident: a second call uploads nothing
    tbls.aggregate_and_verify_batch(duties[:1], stub)
    assert stub.keys == [K1, K2] and stub.calls[1]["pubkey_ids"] == [0]
    assert tbls.aggregate_and_verify_batch([], stub) == [] and len(stub.calls) == 2


def test_status_to_error_mapping():
    codes = [eng.DS_OK, eng.DS_AGG_INVALID, eng.DS_AGG_PUBKEY, eng.DS_AGG_PUBKEY, eng.DS_AGG_PUBKEY, eng.DS_AGG_TOO_FEW,
             eng.DS_AGG_DUPLICATE_ID, eng.DS_AGG_IDENTITY, eng.DS_DECODE, -99]
    stub = StubEngine([codes, [eng.DS_AGG_INVALID], [eng.DS_OK]],
                      key_status={KBAD: eng.PS_ERR_CURVE, K2: 1})
    keys = [K1, K1, None, KBAD, K2, K1, K1, K1, K1, K1]
    duties = [dict(partials=[_ps(1, 1), _ps(2, 2)], msg=b"r" * 32, public_key=k) for k in keys]
    out = tbls.aggregate_and_verify_batch(duties, stub)
    assert isinstance(out[0], tbls.Signature)
    assert [str(r) for r in out[1:]] == [
        "invalid aggregated signature",
        "verify aggregate: public key cannot be nil",
        "verify aggregate: public key point is not on the curve",
        "verify aggregate: public key is the identity",
        "aggregate signatures: insufficient partial signatures",
        "aggregate signatures: duplicate identifier",
        "aggregate signatures: identity signature",
        "uncompress sig",
        "aggregate signatures: status -99"]
    assert all(isinstance(r, tbls.TblsError) for r in out[1:])
    with pytest.raises(tbls.TblsError, match="^invalid aggregated signature$"):
        tbls.aggregate_and_verify([_ps(1, 1), _ps(2, 2)], b"r" * 32, K1, stub)
    assert tbls.aggregate_and_verify([_ps(1, 1), _ps(2, 2)], b"r" * 32, K1, stub).raw[0] == 0xA0


def _pd(idx, root=b"\x07" * 32, fill=0x40, domain=signing.DOMAIN_BEACON_ATTESTER, epoch=3):
    return ParSignedData(domain, epoch, root, bytes([fill + idx]) * 96, idx)


def test_aggregator_verified_batch_roots_keys_and_subscribers():
    spec = signing.Spec()
    stub = StubEngine([[eng.DS_OK, eng.DS_AGG_INVALID, eng.DS_DECODE, eng.DS_OK]])
    agg = parsig.Aggregator(2, stub)
    seen = []
    agg.subscribe(lambda d, pk, signed: seen.append((d.slot, pk, signed.signature[0], signed.share_idx)))
    hex1, hex2 = "0x" + K1.hex(), K2.hex()
    items = [(Duty(1, parsig.DUTY_ATTESTER), hex1, [_pd(1), _pd(2)]),
             (Duty(2, parsig.DUTY_ATTESTER), hex2, [_pd(1), _pd(3)]),
             (Duty(3, parsig.DUTY_ATTESTER), K1, [_pd(2), _pd(3)]),
             (Duty(4, parsig.DUTY_RANDAO), tbls.PublicKey(K2),
              [_pd(1, root=b"\x09" * 32, domain=signing.DOMAIN_RANDAO), _pd(4, root=b"\x09" * 32,
                                                                            domain=signing.DOMAIN_RANDAO)]),
             (Duty(5, parsig.DUTY_ATTESTER), hex1, [_pd(1)]),                                   # below threshold
             (Duty(6, parsig.DUTY_ATTESTER), hex1, [_pd(1, domain="NO_SUCH"), _pd(2, domain="NO_SUCH")]),
             (Duty(7, parsig.DUTY_ATTESTER), "0xzz", [_pd(1), _pd(2)]),
             (Duty(8, parsig.DUTY_ATTESTER), hex1, [_pd(1, root=b"\x01" * 31), _pd(2, root=b"\x01" * 31)])]
    out = agg.aggregate_verified_batch(items, spec)
    assert len(stub.calls) == 1  # one launch for the live items; host refusals never reach it
    c = stub.calls[0]
    assert c["op"] == eng.OP_AGGREGATE_VERIFY and c["duty_first"] == [0, 2, 4, 6, 8]
    assert c["identifiers"] == [1, 2, 1, 3, 2, 3, 1, 4]
    # the signing roots as signing.verify_batch forms them; three items share one
    att = signing.get_data_root(spec, signing.DOMAIN_BEACON_ATTESTER, 3, b"\x07" * 32)
    ran = signing.get_data_root(spec, signing.DOMAIN_RANDAO, 3, b"\x09" * 32)
    assert c["msgs"] == [att, ran] and c["duty_msg"] == [0, 0, 0, 1]
    assert [stub.keys[i] for i in c["pubkey_ids"]] == [K1, K2, K1, K2]
    assert out[0].signature[0] == 0xA0 and out[0].share_idx == 0 and out[3].signature[0] == 0xA3
    assert str(out[1]) == "invalid aggregated signature"
    assert str(out[2]) == "convert signature: uncompress sig"
    assert str(out[4]) == "require threshold signatures"
    assert "domain type not found" in str(out[5])
    assert str(out[6]) == "decode public key hex"
    assert str(out[7]) == "marshal signing data"
    assert all(isinstance(r, parsig.ParSigError) for r in out[1:3] + out[4:])
    assert seen == [(1, hex1, 0xA0, 0), (4, tbls.PublicKey(K2), 0xA3, 0)]  # only verified aggregates


def test_aggregate_batch_still_makes_its_call():
    stub = StubEngine()
    agg = parsig.Aggregator(2, stub)
    out = agg.aggregate_batch([(Duty(1, parsig.DUTY_ATTESTER), "dv", [_pd(1), _pd(2)])])
    assert out[0].signature[0] == 0xA0
    assert [c["op"] for c in stub.calls] == [eng.OP_AGGREGATE] and set(stub.calls[0]) == {"op", "duty_first",
                                                                                             "identifiers", "sigs"}
    assert stub.keys == []


def test_dkg_pair_unchanged_and_the_fused_form():
    dv1, dv2 = K1, K2
    data = {dv1: [dkg.DKGPartial(1, bytes([0x51]) * 96), dkg.DKGPartial(2, bytes([0x52]) * 96)],
            dv2: [dkg.DKGPartial(1, bytes([0x61]) * 96), dkg.DKGPartial(3, bytes([0x63]) * 96)]}
    shares = {dv1: {1: bytes([0x11]) * 48, 2: bytes([0x12]) * 48}, dv2: {1: bytes([0x21]) * 48, 3: bytes([0x23]) * 48}}
    msgs = {dv1: b"a" * 32, dv2: b"b" * 32}
    # the existing pair: one OP_VERIFY_AGGREGATE launch, then one OP_VERIFY launch of the aggregates
    stub = StubEngine()
    aggs = dkg.agg_deposit_data_sigs(data, shares, msgs, stub)
    dkg.verify_deposit_aggregates(aggs, msgs, stub)
    assert [c["op"] for c in stub.calls] == [eng.OP_VERIFY_AGGREGATE, eng.OP_VERIFY]
    assert stub.calls[0]["duty_threshold"] == [2, 2] and len(stub.calls[0]["pubkey_ids"]) == 4
    assert stub.calls[1]["duty_first"] == [0, 1, 2] and stub.calls[1]["sigs"] == aggs[dv1] + aggs[dv2]
    # the fused form: the same first launch, then ONE op-4 launch over the verified partials, DV keys per duty
    stub = StubEngine()
    got = dkg.agg_and_verify_deposit_data(data, shares, msgs, stub)
    assert got == aggs
    assert [c["op"] for c in stub.calls] == [eng.OP_VERIFY_AGGREGATE, eng.OP_AGGREGATE_VERIFY]
    c = stub.calls[1]
    assert c["duty_first"] == [0, 2, 4] and c["identifiers"] == [1, 2, 1, 3] and c["msgs"] == [b"a" * 32, b"b" * 32]
    assert [stub.keys[i] for i in c["pubkey_ids"]] == [dv1, dv2] and c["sigs"] == stub.calls[0]["sigs"]
    # a failed aggregate check, and a DV key that does not decode, read as the pair's error
    for codes, ks in (([eng.DS_OK, eng.DS_AGG_INVALID], None), ([eng.DS_AGG_PUBKEY, eng.DS_OK], {dv1: eng.PS_ERR_FIELD})):
        stub = StubEngine([[eng.DS_OK, eng.DS_OK], codes], key_status=ks)
        with pytest.raises(dkg.DKGError, match="^invalid deposit data aggregated signature$"):
            dkg.agg_and_verify_deposit_data(data, shares, msgs, stub)
    stub = StubEngine([[eng.DS_OK, eng.DS_AGG_DUPLICATE_ID]])
    with pytest.raises(dkg.DKGError, match="^aggregate signatures: duplicate identifier$"):
        dkg.agg_and_verify_deposit_data(data, shares, msgs, stub)
    assert len(stub.calls) == 1  # (the first launch's error: nothing else runs)


def test_engine_checks_the_per_duty_key_count_before_any_native_call():
    e = object.__new__(eng.Engine)  # (no library, no device: _batch is host code)
    kw = dict(msgs=[b"m"], duty_msg=[0, 0])
    with pytest.raises(ValueError, match="one id per duty"):
        eng.Engine._batch(e, eng.OP_AGGREGATE_VERIFY, [0, 2, 4], bytes(96 * 4), [1, 2, 1, 2], pubkey_ids=[0, 1, 2, 3], **kw)
    b, keep, nd, np_ = eng.Engine._batch(e, eng.OP_AGGREGATE_VERIFY, [0, 2, 4], bytes(96 * 4), [1, 2, 1, 2],
                                         pubkey_ids=[7, 8], **kw)
    assert (b.op, nd, np_, b.n_msgs) == (4, 2, 4, 1) and not b.duty_threshold
    # the per-partial ops keep their layout
    b, _, _, _ = eng.Engine._batch(e, eng.OP_VERIFY, [0, 2, 4], bytes(96 * 4), [1, 2, 1, 2], pubkey_ids=[0, 1, 2, 3], **kw)
    assert b.op == 1


def test_shard_cuts_per_duty_keys_at_the_duty_offset():
    duty_first = [0, 3, 3, 7, 9]
    args = dict(duty_first=duty_first, sigs=np.zeros((9, 96), np.uint8), identifiers=np.arange(9) % 4 + 1)
    sb = shard.sub_batch(1, 3, pubkey_ids=np.array([10, 11, 12, 13]), key_per_duty=True, **args)
    assert sb.pubkey_ids.tolist() == [11, 12] and (sb.p0, sb.p1) == (3, 7)
    sb = shard.sub_batch(1, 3, pubkey_ids=np.arange(100, 109), **args)
    assert sb.pubkey_ids.tolist() == [103, 104, 105, 106]


def test_header_is_plain_c_and_python_mirrors_its_codes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None and os.path.exists("/opt/rocm/llvm/bin/clang"):
        cc = "/opt/rocm/llvm/bin/clang"
    assert cc, "no C compiler"
    src = tmp_path / "aggver_abi.c"
    src.write_text('#include "tbls_gpu.h"\n'
                   "int op_is_4[TBG_OP_AGGREGATE_VERIFY == 4 ? 1 : -1];\n"
                   "int codes[(TBG_DS_AGG_INVALID == -26 && TBG_DS_AGG_PUBKEY == -27) ? 1 : -1];\n"
                   "tbg_batch b = {TBG_OP_AGGREGATE_VERIFY, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};\n")
    r = subprocess.run([cc, "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "include", "tbls_gpu.h")).read()
    ds = dict(re.findall(r"#define (TBG_DS_\w+) \(?(-?\d+)\)?", text))
    assert (int(ds["TBG_DS_AGG_INVALID"]), int(ds["TBG_DS_AGG_PUBKEY"])) == (eng.DS_AGG_INVALID, eng.DS_AGG_PUBKEY)
    assert len(set(ds.values())) == len(ds)  # no duty code is reused
    assert re.search(r"TBG_OP_AGGREGATE_VERIFY = (\d+)", text).group(1) == str(eng.OP_AGGREGATE_VERIFY)
