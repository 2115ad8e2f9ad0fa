"""DKG and cluster-lock signature work on the GPU.

  agg_deposit_data_sigs    dkg/dkg.go:545-601   verify every peer's deposit-data
                           partial against its pubshare, threshold-aggregate per DV
  verify_deposit_aggregates dkg/dkg.go:408-421  the aggregate of each DV verifies
                           under the DV's own public key
  agg_and_verify_deposit_data  both of the above; the aggregates are recombined
                           and verified under the DV keys in one launch
  agg_lock_hash_sig        dkg/dkg.go:428-478   verify every lock-hash partial,
                           then AggregateSignatures / AggregatePublicKeys
                           (plain sums: the multi-signature of all shares)
  verify_multi_signature   dkg/dkg.go:377       VerifyMultiSignature
  lock_verify_hashes       cluster/lock.go:117-131  the JSON lock hash == hashLock(l)
  lock_verify_signatures   cluster/lock.go:137-179  the lock's aggregate
                           signature: FastAggregateVerify over every pubshare,
                           over the hash the caller recomputed (not the JSON's)

and the producing halves, through the hardened signer (tbg_sign_ct):

  sign_deposit_data        dkg/dkg.go:505-542   a peer's deposit-data partials
  sign_lock_hash           dkg/dkg.go:480-503   a peer's lock-hash partials
  create_cluster_sign_deposit_data  cmd/createcluster.go:185-207
  agg_sign_lock_hash       cmd/createcluster.go:487-515  sign with every share, sum

Each step is one GPU submit over the whole ceremony (every DV and peer at
once) instead of the reference's per-partial loop: the deposit data runs as a
TBG_OP_VERIFY_AGGREGATE batch with threshold = the partial count (all must
verify, as the reference aborts on the first bad one), the lock hash as one
TBG_OP_VERIFY batch over a single message, and the sums / FastAggregateVerify
through tbg_sum_pubkeys, tbg_sum_sigs and tbg_fast_aggregate_verify.

Errors mirror the reference's strings; where the reference iterates a Go map
(random order) the first error in the caller's order is raised.  Out of scope
(host work off the signature path): the definition's operator ECDSA
signatures (Definition.VerifySignatures) and hashLock's SSZ walk -- the
caller passes the lock hash it recomputed; the JSON's lock_hash is only
compared against it.
"""
from __future__ import annotations

import base64
from dataclasses import dataclass

import numpy as np

from . import engine as eng
from . import tbls


class DKGError(Exception):
    pass


@dataclass(frozen=True)
class DKGPartial:
    """core.ParSignedData of the DKG exchange: the peer's share index (1-based)
    and its 96-byte partial signature."""
    share_idx: int
    signature: bytes


def _pk_ids(e, keys):
    present = [k for k in keys if k is not None]
    it = iter(tbls._pk_cache.ids_for(e, present))
    return [next(it) if k is not None else eng.NO_PUBKEY for k in keys]


def _decode_error(st: int) -> str:
    return "signature from core: uncompress sig: " + tbls._DECODE_ERRORS.get(st, str(st))


def _is_decode_error(st: int) -> bool:
    return st < 0 and st not in (eng.PS_ERR_PUBKEY, eng.PS_ERR_IDENTITY)


def agg_deposit_data_sigs(data, shares, msgs, engine=None) -> dict:
    """data {dv_pk48: [DKGPartial]}, shares {dv_pk48: {share_idx: pubshare48}},
    msgs {dv_pk48: deposit signing root}.  Returns {dv_pk48: 96-byte aggregate}."""
    e = tbls._engine(engine)
    dvs = list(data)
    if not dvs:
        return {}
    duty_first, sigs, ids, keys, mlist, thr = [0], [], [], [], [], []
    for dv in dvs:
        ps = list(data[dv])
        pub = shares.get(dv)
        for p in ps:
            sigs.append(bytes(p.signature))
            ids.append(p.share_idx)
            k = pub.get(p.share_idx) if pub is not None else None
            keys.append(tbls._raw(k, tbls.PublicKey) if k is not None else None)
        duty_first.append(duty_first[-1] + len(ps))
        mlist.append(bytes(msgs.get(dv, b"")))
        thr.append(len(ps))
    res = e.run(eng.OP_VERIFY_AGGREGATE, duty_first, b"".join(sigs), ids, msgs=mlist, duty_msg=np.arange(len(dvs)),
                pubkey_ids=_pk_ids(e, keys), duty_threshold=thr)
    out = {}
    for d, dv in enumerate(dvs):
        for j in range(duty_first[d], duty_first[d + 1]):
            st = int(res.partial_status[j])
            if _is_decode_error(st):
                raise DKGError(_decode_error(st))
            if dv not in shares:
                raise DKGError("invalid pubkey in deposit data partial signature from peer")
            if ids[j] not in shares[dv]:
                raise DKGError("invalid pubshare")
            if st != eng.PS_VALID:
                raise DKGError("invalid deposit data partial signature from peer")
        ds = int(res.duty_status[d])
        if ds != eng.DS_OK:
            raise DKGError(tbls._DUTY_ERRORS.get(ds, f"aggregate signatures: status {ds}"))
        out[dv] = bytes(res.agg[d])
    return out


def verify_deposit_aggregates(aggs, msgs, engine=None) -> None:
    """dkg.go:408-421: every DV's aggregate verifies under the DV key."""
    items = [(tbls.PublicKey(bytes(dv)), bytes(msgs[dv]), tbls.Signature(bytes(sig))) for dv, sig in aggs.items()]
    for r in tbls.verify_batch(items, engine):
        if isinstance(r, Exception):
            raise DKGError(str(r))
        if not r:
            raise DKGError("invalid deposit data aggregated signature")


def agg_and_verify_deposit_data(data, shares, msgs, engine=None) -> dict:
    """agg_deposit_data_sigs followed by verify_deposit_aggregates (dkg.go:593,
    then :408-421), without the second pass's decode of what the first has
    just encoded.  The partials are verified against their pubshares by the
    same launch as before (the reference aborts on the first bad partial:
    the errors and their order are agg_deposit_data_sigs'); then ONE
    OP_AGGREGATE_VERIFY launch over the verified partials recombines every
    DV's aggregate and checks it under the DV key.  Same return value and the
    same DKGError strings as the pair."""
    e = tbls._engine(engine)
    aggs = agg_deposit_data_sigs(data, shares, msgs, e)  # (raises on a bad partial)
    dvs = list(aggs)
    if not dvs:
        return {}
    duties = [{"partials": [tbls.PartialSignature(p.share_idx, tbls.Signature(bytes(p.signature)))
                            for p in data[dv]],
               "msg": bytes(msgs[dv]), "public_key": tbls.PublicKey(bytes(dv))} for dv in dvs]
    out = {}
    for dv, r in zip(dvs, tbls.aggregate_and_verify_batch(duties, e)):
        if isinstance(r, Exception):
            # (a DV key that does not decode fails the check as it does in verify_deposit_aggregates)
            if str(r) == "invalid aggregated signature" or str(r).startswith("verify aggregate: public key"):
                raise DKGError("invalid deposit data aggregated signature")
            raise DKGError(str(r))
        out[dv] = r.raw
    return out


def agg_lock_hash_sig(data, shares, lock_hash: bytes, engine=None):
    """data {dv_pk48: [DKGPartial]}, shares {dv_pk48: {share_idx: pubshare48}}.
    Returns (aggregate signature 96 B, aggregate public key 48 B)."""
    e = tbls._engine(engine)
    flat = [(dv, p) for dv, ps in data.items() for p in ps]
    if not flat:
        raise DKGError("bls aggregate Signatures: no signatures")
    keys = []
    for dv, p in flat:
        k = shares.get(dv, {}).get(p.share_idx)
        keys.append(tbls._raw(k, tbls.PublicKey) if k is not None else None)
    n = len(flat)
    pk_ids = _pk_ids(e, keys)
    sigs = b"".join(bytes(p.signature) for _, p in flat)
    res = e.run(eng.OP_VERIFY, np.arange(n + 1), sigs, np.zeros(n, np.uint8), msgs=[bytes(lock_hash)],
                duty_msg=np.zeros(n, np.int64), pubkey_ids=pk_ids)
    for j, (dv, p) in enumerate(flat):
        st = int(res.partial_status[j])
        if _is_decode_error(st):
            raise DKGError(_decode_error(st))
        if dv not in shares:
            raise DKGError("invalid pubkey in lock hash partial signature from peer")
        if p.share_idx not in shares[dv]:
            raise DKGError("invalid pubshare")
        if st != eng.PS_VALID:
            raise DKGError("invalid lock hash partial signature from peer")
    agg_sig, sst, _ = e.sum_sigs(sigs, [0, n])
    if int(sst[0]) != eng.DS_OK:
        raise DKGError("bls aggregate Signatures: " + tbls._DUTY_ERRORS.get(int(sst[0]), str(int(sst[0]))))
    agg_pk, pst = e.sum_pubkeys(pk_ids, [0, n])
    if int(pst[0]) != eng.DS_OK:
        raise DKGError("bls aggregate Public Keys: status %d" % int(pst[0]))
    return bytes(agg_sig[0]), bytes(agg_pk[0])


def verify_multi_signature(agg_pk48: bytes, msg: bytes, agg_sig96: bytes, engine=None) -> bool:
    """VerifyMultiSignature (dkg.go:377): CoreVerify of the aggregates."""
    r = tbls.verify_batch([(tbls.PublicKey(bytes(agg_pk48)), bytes(msg), tbls.Signature(bytes(agg_sig96)))], engine)[0]
    if isinstance(r, Exception):
        raise DKGError(str(r))
    return r


# ---- the producing halves: every signature a ceremony makes, through the
# hardened signer (tbls.sign_batch: tbg_sign_ct, fixed-schedule [sk]H(m), key
# material wiped) -- each one launch over every share at hand.
def _share_value(s) -> int:
    return s.value if isinstance(s, tbls.SecretKeyShare) else int(s)


def _sign_all(secrets, msgs, engine):
    """One hardened launch; the first failing item (caller's order) raises."""
    out = []
    for r in tbls.sign_batch(zip(secrets, msgs), engine):
        if isinstance(r, Exception):
            raise DKGError(str(r))
        out.append(r.raw)
    return out


def sign_deposit_data(shares, share_idx: int, msgs, engine=None) -> dict:
    """signDepositData (dkg/dkg.go:505-542): this peer's partial signature of
    every DV's deposit-data signing root.  shares {dv_pk48: secret share (int
    or SecretKeyShare)}, share_idx this peer's 1-based index, msgs {dv_pk48:
    signing root} (the roots are host work: deposit.GetMessageSigningRoot).
    Returns {dv_pk48: DKGPartial}.  A zero or out-of-range share raises
    DKGError("unmarshal secret: ...") (tblsconv.ShareToSecret)."""
    dvs = list(shares)
    for dv in dvs:
        if dv not in msgs:
            raise DKGError("deposit data signing root missing for a distributed validator")
    sigs = _sign_all([_share_value(shares[dv]) for dv in dvs], [bytes(msgs[dv]) for dv in dvs], engine)
    return {dv: DKGPartial(share_idx, sig) for dv, sig in zip(dvs, sigs)}


def sign_lock_hash(shares, share_idx: int, lock_hash: bytes, engine=None) -> dict:
    """signLockHash (dkg/dkg.go:480-503): this peer's partial signature of the
    lock hash with every share it holds -- one message, hashed once.
    Arguments and errors as sign_deposit_data.  Returns {dv_pk48: DKGPartial}."""
    dvs = list(shares)
    sigs = _sign_all([_share_value(shares[dv]) for dv in dvs], [bytes(lock_hash)] * len(dvs), engine)
    return {dv: DKGPartial(share_idx, sig) for dv, sig in zip(dvs, sigs)}


def create_cluster_sign_deposit_data(secrets, msgs, engine=None) -> list:
    """signDepositDatas of `charon create cluster` (cmd/createcluster.go:185-207):
    every validator SECRET signs its own deposit-data signing root.  secrets
    and msgs are parallel lists (the roots depend on the public keys, which
    tbls.secret_to_public_key_batch gives in one launch).  Returns the 96-byte
    signatures in the same order."""
    secrets, msgs = list(secrets), [bytes(m) for m in msgs]
    if len(secrets) != len(msgs):
        raise DKGError("one deposit data signing root per validator secret is needed")
    return _sign_all(secrets, msgs, engine)


def agg_sign_lock_hash(share_lists, lock_hash: bytes, engine=None) -> bytes:
    """aggSign (cmd/createcluster.go:487-515): the lock hash signed with every
    share of every validator (one hardened launch), then AggregateSignatures
    (the existing plain sum).  share_lists: one list of shares per validator.
    Returns the 96-byte aggregate."""
    flat = [_share_value(s) for shares in share_lists for s in shares]
    if not flat:
        raise DKGError("aggregate signatures: no signatures")
    e = tbls._engine(engine)
    sigs = _sign_all(flat, [bytes(lock_hash)] * len(flat), e)
    agg, st, _ = e.sum_sigs(b"".join(sigs), [0, len(sigs)])
    if int(st[0]) != eng.DS_OK:
        raise DKGError("aggregate signatures: " + tbls._DUTY_ERRORS.get(int(st[0]), str(int(st[0]))))
    return bytes(agg[0])


def create_cluster_tss(secrets, t: int, n: int, rng, engine=None, hardened=False, from_commitments=False,
                       device_split=False):
    """getTSSShares of `charon create cluster` (cmd/createcluster.go:250-270):
    every validator secret split t-of-n and its TSS.  One split on the host
    (integers), ONE sk_to_pk launch for every commitment and every pubshare
    (the shares are at hand here, so pubshare i is sk_to_pk(f(i))) and ONE
    key_from_bytes_batch that validates the pubshares and leaves them
    resident for the verifies that follow, instead of a SplitSecret + NewTSS
    pair per validator.  Returns (list of TSS, list of share lists).  Host
    integers and the test-only tbg_sk_to_pk: not side-channel safe, not for
    production keys (tbls.split_secret).  hardened=True forms every commitment
    and pubshare on the fixed schedule (tbg_sk_to_pk_ct; a zero or out-of-range
    scalar raises); the split itself stays on host integers and keeps the
    warning -- device_split (below) moves it to the device as well.

    from_commitments=True derives the pubshares the way NewTSS does: the
    scalar-multiplication launch forms the V*t commitments only (hardened or
    not as above), ONE Engine.eval_commitments launch evaluates them at
    1..n for all V*n pubshares, and no share value reaches the device.  Same
    return value, errors and residency.  Off by default: at large thresholds
    (170-of-255) Horner's rule over the commitments needs more group
    operations than one 256-bit ladder per share.

    device_split=True is the ceremony for keys that matter: ONE
    Engine.split_secret_ct call (tbg_split_secret_ct) evaluates every
    polynomial on the device in masks and forms every commitment and pubshare
    with the fixed-schedule ladder from the device copies -- no share travels
    back to the host between the split and its ladder -- then the same
    key_from_bytes_batch.  The coefficients are drawn from ``rng`` in the same
    order, so the return value equals the hardened=True path's.  A secret is
    sent as given: zero or >= r raises instead of being reduced mod r.  It
    implies hardened and does not combine with from_commitments."""
    e = tbls._engine(engine)
    if device_split:
        if from_commitments:
            raise tbls.TblsError("create cluster: device_split forms the pubshares itself (no from_commitments)")
        return _create_cluster_tss_device(list(secrets), t, n, rng, e)
    splits, polys = [], []
    for s in secrets:
        shares, poly = tbls._split_host(s, t, n, rng)
        splits.append(shares)
        polys.append(poly)
    if not splits:
        return [], []
    nd = len(polys)
    if from_commitments:
        commits = tbls._sk_to_pk([c for p in polys for c in p], e, hardened, "unmarshal secret")
        if hardened and any(s.value == 0 for sh in splits for s in sh):  # (what the fixed-schedule ladder refuses)
            raise tbls.TblsError("unmarshal secret: " + tbls._KS_ERRORS[eng.KS_ZERO])
        shares48 = []
        ids = list(range(1, n + 1))
        for pks, st, cst in tbls._eval_verifiers([commits[d * t:(d + 1) * t] for d in range(nd)], [ids] * nd, e):
            for pk, s in zip(pks, st):
                if s not in (eng.FV_OK, eng.FV_IDENTITY):  # (an identity pubshare is refused below, as without the keyword)
                    raise tbls._fv_error(s, cst)
                shares48.append(bytes(pk))
    else:
        scalars = [c for p in polys for c in p] + [s.value for sh in splits for s in sh]
        pks = tbls._sk_to_pk(scalars, e, hardened, "unmarshal secret")
        commits, shares48 = pks[:nd * t], pks[nd * t:]
    keys = tbls.key_from_bytes_batch(shares48, e)
    dvs = []
    for d in range(nd):
        pub = {}
        for i in range(n):
            k = keys[d * n + i]
            if isinstance(k, Exception):
                raise tbls.TblsError(str(k).replace("unmarshal pubkey", "unmarshal pubshare"))
            pub[i + 1] = k
        c = commits[d * t:(d + 1) * t]
        dvs.append(tbls.TSS(pub, n, t, tbls.PublicKey(c[0]), tuple(c)))
    return dvs, splits


def _create_cluster_tss_device(secrets, t, n, rng, e):
    """create_cluster_tss(device_split=True): the split, the commitments and the pubshares of every
    validator in one engine call."""
    if not (2 <= t <= n <= 255):
        raise tbls.TblsError("new Feldman VSS: need 2 <= t <= n <= 255")
    if not secrets:
        return [], []
    polys = [[int(s)] + [rng.randrange(1, tbls.R) for _ in range(t - 1)] for s in secrets]
    res = tbls._split_device(polys, n, e)
    for r in res:
        if isinstance(r, Exception):
            raise r
    keys = tbls.key_from_bytes_batch([pk for _, _, pks in res for pk in pks], e)
    dvs = []
    for d, (_, commits, _) in enumerate(res):
        pub = {}
        for i in range(n):
            k = keys[d * n + i]
            if isinstance(k, Exception):
                raise tbls.TblsError(str(k).replace("unmarshal pubkey", "unmarshal pubshare"))
            pub[i + 1] = k
        dvs.append(tbls.TSS(pub, n, t, tbls.PublicKey(commits[0]), tuple(commits)))
    return dvs, [shares for shares, _, _ in res]


def _lock_bytes(v) -> bytes:
    """Lock JSON byte fields: 0x-hex (v1.2+) or base64 (v1.0 / v1.1)."""
    if v is None:
        return b""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    if v.startswith("0x"):
        return bytes.fromhex(v[2:])
    return base64.b64decode(v)


def lock_verify_hashes(lock: dict, lock_hash: bytes) -> None:
    """The lock-hash half of Lock.VerifyHashes (cluster/lock.go:117-131): the
    JSON's lock_hash must equal the caller's recomputed hashLock(l)
    ("invalid lock hash").  The definition-hash half and the SSZ walk that
    recomputes both hashes are host work outside the BLS path."""
    lock_hash = bytes(lock_hash)
    if len(lock_hash) != 32:
        raise ValueError("lock_hash must be the 32-byte hashLock(l)")
    if _lock_bytes(lock.get("lock_hash")) != lock_hash:
        raise DKGError("invalid lock hash")


def lock_verify_signatures(lock: dict, lock_hash: bytes | None = None, engine=None) -> None:
    """Lock.VerifySignatures' aggregate check (cluster/lock.go:137-177) over a
    lock in its JSON form: cluster_definition.version, signature_aggregate,
    distributed_validators[].public_shares.

    The reference verifies the aggregate over hashLock(l), the hash it
    recomputes from the lock's fields (lock.go:166), never over the lock_hash
    the JSON carries.  hashLock's SSZ walk of the definition and validators is
    host work outside this path, so the CALLER supplies the hash it recomputed
    as `lock_hash`; without it this raises (ValueError) instead of trusting
    the file.  Like VerifySignatures this never reads the JSON's lock_hash:
    comparing it with the recomputed hash is VerifyHashes' job
    (lock_verify_hashes).  The definition's operator signatures
    (Definition.VerifySignatures, lock.go:138-140) are ECDSA work outside the
    BLS path and are not checked here."""
    version = lock.get("cluster_definition", {}).get("version", "")
    sig = _lock_bytes(lock.get("signature_aggregate"))
    if not sig:
        if version in ("v1.0.0", "v1.1.0"):
            return  # earlier versions did not populate SignatureAggregate
        raise DKGError("empty lock aggregate signature")
    if len(sig) != 96:  # (the reference's (*[96]byte) conversion would panic)
        raise DKGError("uncompress sig: invalid length")
    if lock_hash is None:
        raise ValueError("lock_verify_signatures needs the caller's recomputed hashLock(l) (cluster/lock.go:166); "
                         "the lock_hash field of the JSON is not trusted")
    lock_hash = bytes(lock_hash)
    if len(lock_hash) != 32:
        raise ValueError("lock_hash must be the 32-byte hashLock(l)")
    e = tbls._engine(engine)
    _, st, sst = e.sum_sigs(sig, [0, 1])  # tblsconv.SigFromBytes: decode only
    if _is_decode_error(int(sst[0])):
        raise DKGError("uncompress sig: " + tbls._DECODE_ERRORS.get(int(sst[0]), str(int(sst[0]))))
    raws = [_lock_bytes(s) for dv in lock.get("distributed_validators", []) for s in dv.get("public_shares", [])]
    keys = tbls.key_from_bytes_batch(raws, e)
    for k in keys:
        if isinstance(k, Exception):
            raise DKGError(str(k))
    ids = tbls._pk_cache.ids_for(e, raws)
    out = e.fast_aggregate_verify(ids, [0, len(ids)], [lock_hash], sig)
    if int(out[0]) != eng.PS_VALID:
        raise DKGError("invalid lock signature aggregate")
