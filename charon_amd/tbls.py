"""Host-side mirror of Charon's ``tbls`` package (reference tbls/tss.go) on the
MI355X engine.

Same names, argument meaning and error behaviour as the Go API, so that a
parity test reads like ``tbls/tss_test.go``:

  verify(pk, msg, sig) -> bool                         tss.go:190-197
  aggregate(partial_sigs) -> Signature                 tss.go:142-149
  verify_and_aggregate(tss, partial_sigs, msg)         tss.go:153-187
  TSS(pubshares, num_shares, threshold, public_key)    tss.go:62-116
  new_tss(commitments, num_shares) -> TSS              tss.go:95-116, 293-325 (NewTSS, getPubShare)
  split_secret / combine_shares / generate_tss         tss.go:256-290, 220-253, 120-139
  sign / partial_sign (test-only, not side-channel safe unless
  hardened=True)                                        tss.go:200-217

plus the batch entry points the batch-aware call sites use:

  verify_batch(items) -> list[bool | TblsError]
  verify_and_aggregate_batch(duties) -> list[(Signature, signers) | TblsError]
  aggregate_batch(duties) -> list[Signature | TblsError]
  aggregate_and_verify_batch(duties) -> list[Signature | TblsError]
  new_tss_batch(verifiers, n) / pubshares_from_commitments_batch(verifiers, n)
  feldman_verify_batch(items) -> list[bool | TblsError]

and the hardened signer (tbg_sign_ct / tbg_sk_to_pk_ct: fixed-schedule scalar
multiplication, key material wiped), for the keys of a create-cluster or DKG
ceremony:

  sign_batch(items) / partial_sign_batch(items) -> list[Signature | PartialSignature | TblsError]
  secret_to_public_key_batch(secrets) -> list[PublicKey | TblsError]

Keys and signatures are carried as their wire encodings (48-byte G1 /
96-byte G2, ZCash-compressed); decoding, hashing, pairing and Lagrange
recombination all run on the GPU.  Errors follow the Go strings:
"uncompress sig" (tblsconv.go:128), "verify signature" (tss.go:193),
"aggregate signatures" (tss.go:145), "insufficient signatures" (tss.go:155),
"insufficient valid signatures" (tss.go:177).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import engine as eng


class TblsError(Exception):
    """Mirror of the Go ``error`` values returned by tbls / tblsconv."""


@dataclass(frozen=True)
class PublicKey:
    """bls_sig.PublicKey (48-byte compressed G1)."""
    raw: bytes

    def __post_init__(self):
        if len(self.raw) != 48:
            raise TblsError("unmarshal pubkey: invalid length")


@dataclass(frozen=True)
class Signature:
    """bls_sig.Signature (96-byte compressed G2)."""
    raw: bytes

    def __post_init__(self):
        if len(self.raw) != 96:
            raise TblsError("uncompress sig: invalid length")


@dataclass(frozen=True)
class PartialSignature:
    """bls_sig.PartialSignature{Identifier byte; Signature G2}."""
    identifier: int
    signature: Signature

    def __post_init__(self):
        if not 0 <= self.identifier <= 255:
            raise TblsError("identifier must fit a byte")


@dataclass
class TSS:
    """tbls.TSS: pubshares by share index, n, t, group public key."""
    pubshares: dict
    num_shares: int
    threshold: int
    public_key: PublicKey | None = None
    commitments: tuple = ()  # the Feldman commitments [a_j] g1 (48 bytes each) when built by generate_tss

    def public_share(self, share_idx: int):
        return self.pubshares.get(share_idx)

    def public_shares(self):
        return self.pubshares


_DECODE_ERRORS = {
    eng.PS_ERR_FLAGS: "compressed flag must be set / invalid infinity encoding",
    eng.PS_ERR_FIELD: "invalid bytes - not in field",
    eng.PS_ERR_CURVE: "point is not on the curve",
    eng.PS_ERR_SUBGROUP: "point is not in correct subgroup",
}
_DUTY_ERRORS = {
    eng.DS_INSUFFICIENT: "insufficient signatures",
    eng.DS_INSUFFICIENT_VALID: "insufficient valid signatures",
    eng.DS_AGG_TOO_FEW: "aggregate signatures: insufficient partial signatures",
    eng.DS_AGG_DUPLICATE_ID: "aggregate signatures: duplicate identifier",
    eng.DS_AGG_IDENTITY: "aggregate signatures: identity signature",
    eng.DS_DECODE: "uncompress sig",
}


class _PubkeyCache:
    """Resident pubkey ids per engine (the startup pubshare upload of
    app/app.go:334-376 happens here, lazily).  Every distinct key is uploaded
    (decoded into the device table) once per engine; its table id and decode
    status are kept, so repeated lookups never grow the device table."""

    def __init__(self):
        self.ids = {}
        self.status = {}

    def _load(self, e: eng.Engine, keys):
        """Upload the keys not resident yet; returns (id cache, status cache)."""
        cache = self.ids.setdefault(e.uid, {})
        stat = self.status.setdefault(e.uid, {})
        missing = [k for k in dict.fromkeys(keys) if k not in cache]
        if missing:
            first, st = e.load_pubkeys(b"".join(missing))
            for i, (k, s) in enumerate(zip(missing, st.tolist())):
                cache[k] = first + i
                stat[k] = int(s)
        return cache, stat

    def ids_for(self, e: eng.Engine, keys):
        cache, _ = self._load(e, keys)
        return [cache[k] for k in keys]

    def statuses_for(self, e: eng.Engine, keys):
        _, stat = self._load(e, keys)
        return [stat[k] for k in keys]


_pk_cache = _PubkeyCache()

_PK_ERRORS = {
    1: "public key is the identity",
    eng.PS_ERR_FLAGS: "compressed flag must be set / invalid infinity encoding",
    eng.PS_ERR_FIELD: "invalid bytes - not in field",
    eng.PS_ERR_CURVE: "point is not on the curve",
    eng.PS_ERR_SUBGROUP: "point is not in correct subgroup",
}


def key_from_bytes_batch(raws, engine=None):
    """tblsconv.KeyFromBytes (tblsconv.go:30-37) for many 48-byte keys at once:
    decoded and validated on the GPU (flags, field, curve, subgroup; the
    identity is refused as a public key), and made resident.  Per key returns
    a PublicKey or TblsError("unmarshal pubkey: ...")."""
    raws = [bytes(r) for r in raws]
    if not raws:
        return []
    e = _engine(engine)
    for r in raws:
        if len(r) != 48:
            raise TblsError("unmarshal pubkey: invalid length")
    out = []
    for r, s in zip(raws, _pk_cache.statuses_for(e, raws)):  # only keys not resident yet are uploaded
        if s == 0:
            out.append(PublicKey(r))
        else:
            out.append(TblsError("unmarshal pubkey: " + _PK_ERRORS.get(s, str(s))))
    return out


def wire_pubshares(validators, engine=None):
    """Startup pubshare wiring of app/app.go:334-376 (wireCoreWorkflow):
    ``validators`` maps a DV public key to its list of 48-byte pubshares (share
    index = list position + 1).  Every pubshare of the cluster is decoded in
    ONE GPU batch and stays resident for the verifies that follow; the first
    bad pubshare, in the reference's loop order, aborts with its
    KeyFromBytes error (app.go:347-350).  Returns {dv: {share_idx: PublicKey}}."""
    flat = [(dv, i, bytes(b)) for dv, shares in validators.items() for i, b in enumerate(shares)]
    keys = key_from_bytes_batch([b for _, _, b in flat], engine)
    out = {dv: {} for dv in validators}
    for (dv, i, _), k in zip(flat, keys):
        if isinstance(k, TblsError):
            raise k
        out[dv][i + 1] = k
    return out


def _engine(e):
    return e if e is not None else eng.default_engine()


def _raw(x, cls):
    if isinstance(x, cls):
        return x.raw
    return bytes(x)


# --------------------------------------------------------------------- batch API
def _distinct_msgs(msgs):
    """(distinct messages in first-seen order, item -> message index): equal
    message bytes are sent -- and hashed to G2 -- once, and a fused level 0
    pairs one key sum per distinct message (tbg_config.l0_msg_share).  A
    parsigex set is N items over ONE root."""
    index = {}
    item_msg = np.fromiter((index.setdefault(m, len(index)) for m in msgs), dtype=np.uint32, count=len(msgs))
    return list(index), item_msg


def verify_batch(items, engine=None):
    """items: iterable of (pk, msg, sig).  Returns a list with True/False per
    item, or a TblsError for items whose encodings do not decode."""
    items = list(items)
    if not items:
        return []
    e = _engine(engine)
    pks = [_raw(pk, PublicKey) if pk is not None else None for pk, _, _ in items]
    present = [p for p in pks if p is not None]
    ids_present = iter(_pk_cache.ids_for(e, present))
    pk_ids = [next(ids_present) if p is not None else eng.NO_PUBKEY for p in pks]
    msgs, item_msg = _distinct_msgs([bytes(m) for _, m, _ in items])
    sigs = b"".join(_raw(s, Signature) for _, _, s in items)
    n = len(items)
    res = e.run(eng.OP_VERIFY, np.arange(n + 1), sigs, np.zeros(n, np.uint8), msgs=msgs, duty_msg=item_msg,
                pubkey_ids=pk_ids)
    out = []
    for st in res.partial_status.tolist():
        if st == eng.PS_VALID:
            out.append(True)
        elif st in (eng.PS_INVALID, eng.PS_ERR_IDENTITY, eng.PS_ERR_PUBKEY):
            out.append(False)
        else:
            out.append(TblsError("uncompress sig: " + _DECODE_ERRORS.get(st, str(st))))
    return out


def verify_sets_batch(sets, engine=None):
    """sets: list of lists of (pk, msg, sig).  Returns True per set whose
    every item verifies, else False -- all or nothing, the meaning of a
    receive path that drops a whole set on its first failing item (reference
    core/parsigex/parsigex.go:101-107).  One set launch (tbg_submit_sets): a
    failed set is not narrowed to its bad item, and a set with an item that
    does not decode (SS_ERROR) is False too, since it is dropped either way.
    An empty set is True."""
    sets = [list(s) for s in sets]
    items = [it for s in sets for it in s]
    if not items:
        return [True] * len(sets)
    e = _engine(engine)
    pks = [_raw(pk, PublicKey) if pk is not None else None for pk, _, _ in items]
    present = [p for p in pks if p is not None]
    ids_present = iter(_pk_cache.ids_for(e, present))
    pk_ids = [next(ids_present) if p is not None else eng.NO_PUBKEY for p in pks]
    msgs, item_msg = _distinct_msgs([bytes(m) for _, m, _ in items])
    sigs = b"".join(_raw(s, Signature) for _, _, s in items)
    n = len(items)
    set_first = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    res = e.run_sets(set_first, np.arange(n + 1), sigs, np.zeros(n, np.uint8), msgs=msgs, duty_msg=item_msg,
                     pubkey_ids=pk_ids)
    return [st == eng.SS_VALID for st in res.set_status.tolist()]


def _duty_arrays(duties, with_msg):
    duty_first = [0]
    sigs, ids, msgs, thr, pk_keys = [], [], [], [], []
    for d in duties:
        partials = d["partials"]
        for p in partials:
            sigs.append(_raw(p.signature, Signature))
            ids.append(p.identifier)
            if with_msg:
                pk = d["tss"].public_share(int(p.identifier))
                pk_keys.append(_raw(pk, PublicKey) if pk is not None else None)
        duty_first.append(duty_first[-1] + len(partials))
        if with_msg:
            msgs.append(bytes(d["msg"]))
            thr.append(d["tss"].threshold)
    return duty_first, b"".join(sigs), ids, msgs, thr, pk_keys


def verify_and_aggregate_batch(duties, engine=None):
    """duties: iterable of dicts {tss, partials, msg}.  Per duty returns
    (Signature, signers) or a TblsError, like tbls.VerifyAndAggregate."""
    duties = list(duties)
    if not duties:
        return []
    e = _engine(engine)
    duty_first, sigs, ids, msgs, thr, pk_keys = _duty_arrays(duties, True)
    present = [k for k in pk_keys if k is not None]
    it = iter(_pk_cache.ids_for(e, present))
    pk_ids = [next(it) if k is not None else eng.NO_PUBKEY for k in pk_keys]
    res = e.run(eng.OP_VERIFY_AGGREGATE, duty_first, sigs, ids, msgs=msgs, duty_msg=np.arange(len(duties)),
                pubkey_ids=pk_ids, duty_threshold=thr)
    out = []
    for d, ds in enumerate(res.duty_status.tolist()):
        lo, hi = duty_first[d], duty_first[d + 1]
        ps = res.partial_status[lo:hi].tolist()
        if ds == eng.DS_OK:
            signers = [ids[lo + j] for j, s in enumerate(ps) if s == eng.PS_VALID]
            out.append((Signature(bytes(res.agg[d])), signers))
        else:
            out.append(TblsError(_DUTY_ERRORS.get(ds, f"aggregate signatures: status {ds}")))
    return out


def aggregate_batch(duties, engine=None):
    """duties: iterable of lists of PartialSignature.  Per duty returns the
    aggregate Signature or a TblsError, like tbls.Aggregate."""
    duties = [{"partials": list(p)} for p in duties]
    if not duties:
        return []
    e = _engine(engine)
    duty_first, sigs, ids, _, _, _ = _duty_arrays(duties, False)
    res = e.run(eng.OP_AGGREGATE, duty_first, sigs, ids)
    out = []
    for d, ds in enumerate(res.duty_status.tolist()):
        if ds == eng.DS_OK:
            out.append(Signature(bytes(res.agg[d])))
        else:
            out.append(TblsError(_DUTY_ERRORS.get(ds, f"aggregate signatures: status {ds}")))
    return out


def aggregate_and_verify_batch(duties, engine=None):
    """duties: iterable of dicts {partials, msg, public_key}.  Per duty:
    tbls.Aggregate over all its partials, then tbls.Verify of the aggregate
    under the duty's group public key -- in ONE launch (OP_AGGREGATE_VERIFY:
    the aggregate is checked in the form the recombination leaves it in, with
    no second decode).  Returns the aggregate Signature, or a TblsError: the
    strings of aggregate_batch when the combination fails, "invalid aggregated
    signature" when the aggregate does not verify, "verify aggregate: public
    key ..." when the duty's key is missing or does not decode.  Equal
    messages are hashed once; group keys stay resident like pubshares."""
    duties = list(duties)
    if not duties:
        return []
    e = _engine(engine)
    duty_first, sigs, ids, _, _, _ = _duty_arrays(duties, False)
    keys = [_raw(d["public_key"], PublicKey) if d.get("public_key") is not None else None for d in duties]
    present = [k for k in keys if k is not None]
    it = iter(_pk_cache.ids_for(e, present))
    pk_ids = [next(it) if k is not None else eng.NO_PUBKEY for k in keys]
    msgs, duty_msg = _distinct_msgs([bytes(d["msg"]) for d in duties])
    res = e.run(eng.OP_AGGREGATE_VERIFY, duty_first, sigs, ids, msgs=msgs, duty_msg=duty_msg, pubkey_ids=pk_ids)
    out = []
    for d, ds in enumerate(res.duty_status.tolist()):
        if ds == eng.DS_OK:
            out.append(Signature(bytes(res.agg[d])))
        elif ds == eng.DS_AGG_INVALID:
            out.append(TblsError("invalid aggregated signature"))
        elif ds == eng.DS_AGG_PUBKEY:
            if keys[d] is None:
                why = "cannot be nil"
            else:
                st = _pk_cache.statuses_for(e, [keys[d]])[0]
                why = _PK_ERRORS.get(st, f"status {st}")
                why = why[len("public key "):] if why.startswith("public key ") else why
            out.append(TblsError("verify aggregate: public key " + why))
        else:
            out.append(TblsError(_DUTY_ERRORS.get(ds, f"aggregate signatures: status {ds}")))
    return out


# ------------------------------------------------------------ Go-API mirror
def aggregate_and_verify(partial_sigs, msg: bytes, public_key, engine=None) -> Signature:
    """tbls.Aggregate, then tbls.Verify of the result under the group key (what
    the DKG and the sigagg tests do with two calls), in one launch.  Raises the
    TblsError of aggregate_and_verify_batch."""
    r = aggregate_and_verify_batch([{"partials": list(partial_sigs), "msg": msg, "public_key": public_key}],
                                   engine)[0]
    if isinstance(r, Exception):
        raise r
    return r


def verify(pk, msg: bytes, sig, engine=None) -> bool:
    """tbls.Verify: (bool, error).  Decode failures raise TblsError."""
    if pk is None:
        raise TblsError("verify signature: public key cannot be nil")
    r = verify_batch([(pk, msg, sig)], engine)[0]
    if isinstance(r, Exception):
        raise r
    return r


def aggregate(partial_sigs, engine=None) -> Signature:
    """tbls.Aggregate (CombineSignatures over all partials)."""
    r = aggregate_batch([partial_sigs], engine)[0]
    if isinstance(r, Exception):
        raise r
    return r


def verify_and_aggregate(tss: TSS, partial_sigs, msg: bytes, engine=None):
    """tbls.VerifyAndAggregate: returns (Signature, signers)."""
    partial_sigs = list(partial_sigs)
    if len(partial_sigs) < tss.threshold:
        raise TblsError("insufficient signatures")
    r = verify_and_aggregate_batch([{"tss": tss, "partials": partial_sigs, "msg": msg}], engine)[0]
    if isinstance(r, Exception):
        raise r
    return r


# ------------------------------------------------- the key side of tss.go (test clusters)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # the group order


@dataclass(frozen=True)
class SecretKeyShare:
    """bls_sig.SecretKeyShare{identifier byte; value}: f(identifier) mod r."""
    identifier: int
    value: int

    def __post_init__(self):
        if not 1 <= self.identifier <= 255:
            raise TblsError("share identifier must be 1..255")


def _sk32(v: int) -> bytes:
    return (int(v) % R).to_bytes(32, "big")


def split_secret(secret: int, t: int, n: int, rng, engine=None, hardened=False):
    """tbls.SplitSecret (tss.go:256-290): n shares f(1..n) of f(x) = secret +
    a_1 x + ... + a_(t-1) x^(t-1) mod r, the a_j drawn from ``rng``
    (``randrange``), and the t Feldman commitments [a_j] g1 (48 bytes each,
    through Engine.sk_to_pk).  Host integers: NOT side-channel safe, and the
    engine's sk_to_pk is the test-only double-and-add of tbg_sk_to_pk -- not
    for production keys.  hardened=True forms the commitments on the fixed
    schedule (tbg_sk_to_pk_ct); the polynomial is still split here on host
    integers and keeps this warning.  A key that matters is split by
    split_secret_batch (tbg_split_secret_ct), which evaluates the polynomial
    on the device in masks and gives the same shares for the same rng."""
    shares, poly = _split_host(secret, t, n, rng)
    return shares, _sk_to_pk(poly, engine, hardened, "marshalling Secret Key")


def _split_host(secret: int, t: int, n: int, rng):
    """The integer half of split_secret: (shares, polynomial coefficients)."""
    if not (2 <= t <= n <= 255):
        raise TblsError("new Feldman VSS: need 2 <= t <= n <= 255")
    secret = int(secret) % R
    if secret == 0:
        raise TblsError("convert to scaler: zero secret")
    poly = [secret] + [rng.randrange(1, R) for _ in range(t - 1)]
    shares = []
    for i in range(1, n + 1):
        acc = 0
        for c in reversed(poly):
            acc = (acc * i + c) % R
        shares.append(SecretKeyShare(i, acc))
    return shares, poly


def _sk_to_pk(scalars, engine, hardened, what):
    """48-byte public keys of integer scalars: Engine.sk_to_pk, or with
    hardened the fixed-schedule Engine.sk_to_pk_ct (a zero or out-of-range
    scalar raises)."""
    e = _engine(engine)
    if not hardened:
        return [bytes(k) for k in e.sk_to_pk(b"".join(_sk32(v) for v in scalars))]
    pks, st = e.sk_to_pk_ct(b"".join(_sk32_exact(v) for v in scalars))
    for s in st.tolist():
        if s != eng.KS_OK:
            raise TblsError(what + ": " + _KS_ERRORS.get(s, f"status {s}"))
    return [bytes(k) for k in pks]


def tss_from_shares(shares, commits, engine=None, hardened=False) -> TSS:
    """The TSS of a split whose scalar shares are at hand: pubshare i is
    sk_to_pk(f(i)) (what NewTSS's sum over the commitments evaluates to), the
    group key is C_0 and the threshold is the number of commitments.  For
    callers that hold the shares (GenerateTSS, create cluster); a caller with
    the commitments alone uses new_tss (tbls.NewTSS proper), which reaches
    the same pubshares without any share.  Test-only scalar multiplication
    unless hardened, see split_secret."""
    shares = list(shares)
    commits = [bytes(c) for c in commits]
    pks = _sk_to_pk([s.value for s in shares], engine, hardened, "unmarshal secret")
    ident = bytes([0xC0]) + bytes(47)
    if commits[0] == ident:
        raise TblsError("unmarshal pubkey: " + _PK_ERRORS[1])
    pub = {}
    for s, pk in zip(shares, pks):
        if bytes(pk) == ident:
            raise TblsError("unmarshal pubshare: " + _PK_ERRORS[1])
        pub[s.identifier] = PublicKey(bytes(pk))
    return TSS(pub, len(shares), len(commits), PublicKey(commits[0]), tuple(commits))


# ---- tbls.NewTSS: the TSS from the Feldman verifier alone (tss.go:95-116, getPubShare :293-325)
_IDENT48 = bytes([0xC0]) + bytes(47)


def _verifier_bytes(commitments):
    """The 48-byte encodings of one verifier's commitments (PublicKey or bytes each)."""
    cs = [_raw(c, PublicKey) for c in commitments]
    if not cs:
        raise TblsError("new TSS: the verifier has no commitments")
    for c in cs:
        if len(c) != 48:
            raise TblsError("unmarshal pubkey: invalid length")
    return cs


def _eval_verifiers(verifiers, ids, e):
    """ONE Engine.eval_commitments launch: verifier v at every identifier of
    ids[v].  Per verifier returns (outputs, eval statuses, commitment statuses)."""
    first = np.concatenate([[0], np.cumsum([len(v) for v in verifiers])]).astype(np.uint32)
    eval_poly = [v for v, iv in enumerate(ids) for _ in iv]
    out, st, cst = e.eval_commitments(b"".join(c for v in verifiers for c in v), first, eval_poly,
                                      [i for iv in ids for i in iv])
    res, k = [], 0
    for v, iv in enumerate(ids):
        res.append((out[k:k + len(iv)], st[k:k + len(iv)].tolist(), cst[first[v]:first[v + 1]].tolist()))
        k += len(iv)
    return res


def _fv_error(st, commit_status):
    """The TblsError of a failed evaluation (FV_*), the strings of NewTSS."""
    if st == eng.FV_COMMIT:
        code = next(c for c in commit_status if c not in (0, 1))
        return TblsError("unmarshal commitment: " + _PK_ERRORS.get(code, str(code)))
    if st == eng.FV_KEY_IDENTITY:
        return TblsError("unmarshal pubkey: " + _PK_ERRORS[1])
    if st == eng.FV_IDENTITY:
        return TblsError("unmarshal pubshare: " + _PK_ERRORS[1])
    return TblsError("share identifier must be 1..255" if st == eng.FV_ID else f"evaluate commitments: status {st}")


def pubshares_from_commitments_batch(verifiers, num_shares: int, engine=None):
    """getPubShare (tss.go:293-325) for every identifier 1..num_shares of every
    verifier, in ONE launch: pubshare_i = C_0 + [i] C_1 + ... + [i^(t-1)] C_(t-1)
    from the t commitments alone -- no share, and no secret, is needed or
    touched.  Per verifier returns the list of 48-byte pubshares, or the
    TblsError of new_tss for the first failing identifier."""
    verifiers = [_verifier_bytes(v) for v in verifiers]
    if not 1 <= int(num_shares) <= 255:
        raise TblsError("new TSS: need 1 <= num_shares <= 255")
    if not verifiers:
        return []
    ids = list(range(1, int(num_shares) + 1))
    out = []
    for pks, st, cst in _eval_verifiers(verifiers, [ids] * len(verifiers), _engine(engine)):
        bad = next((s for s in st if s != eng.FV_OK), None)
        out.append([bytes(pk) for pk in pks] if bad is None else _fv_error(bad, cst))
    return out


def new_tss_batch(verifiers, num_shares: int, engine=None):
    """new_tss for many verifiers in ONE launch: a TSS per verifier, or its TblsError."""
    verifiers = [_verifier_bytes(v) for v in verifiers]
    out = []
    for cs, r in zip(verifiers, pubshares_from_commitments_batch(verifiers, num_shares, engine)):
        if isinstance(r, Exception):
            out.append(r)
        else:
            out.append(TSS({i + 1: PublicKey(pk) for i, pk in enumerate(r)}, int(num_shares), len(cs), PublicKey(cs[0]),
                           tuple(cs)))
    return out


def new_tss(commitments, num_shares: int, engine=None) -> TSS:
    """tbls.NewTSS (tss.go:95-116): the TSS of a Feldman verifier -- the t
    commitments C_j = [a_j] g1, 48 bytes each, lowest coefficient first.  The
    threshold is their number, the group key is C_0 and pubshare i is the
    commitment polynomial evaluated at i on the GPU (Engine.eval_commitments).
    Raises as the reference does, for the first failing i in the order 1..n:
    "unmarshal pubkey: public key is the identity" when C_0 is the identity,
    "unmarshal pubshare: public key is the identity" when a pubshare is.  Go
    receives the verifier as decoded points; here it arrives as bytes, so a
    commitment that does not decode raises "unmarshal commitment: ..." with
    key_from_bytes_batch's reason -- that string is this project's own.  A
    commitment of another length raises as PublicKey does."""
    r = new_tss_batch([commitments], num_shares, engine)[0]
    if isinstance(r, Exception):
        raise r
    return r


def feldman_verify_batch(items, engine=None):
    """Feldman share verification (kryptology FeldmanVerifier.Verify, the check
    a DKG participant runs on every share it receives): items is a list of
    (commitments, SecretKeyShare); item k is True when [value] g1 equals the
    verifier's polynomial evaluated at the share's identifier.  ONE
    eval_commitments launch for the public side and ONE launch of the hardened
    signer (tbg_sk_to_pk_ct: the share is a real secret) for [value] g1; the two
    48-byte encodings are compared here.  A zero or out-of-range share value is
    False; a verifier that does not decode (or has no group key) is a TblsError
    with new_tss's string."""
    items = [(_verifier_bytes(v), s) for v, s in items]
    if not items:
        return []
    e = _engine(engine)
    res = _eval_verifiers([v for v, _ in items], [[s.identifier] for _, s in items], e)
    # (a value that does not fit 32 bytes is sent as 0: refused like a zero share)
    sk = b"".join(int(s.value).to_bytes(32, "big") if 0 <= int(s.value) < 1 << 256 else bytes(32) for _, s in items)
    pks, kst = e.sk_to_pk_ct(sk)
    out = []
    for (rhs, st, cst), pk, ks in zip(res, pks, kst.tolist()):
        if st[0] not in (eng.FV_OK, eng.FV_IDENTITY):
            out.append(_fv_error(st[0], cst))
        else:
            out.append(ks == eng.KS_OK and bytes(pk) == bytes(rhs[0]))
    return out


def generate_tss(t: int, n: int, rng, engine=None, hardened=False):
    """tbls.GenerateTSS (tss.go:120-139): a random secret split t-of-n and its
    TSS.  Returns (TSS, shares, secret); the secret is returned for the parity
    tests (the reference discards it).  Test clusters only: see split_secret
    (hardened=True: every scalar multiplication on the fixed schedule, the
    split itself still on host integers).  generate_tss_batch runs the split
    on the device too and returns the same values for the same rng."""
    secret = rng.randrange(1, R)
    try:
        shares, commits = split_secret(secret, t, n, rng, engine, hardened=hardened)
    except TblsError as err:
        raise TblsError("generate secret shares: " + str(err))
    return tss_from_shares(shares, commits, engine, hardened=hardened), shares, secret


def combine_shares(shares, t: int, n: int) -> int:
    """tbls.CombineShares (tss.go:220-253): the secret from at least t shares,
    Lagrange interpolation at 0 mod r over ALL shares given.  Host integers,
    not side-channel safe: not for production keys -- those go through
    combine_shares_batch (tbg_combine_shares_ct), which interpolates on the
    device in masks."""
    shares = list(shares)
    if not (2 <= t <= n <= 255):
        raise TblsError("new Feldman VSS: need 2 <= t <= n <= 255")
    if len(shares) < t:
        raise TblsError("combine shares: fewer shares than the threshold")
    ids = [s.identifier for s in shares]
    if len(set(ids)) != len(ids):
        raise TblsError("combine shares: duplicate share identifier")
    if any(i > n for i in ids):
        raise TblsError("combine shares: invalid share identifier")
    acc = 0
    for s in shares:
        num = den = 1
        for j in ids:
            if j != s.identifier:
                num = num * j % R
                den = den * (j - s.identifier) % R
        acc = (acc + s.value * num * pow(den, R - 2, R)) % R
    return acc


def sign(secret: int, msg: bytes, engine=None, hardened=False) -> Signature:
    """tbls.Sign (tss.go:210-217) over Engine.sign.  TEST-ONLY like tbg_sign:
    a plain double-and-add whose timing depends on the key -- not side-channel
    safe, never for a production validator key.  hardened=True signs through
    sign_batch (tbg_sign_ct) instead and raises its TblsError."""
    if hardened:
        r = sign_batch([(secret, msg)], engine)[0]
        if isinstance(r, Exception):
            raise r
        return r
    return Signature(bytes(_engine(engine).sign(_sk32(secret), [bytes(msg)], [0])[0]))


def partial_sign(share: SecretKeyShare, msg: bytes, engine=None, hardened=False) -> PartialSignature:
    """tbls.PartialSign (tss.go:200-207) over Engine.sign.  TEST-ONLY like
    tbg_sign: not side-channel safe, never for a production key share.
    hardened=True signs through partial_sign_batch (tbg_sign_ct) instead."""
    if hardened:
        r = partial_sign_batch([(share, msg)], engine)[0]
        if isinstance(r, Exception):
            raise r
        return r
    return PartialSignature(share.identifier, sign(share.value, msg, engine))


# ------------------------------------------------------------ the hardened signer
# tbg_sign_ct / tbg_sk_to_pk_ct (include/tbls_gpu.h): [sk]H(m) and [sk]G1 on a
# fixed schedule -- the device's instruction and address streams do not depend
# on the key, and the engine wipes every byte it allocated for keys.  The
# Python integers and byte strings a caller holds are the caller's to guard.
_KS_ERRORS = {
    eng.KS_ZERO: "secret key cannot be zero",
    eng.KS_RANGE: "secret key is not below the group order",
    eng.KS_MSG: "hash to curve failed",
}


def _sk32_exact(v: int) -> bytes:
    """32 big-endian bytes of v WITHOUT reduction mod r: the engine's range
    check decides (KS_ZERO / KS_RANGE)."""
    v = int(v)
    if not 0 <= v < 1 << 256:
        raise TblsError("unmarshal secret: secret key must be 32 bytes")
    return v.to_bytes(32, "big")


def sign_batch(items, engine=None):
    """items: iterable of (secret, msg).  tbls.Sign for each in ONE launch of
    the hardened signer; equal messages are sent (and hashed) once.  Returns
    a Signature per item, or a TblsError: "unmarshal secret: ..." for a zero
    or out-of-range secret (tblsconv.ShareToSecret / SecretFromBytes,
    tblsconv.go:149-159), "sign: ..." (tss.go:213) when H(m) failed."""
    items = list(items)
    if not items:
        return []
    msgs, item_msg = _distinct_msgs([bytes(m) for _, m in items])
    sigs, st = _engine(engine).sign_ct(b"".join(_sk32_exact(s) for s, _ in items), msgs, item_msg)
    out = []
    for sig, s in zip(sigs, st.tolist()):
        if s == eng.KS_OK:
            out.append(Signature(bytes(sig)))
        else:
            out.append(TblsError(("sign: " if s == eng.KS_MSG else "unmarshal secret: ") + _KS_ERRORS.get(s, f"status {s}")))
    return out


def partial_sign_batch(items, engine=None):
    """items: iterable of (SecretKeyShare, msg).  tbls.PartialSign for each in
    one launch of the hardened signer: a PartialSignature per item, or
    sign_batch's TblsError ("partial sign: ..." when H(m) failed, tss.go:203)."""
    items = list(items)
    out = []
    for (share, _), r in zip(items, sign_batch([(sh.value, m) for sh, m in items], engine)):
        if isinstance(r, Exception):
            out.append(TblsError(str(r).replace("sign: ", "partial sign: ", 1) if str(r).startswith("sign: ") else str(r)))
        else:
            out.append(PartialSignature(share.identifier, r))
    return out


def secret_to_public_key_batch(secrets, engine=None):
    """SecretKey.GetPublicKey for many secrets in one launch of the hardened
    signer: a PublicKey per secret, or TblsError("secret to pubkey: ...")
    (cmd/createcluster.go:185-188) for a zero or out-of-range one."""
    secrets = list(secrets)
    if not secrets:
        return []
    pks, st = _engine(engine).sk_to_pk_ct(b"".join(_sk32_exact(s) for s in secrets))
    return [PublicKey(bytes(pk)) if s == eng.KS_OK else TblsError("secret to pubkey: " + _KS_ERRORS.get(s, f"status {s}"))
            for pk, s in zip(pks, st.tolist())]


# ------------------------------------------------------------ shares on a fixed schedule
# tbg_split_secret_ct / tbg_combine_shares_ct (include/tbls_gpu.h): the Fr
# arithmetic of SplitSecret, GenerateTSS and CombineShares on the device, in
# masks -- what split_secret and combine_shares do on host integers.  Same
# limits as the hardened signer: the Python integers a caller holds (and the
# coefficients drawn here from its rng) are the caller's to guard.
_SH_SPLIT_ERRORS = {
    eng.SH_COEF_RANGE: "convert to scaler: a coefficient is not below the group order",
    eng.SH_COEF_ZERO: "split Secret Key: invalid secret (a zero coefficient)",
    eng.SH_SHARE_ZERO: "unmarshalling shamir share: secret key cannot be zero",
}
_SH_COMBINE_ERRORS = {
    eng.SH_TOO_FEW: "combine shares: fewer than two shares",
    eng.SH_ID: "combine shares: invalid share identifier",
    eng.SH_DUPLICATE_ID: "combine shares: duplicate share identifier",
    eng.SH_VALUE_ZERO: "combine shares: a share value is zero",
    eng.SH_VALUE_RANGE: "combine shares: a share value is not below the group order",
    eng.SH_SECRET_ZERO: "unmarshal secret: secret key cannot be zero",
}


def _split_device(polys, n: int, e, pubshares=True):
    """ONE Engine.split_secret_ct call over integer polynomials (lowest
    coefficient first, sent WITHOUT reduction: the engine's range check
    decides).  Per polynomial: (shares, commitments, pubshares or None), or
    the TblsError of its SH_* code."""
    first = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)
    sh, cm, pub, st = e.split_secret_ct(b"".join(_sk32_exact(c) for p in polys for c in p), first, n, pubshares)
    out = []
    for k, s in enumerate(st.tolist()):
        if s != eng.SH_OK:
            out.append(TblsError(_SH_SPLIT_ERRORS.get(s, f"split secret: status {s}")))
            continue
        shares = [SecretKeyShare(i + 1, int.from_bytes(bytes(sh[k * n + i]), "big")) for i in range(n)]
        commits = [bytes(c) for c in cm[first[k]:first[k + 1]]]
        out.append((shares, commits, [bytes(pk) for pk in pub[k * n:(k + 1) * n]] if pubshares else None))
    return out


def split_secret_batch(items, n: int, rng, engine=None):
    """tbls.SplitSecret for many secrets in ONE engine call on the fixed
    schedule (tbg_split_secret_ct): items is a list of (secret, t).  The
    coefficients are drawn with ``rng.randrange(1, R)`` in the order sequential
    split_secret calls draw them, so the same seed gives the same shares; the
    polynomial is evaluated on the device in masks (csrc/bls_frct.h), and the
    commitments and pubshares are formed by the hardened ladder from the
    device copies.  Per item returns (shares, commitments, pubshares) or a
    TblsError: "new Feldman VSS: ..." for a bad (t, n) (nothing is drawn, as
    in split_secret), "convert to scaler: ..." / "split Secret Key: ..." for a
    secret (or coefficient) the engine refuses -- it is sent as given, not
    reduced mod r, and its t - 1 draws are consumed -- and "unmarshalling
    shamir share: ..." when some f(i) is zero."""
    items = [(int(s), int(t)) for s, t in items]
    res, polys, slots = [], [], []
    for k, (secret, t) in enumerate(items):
        if not (2 <= t <= n <= 255):
            res.append(TblsError("new Feldman VSS: need 2 <= t <= n <= 255"))
            continue
        polys.append([secret] + [rng.randrange(1, R) for _ in range(t - 1)])
        slots.append(k)
        res.append(None)
    if polys:
        for k, r in zip(slots, _split_device(polys, n, _engine(engine))):
            res[k] = r
    return res


def generate_tss_batch(count: int, t: int, n: int, rng, engine=None):
    """tbls.GenerateTSS ``count`` times in ONE engine call: a list of (TSS,
    shares, secret), bit-identical to ``count`` sequential generate_tss calls
    with the same seed (per item the secret is drawn, then its t - 1
    coefficients).  Split, commitments and pubshares all on the fixed
    schedule (split_secret_batch).  Raises generate_tss's TblsError."""
    if not (2 <= t <= n <= 255):
        raise TblsError("generate secret shares: new Feldman VSS: need 2 <= t <= n <= 255")
    polys = []
    for _ in range(int(count)):
        secret = rng.randrange(1, R)
        polys.append([secret] + [rng.randrange(1, R) for _ in range(t - 1)])
    if not polys:
        return []
    out = []
    for poly, r in zip(polys, _split_device(polys, n, _engine(engine))):
        if isinstance(r, Exception):
            raise TblsError("generate secret shares: " + str(r))
        shares, commits, pks = r
        out.append((TSS({s.identifier: PublicKey(pk) for s, pk in zip(shares, pks)}, n, t, PublicKey(commits[0]),
                        tuple(commits)), shares, poly[0]))
    return out


def combine_shares_batch(sets, engine=None):
    """tbls.CombineShares for many share sets in ONE launch on the fixed
    schedule (tbg_combine_shares_ct): sets is a list of (shares, t, n).
    combine_shares's host checks on public data run first, with its exact
    strings; the sets that pass go out together.  Per set returns the secret
    (int) or a TblsError: "combine shares: ..." for what the engine refuses (a
    zero or out-of-range value), "unmarshal secret: ..." when the combined
    secret is zero."""
    res, good, slots = [], [], []
    for k, (shares, t, n) in enumerate(sets):
        shares = list(shares)
        ids = [s.identifier for s in shares]
        err = None
        if not (2 <= t <= n <= 255):
            err = "new Feldman VSS: need 2 <= t <= n <= 255"
        elif len(shares) < t:
            err = "combine shares: fewer shares than the threshold"
        elif len(set(ids)) != len(ids):
            err = "combine shares: duplicate share identifier"
        elif any(i > n for i in ids):
            err = "combine shares: invalid share identifier"
        if err is None:
            try:
                good.append((ids, b"".join(_sk32_exact(s.value) for s in shares)))
                slots.append(k)
            except TblsError as e32:
                err = "combine shares: " + str(e32).split(": ", 1)[-1]
        res.append(TblsError(err) if err else None)
    if good:
        first = np.concatenate([[0], np.cumsum([len(ids) for ids, _ in good])]).astype(np.uint32)
        out, st = _engine(engine).combine_shares_ct(b"".join(v for _, v in good), [i for ids, _ in good for i in ids], first)
        for k, sec, s in zip(slots, out, st.tolist()):
            res[k] = int.from_bytes(bytes(sec), "big") if s == eng.SH_OK else \
                TblsError(_SH_COMBINE_ERRORS.get(s, f"combine shares: status {s}"))
    return res
