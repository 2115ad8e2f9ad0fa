"""The hardened signer's boundary without a GPU: the two calls are declared in
include/tbls_gpu.h with their status codes, exported by the built library and
bound in charon_amd/_native.py; the Python mirror's `hardened` keyword exists
and is off by default, so the existing entry points keep their code path."""
import ctypes
import inspect
import os
import re

from charon_amd import _native, dkg, engine, tbls
from tests import edge_scalars as es

NAMES = ["tbg_sk_to_pk_ct", "tbg_sign_ct"]


def test_header_declares_the_calls_and_their_codes():
    src = open(_native.HEADER).read()
    for n in NAMES:
        assert re.search(r"^int %s\(tbg_ctx\*" % n, src, re.M), n
    codes = dict(re.findall(r"^#define (TBG_KS_\w+) \(?(-?\d+)\)?", src, re.M))
    assert {k: int(v) for k, v in codes.items()} == {"TBG_KS_OK": 0, "TBG_KS_ZERO": es.KS_ZERO,
                                                     "TBG_KS_RANGE": es.KS_RANGE, "TBG_KS_MSG": es.KS_MSG}
    assert (engine.KS_OK, engine.KS_ZERO, engine.KS_RANGE, engine.KS_MSG) == (0, es.KS_ZERO, es.KS_RANGE, es.KS_MSG)
    # the old entry points keep their warning and point to the new ones
    note = src[src.index("TEST-ONLY"):src.index("int tbg_sk_to_pk(")]
    assert "tbg_sk_to_pk_ct" in note and "tbg_sign_ct" in note


def test_library_exports_and_binding():
    assert os.path.exists(_native.LIB_PATH), "libtbls_gpu.so is not built (__graft_entry__.build())"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _native.SIGNATURES
    assert len(_native.SIGNATURES["tbg_sk_to_pk_ct"][1]) == 5 and len(_native.SIGNATURES["tbg_sign_ct"][1]) == 9


def test_hardened_keyword_defaults_to_false():
    for fn in (tbls.sign, tbls.partial_sign, tbls.split_secret, tbls.tss_from_shares, tbls.generate_tss,
               dkg.create_cluster_tss):
        p = inspect.signature(fn).parameters.get("hardened")
        assert p is not None and p.default is False, fn.__name__
    for fn in (tbls.sign_batch, tbls.partial_sign_batch, tbls.secret_to_public_key_batch, dkg.sign_deposit_data,
               dkg.sign_lock_hash, dkg.create_cluster_sign_deposit_data, dkg.agg_sign_lock_hash):
        assert "hardened" not in inspect.signature(fn).parameters  # always the hardened path
    assert hasattr(engine.Engine, "sk_to_pk_ct") and hasattr(engine.Engine, "sign_ct")


def test_exact_key_bytes_are_not_reduced():
    """The hardened path hands the engine the scalar as given: the range check, not a silent
    reduction mod r, decides about r and above."""
    assert tbls._sk32_exact(es.R) == es.be32(es.R) and tbls._sk32(es.R) == bytes(32)
    for bad in (-1, 1 << 256):
        try:
            tbls._sk32_exact(bad)
        except tbls.TblsError as err:
            assert "32 bytes" in str(err)
        else:
            raise AssertionError(bad)
