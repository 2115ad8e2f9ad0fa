"""tbg_eval_commitments' boundary without a GPU: the call is declared in
include/tbls_gpu.h with its status codes, exported by the built library and
bound in charon_amd/_native.py; the Python mirror's names exist and
dkg.create_cluster_tss's `from_commitments` keyword is off by default, so the
existing entry points keep their code path; and the call's workspace
(EvalCommitWork, tbls_work.h) has the sections and sizes that
tests/golden/feldman_workspace.json records, walked on the CPU by a host
twin of its own (tests/feldman/work_host.cpp, in the way of tests/plan)."""
import ctypes
import inspect
import json
import os
import re

import numpy as np

from charon_amd import _native, dkg, engine, tbls
from tests import edge_feldman as ef
from tests.feldman import work_lib

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "tbg_eval_commitments"


def test_header_declares_the_call_and_its_codes():
    src = open(_native.HEADER).read()
    assert re.search(r"^int %s\(tbg_ctx\*" % NAME, src, re.M)
    codes = dict(re.findall(r"^#define (TBG_FV_\w+) \(?(-?\d+)\)?", src, re.M))
    assert {k: int(v) for k, v in codes.items()} == {"TBG_FV_OK": 0, "TBG_FV_ID": -50, "TBG_FV_COMMIT": -51,
                                                     "TBG_FV_KEY_IDENTITY": -52, "TBG_FV_IDENTITY": -53}
    assert (engine.FV_OK, engine.FV_ID, engine.FV_COMMIT, engine.FV_KEY_IDENTITY, engine.FV_IDENTITY) == \
        (ef.FV_OK, ef.FV_ID, ef.FV_COMMIT, ef.FV_KEY_IDENTITY, ef.FV_IDENTITY) == (0, -50, -51, -52, -53)
    decl = src[src.index("int %s(" % NAME):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") == 9  # ten arguments


def test_library_exports_and_binding():
    assert os.path.exists(_native.LIB_PATH), "libtbls_gpu.so is not built (__graft_entry__.build())"
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, NAME)
    res, args = _native.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 10
    assert [args[3], args[6]] == [ctypes.c_uint32, ctypes.c_uint32]  # n_polys, n_evals


def test_python_names_and_the_keyword_default():
    p = inspect.signature(dkg.create_cluster_tss).parameters.get("from_commitments")
    assert p is not None and p.default is False
    assert hasattr(engine.Engine, "eval_commitments")
    for fn in (tbls.new_tss, tbls.new_tss_batch, tbls.pubshares_from_commitments_batch):
        assert list(inspect.signature(fn).parameters)[1:] == ["num_shares", "engine"], fn.__name__
    assert list(inspect.signature(tbls.feldman_verify_batch).parameters) == ["items", "engine"]
    assert "not implemented" not in tbls.tss_from_shares.__doc__


def test_argument_errors_raise_before_the_engine():
    """Wrong lengths raise as PublicKey does, with no engine in sight."""
    for bad in ([bytes(47)], [ef.IDENT48, b""], [b"\x00" * 96]):
        for call in (lambda: tbls.new_tss(bad, 3, engine=object()),
                     lambda: tbls.feldman_verify_batch([(bad, tbls.SecretKeyShare(1, 5))], engine=object())):
            try:
                call()
            except tbls.TblsError as err:
                assert str(err) == "unmarshal pubkey: invalid length"
            else:
                raise AssertionError(bad)
    for n in (0, 256):
        try:
            tbls.new_tss([ef.IDENT48], n, engine=object())
        except tbls.TblsError as err:
            assert "num_shares" in str(err)
        else:
            raise AssertionError(n)
    assert tbls.new_tss_batch([], 3, engine=object()) == [] and tbls.feldman_verify_batch([], engine=object()) == []


def work(dims, base=0):
    n_max = work_lib().fvw_max_sections()
    total = ctypes.c_uint64(0)
    secs = np.zeros((n_max, 2), dtype=np.uint64)
    ptrs = np.zeros(n_max, dtype=np.uint64)
    names = (ctypes.c_char_p * n_max)()
    n = work_lib().fvw_work(dims["n_commits"], dims["n_polys"], dims["n_evals"], base, ctypes.addressof(total),
                            secs.ctypes.data, ptrs.ctypes.data, ctypes.addressof(names))
    assert 0 < n <= n_max
    return total.value, [(names[i].decode(), int(secs[i, 0]), int(secs[i, 1]), int(ptrs[i])) for i in range(n)]


def test_workspace_equals_the_recorded_one():
    with open(os.path.join(HERE, "golden", "feldman_workspace.json")) as f:
        gold = json.load(f)
    assert len(gold["rows"]) == 2
    base = 0x7F0000001000
    for r in gold["rows"]:
        total, secs = work(r["dims"])
        assert [s[0] for s in secs] == gold["names"]
        assert [s[2] for s in secs] == r["sections"] and [s[1] for s in secs] == r["offsets"] and total == r["total"]
        assert all(s[3] == 0 for s in secs)  # (the sizing walk hands out nothing)
        total_b, bound = work(r["dims"], base)
        assert total_b == total and [(s[0], s[1], s[2]) for s in bound] == [(s[0], s[1], s[2]) for s in secs]
        assert [s[3] for s in bound] == [base + off for off in r["offsets"]]
