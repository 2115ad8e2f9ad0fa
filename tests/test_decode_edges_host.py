"""The directed encodings of tests/edge_decode.py on the CPU: every entry
through the HOST build of the decode path (tests/hostcheck: hc_g2_decode_raw,
hc_g2_decompress, hc_pair_decode_sig, hc_subgroup_raw, hc_g1_decompress,
hc_g1_decode_raw; TBG_BOUNDS_CHECK on, so a limb form outside bls_field.h's
documented ranges aborts the process) against the oracle.  The lists' own
claims -- which branch each entry reaches -- are asserted when edge_decode is
imported.  Passing here is what licenses sending the same lists to the GPU
(tests/test_gpu_devcheck_decode.py, tests/test_gpu_decode_edges.py)."""
import ctypes

from oracle import bls12_381 as bls
from tests import edge_decode as ed
from tests import edge_operands as eo
from tests.edge_points import aff_words
from tests.hostcheck import lib

P = bls.P


def _u(words):
    return (ctypes.c_uint32 * len(words))(*words)


def host_g2_raw(data):
    out = _u([eo.SENTINEL] * ed.AFF_W)
    return lib().hc_g2_decode_raw(data, out), list(out)


def host_g1_raw(data):
    out, outx = _u([eo.SENTINEL] * ed.G1A_W), _u([eo.SENTINEL] * ed.G1A_W)
    return lib().hc_g1_decode_raw(data, out, outx), list(out), list(outx)


def test_g2_entries_decode_on_host():
    """k_decode_sigs' body: status and stored limbs per entry."""
    for i, e in enumerate(ed.g2_entries()):
        dec, pt = ed.g2_class(e.data, False)
        st, words = host_g2_raw(e.data)
        err = ed.check_g2_slot(words, ed.ps_of(st), ed.ps_of(dec), pt)
        assert err is None, (i, e.kind, e.branch, err)


def test_g2_entries_full_decompress_on_host():
    """The out-of-line and the inline full decompression (hc_g2_decompress
    compares the two) and the decode + lane-pair subgroup test of the two
    kernels give the oracle's full class."""
    for i, e in enumerate(ed.g2_entries()):
        dec, pt = ed.g2_class(e.data, True)
        buf = ctypes.create_string_buffer(192)
        assert lib().hc_g2_decompress(e.data, buf) == dec, (i, e.kind)
        if dec == ed.DEC_OK:
            got = [int.from_bytes(buf.raw[48 * k:48 * k + 48], "big") for k in range(4)]
            assert ((got[0], got[1]), (got[2], got[3])) == pt, (i, e.kind)
        assert lib().hc_pair_decode_sig(e.data) == dec, (i, e.kind)
        assert lib().hc_k_decode_sigs(e.data) == ed.g2_class(e.data, False)[0], (i, e.kind)


def test_subgroup_kernel_body_on_stored_limb_forms():
    """k_subgroup_sigs' body on points as the decoder may store them and in
    the plus_p / neg16 limb forms of tests/edge_points.py: the verdict is the
    oracle's, and no point sets `exc`."""
    pts = ed.subgroup_points()
    assert sum(bls.g2_in_subgroup(p) for _, p in pts) * 2 == len(pts)
    for name, p in pts:
        for form in ed.SUBGROUP_FORMS:
            flags = lib().hc_subgroup_raw(_u(aff_words(p, form)))
            assert flags == int(bls.g2_in_subgroup(p)), (name, form, flags)
        st, words = host_g2_raw(bls.g2_compress(p))
        assert st == ed.DEC_OK and lib().hc_subgroup_raw(_u(words)) == int(bls.g2_in_subgroup(p)), name


def test_g1_entries_on_host():
    for i, e in enumerate(ed.g1_entries()):
        dec, pt = ed.g1_class(e.data)
        buf = ctypes.create_string_buffer(96)
        assert lib().hc_g1_decompress(e.data, buf) == dec, (i, e.kind)
        if dec == ed.DEC_OK:
            assert (int.from_bytes(buf.raw[:48], "big"), int.from_bytes(buf.raw[48:], "big")) == pt, (i, e.kind)
        st, out, outx = host_g1_raw(e.data)
        err = ed.check_g1_slot(out, outx, st, dec, pt)
        assert err is None, (i, e.kind, e.branch, err)


def test_g1_layout_places_the_failures():
    for blk in (64, 256):
        lay = ed.g1_layout(blk)
        assert len(lay) == blk + 3
        rare = [e for e in ed.g1_entries() if not e.kind.startswith("valid")]
        assert all(e in lay for e in rare)


def test_checkers_reject_one_word_off():
    e = next(e for e in ed.g2_entries() if e.kind == "valid")
    dec, pt = ed.g2_class(e.data, False)
    st, words = host_g2_raw(e.data)
    assert ed.check_g2_slot(words, ed.ps_of(st), ed.ps_of(dec), pt) is None
    for j in range(0, ed.AFF_W, 3):
        for d in (1, -1):
            w = list(words)
            w[j] += d
            assert ed.check_g2_slot(w, ed.ps_of(st), ed.ps_of(dec), pt) is not None, j
    assert ed.check_g2_slot(words, ed.DEC_ERR_FIELD, ed.ps_of(dec), pt) is not None
    assert ed.check_g2_slot(words, ed.ps_of(st), ed.ps_of(dec), ((pt[0][0] ^ 1, pt[0][1]), pt[1])) is not None
    # the right residue in the wrong range, and a limb at 2^28
    w = list(words)
    w[:eo.NL] = eo.limbs(eo.val(words[:eo.NL]) % P + 2 * P)
    assert ed.check_g2_slot(w, ed.ps_of(st), ed.ps_of(dec), pt) is not None
    w = list(words)
    w[0], w[1] = w[0] + (1 << 28), w[1] - 1
    assert w[1] >= 0 and ed.check_g2_slot(w, ed.ps_of(st), ed.ps_of(dec), pt) is not None
    # a failed partial stores zeros
    zero = [0] * ed.AFF_W
    assert ed.check_g2_slot(zero, ed.DEC_ERR_FLAGS, ed.DEC_ERR_FLAGS, None) is None
    assert ed.check_g2_slot(zero[:-1] + [1], ed.DEC_ERR_FLAGS, ed.DEC_ERR_FLAGS, None) is not None
    assert ed.check_g2_slot(zero, ed.DEC_ERR_FIELD, ed.DEC_ERR_FLAGS, None) is not None
    k = next(e for e in ed.g1_entries() if e.kind == "valid")
    dec, pt = ed.g1_class(k.data)
    st, out, outx = host_g1_raw(k.data)
    assert ed.check_g1_slot(out, outx, st, dec, pt) is None
    for j in range(0, ed.G1A_W, 3):
        w = list(out)
        w[j] ^= 1
        assert ed.check_g1_slot(w, outx, st, dec, pt) is not None
        w = list(outx)
        w[j] ^= 1
        assert ed.check_g1_slot(out, w, st, dec, pt) is not None
    assert ed.check_g1_slot(out, outx, ed.DEC_ERR_SUBGROUP, dec, pt) is not None
    assert ed.check_g1_slot(out, outx, st, dec, (pt[0], pt[1] ^ 1)) is not None
