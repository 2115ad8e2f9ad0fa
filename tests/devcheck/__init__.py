"""Device (gfx950) unit harness for the lane-cooperative field arithmetic, the
lane-pair G2 group law, the hash-to-G2 kernel chain and the decode kernels.

TEST TOOLING ONLY -- see devcheck.hip.  The GPU twin of tests/hostcheck:
thin kernels around the product headers' device functions, built with the
engine's compiler and common flags and checked by the same return-address
guard (the objects pull in the out-of-line hex_*_ni functions and the
cofactor clearing's out-of-line rare cases).  Never loaded by charon_amd.

devcheck_h2c.hip and devcheck_h2c_clear.hip #include the product's
k_hash.hip and k_hash_clear.hip themselves, each with the per-unit flags
charon_amd/_native.py gives that unit, so dc_h2c runs the product's own hash
kernels stage by stage on injected inputs; devcheck_decode.hip does the same
with k_decode.hip for dc_decode_sigs / dc_decode_pubkeys.  The library
therefore defines tbg::launch_hash_msgs, tbg::launch_decode_sigs and the
kernels' host stubs under the product's names:
it is linked with devcheck.map (only dc_* exported, everything else local)
and -Bsymbolic, and the build refuses a library that exports a tbg:: symbol, so
libdevcheck.so and libtbls_gpu.so each call their own code when both are
loaded in one process, in either order.  (The sources, their product units
and the build itself: tests/twin_build.py.)
"""
import ctypes

from tests import twin_build

_U32P = ctypes.POINTER(ctypes.c_uint32)
_I32P = ctypes.POINTER(ctypes.c_int32)
_U = ctypes.c_uint32
_I = ctypes.c_int

SIGNATURES = {
    "dc_sticky_error": [],
    "dc_binv_waves": [],
    "dc_fp": [_I, _U32P, _U32P, _U32P, _U32P, _U, _U32P, _U],
    "dc_row": [_I, _I32P, _I32P, _I32P, _I32P, _I32P, _U, _U],
    "dc_row12": [_I, _U32P, _U32P, _I32P, _U32P],
    "dc_row_lines": [_U32P, _U32P],
    "dc_hex": [_I, _U32P, _U32P, _U32P, _U32P, _U32P, _U32P, _U, _U],
    "dc_pair": [_I, _U32P, _U32P, _U32P, _U32P, _U, _U],
    "dc_pair_lines": [_U32P, _U32P, _U, _U],
    "dc_batch_inv": [_I, _U32P, _U32P, _U32P, _U, _U],
    "dc_jac_to_aff": [_I, _I, _U32P, _U32P, _U32P, _U32P, _U, _U],
    "dc_g2_sticky_error": [],
    "dc_g2_a_words": [_I],
    "dc_g2_b_words": [_I],
    "dc_g2": [_I, _U32P, _U32P, _U32P, _U32P, _U, _U],
    "dc_h2c_sticky_error": [],
    "dc_h2c_binv_block": [],
    "dc_h2c": [_I, _I, _U, ctypes.c_char_p, _U32P, _U32P, _U32P, _U32P, _I32P, _U],
    "dc_h2c_sqrt": [_U32P, _U32P, _U32P, _U, _U],
    "dc_decode_sticky_error": [],
    "dc_decode_binv_block": [],
    "dc_decode_cnt_words": [],
    "dc_decode_msm_buckets": [],
    "dc_decode_sigs": [_I, _I, _U, ctypes.c_char_p, _U32P, _I32P, _U32P, _U32P, _U, _U, _U, _U32P, _U],
    "dc_decode_pubkeys": [_U, ctypes.c_char_p, _U32P, _U32P, _I32P, _U],
}

# operation codes (devcheck.hip's enums)
FP_OPS = ["mul", "mul2", "sqr", "add", "sub", "addl_mul", "subl_mul", "neg", "negl_mul", "mul_small", "reduce",
          "canon", "inv", "inv_fermat", "from_signed", "lex"]
ROW_OPS = ["mul", "mul2", "reduce", "norm"]
R12_OPS = ["mul", "cyc", "frob", "conj", "fe", "isone"]
HEX_OPS = ["mul", "sqr", "cyc", "frob", "conj", "line", "inv", "fe", "isone"]
PAIR_OPS = ["mul", "sqr", "inv", "conj", "mul_xi", "mul_const", "eq", "gather"]
# devcheck_g2.hip; the same codes in tests/hostcheck's hc_g2_op_raw
G2_OPS = ["add_x", "add_aff_x", "dbl_lo", "add_in", "add_aff_in", "psi", "mul_xabs_x", "mul_xabs_aff_x",
          "in_subgroup_aff", "clear_cofactor", "sgb_sums", "sgb_sums_complete", "sgb_fold", "sgb_fold_complete"]
# devcheck_h2c.hip: dc_h2c's stages (MAP_MSG and MAP_U are the two forms of the first one)
H2C_STAGES = ["MAP_MSG", "MAP_U", "SSWU", "CLEAR_X1", "CLEAR_X2", "CLEAR_FIN", "AFFINE"]
# devcheck_decode.hip: dc_decode_sigs' stages (k_decode_sigs, k_subgroup_sigs)
DECODE_STAGES = ["DECODE", "SUBGROUP"]


def _signatures(L):
    for name, args in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = args


def build():
    """Compile the devcheck sources for gfx950 if the library is stale; raises
    without hipcc."""
    return twin_build.build("devcheck")


def lib():
    return twin_build.lib("devcheck", _signatures)
