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
and -Bsymbolic, and build() refuses a library that exports a tbg:: symbol, so
libdevcheck.so and libtbls_gpu.so each call their own code when both are
loaded in one process, in either order.
"""
import ctypes
import os
import subprocess
import time

HERE = os.path.dirname(os.path.abspath(__file__))
# devcheck.hip: the field layer; devcheck_g2.hip: the lane-pair G2 group law,
# a source of its own because it is compiled as k_sgb.hip compiles that code
# (TBG_ADD_DBL_INLINE / TBG_SCHED_FENCE set before the product headers)
# devcheck_h2c.hip / devcheck_h2c_clear.hip: the hash-to-G2 chain, one source
# per product unit they include (INCLUDES: the flags of _native.UNIT_FLAGS
# follow the included unit)
# devcheck_decode.hip: the decode kernels, k_decode.hip included the same way
SRCS = [os.path.join(HERE, f) for f in ("devcheck.hip", "devcheck_g2.hip", "devcheck_h2c.hip",
                                        "devcheck_h2c_clear.hip", "devcheck_decode.hip")]
INCLUDES = {"devcheck_h2c.hip": "k_hash.hip", "devcheck_h2c_clear.hip": "k_hash_clear.hip",
            "devcheck_decode.hip": "k_decode.hip"}
LIB = os.path.join(HERE, "libdevcheck.so")
MAP = os.path.join(HERE, "devcheck.map")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Wno-unused-result",
         "-Wno-unused-value"]

# seconds the last build() spent compiling (None: the library was up to date)
LAST_BUILD_SECONDS = None


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    from charon_amd import _native
    deps = SRCS + [MAP, os.path.abspath(__file__), os.path.abspath(_native.__file__)]  # (the last two hold the flags)
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(CSRC, u) for u in INCLUDES.values()]
    return any(os.path.getmtime(d) > t for d in deps)


def unit_flags(src):
    """The per-unit flags of the product unit `src` includes (none for the
    sources that include headers only)."""
    from charon_amd import _native
    return list(_native.UNIT_FLAGS.get(INCLUDES.get(os.path.basename(src), ""), ()))


def _check_exports(lib):
    """Only the dc_* entries may be visible to the dynamic linker (see the
    module docstring)."""
    objdump = "/opt/rocm/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        raise RuntimeError(f"{objdump} is missing: cannot check the exports of {lib}")
    out = subprocess.run([objdump, "-T", lib], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines() if l[:1].isalnum() and l.split()[0].strip("0123456789abcdef") == ""]
    defined = [r[-1] for r in rows if "*UND*" not in r]
    if not any(s == "dc_h2c" for s in defined):
        raise RuntimeError(f"{lib}: dc_h2c not among the dynamic symbols {defined[:5]}")
    bad = [s for s in defined if not s.startswith("dc_")]
    if bad:
        raise RuntimeError(f"{lib} exports {bad[:5]} ({len(bad)} symbols besides dc_*): these could bind across "
                           "libtbls_gpu.so")


def build():
    """Compile the devcheck sources for gfx950 if the library is stale; raises
    without hipcc."""
    global LAST_BUILD_SECONDS
    if _stale():
        from charon_amd import _native
        hipcc = _native._hipcc()  # raises: a stale library is an error, never a skip
        t0 = time.time()
        from concurrent.futures import ThreadPoolExecutor
        objs = [os.path.splitext(src)[0] + ".o" for src in SRCS]
        with ThreadPoolExecutor(max_workers=len(SRCS)) as ex:
            list(ex.map(lambda so: subprocess.check_call([hipcc] + FLAGS + unit_flags(so[0]) +
                                                         ["-c", so[0], "-o", so[1]]),
                        zip(SRCS, objs)))
        for obj in objs:
            _native.check_return_address(obj)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-Bsymbolic",
                               "-Wl,--version-script=" + MAP] + objs + ["-o", LIB + ".tmp"])
        _check_exports(LIB + ".tmp")
        os.replace(LIB + ".tmp", LIB)
        LAST_BUILD_SECONDS = time.time() - t0
    return LIB


_lib = None

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


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = ctypes.c_int
            fn.argtypes = args
        _lib = L
    return _lib
