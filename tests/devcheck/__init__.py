"""Device (gfx950) unit harness for the lane-cooperative field arithmetic.

TEST TOOLING ONLY -- see devcheck.hip.  The GPU twin of tests/hostcheck:
thin kernels around the product headers' device functions, built with the
engine's compiler and common flags and checked by the same return-address
guard (the object pulls in the out-of-line hex_*_ni functions).  Never loaded
by charon_amd.
"""
import ctypes
import os
import subprocess
import time

HERE = os.path.dirname(os.path.abspath(__file__))
# devcheck.hip: the field layer; devcheck_g2.hip: the lane-pair G2 group law,
# a source of its own because it is compiled as k_sgb.hip compiles that code
# (TBG_ADD_DBL_INLINE / TBG_SCHED_FENCE set before the product headers)
SRCS = [os.path.join(HERE, "devcheck.hip"), os.path.join(HERE, "devcheck_g2.hip")]
LIB = os.path.join(HERE, "libdevcheck.so")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Wno-unused-result",
         "-Wno-unused-value"]

# seconds the last build() spent compiling (None: the library was up to date)
LAST_BUILD_SECONDS = None


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > t for d in deps)


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
            list(ex.map(lambda so: subprocess.check_call([hipcc] + FLAGS + ["-c", so[0], "-o", so[1]]),
                        zip(SRCS, objs)))
        for obj in objs:
            _native.check_return_address(obj)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB + ".tmp"])
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
}

# operation codes (devcheck.hip's enums)
FP_OPS = ["mul", "mul2", "sqr", "add", "sub", "addl_mul", "subl_mul", "neg", "negl_mul", "mul_small", "reduce",
          "canon", "inv", "inv_fermat", "from_signed"]
ROW_OPS = ["mul", "mul2", "reduce", "norm"]
R12_OPS = ["mul", "cyc", "frob", "conj", "fe", "isone"]
HEX_OPS = ["mul", "sqr", "cyc", "frob", "conj", "line", "inv", "fe", "isone"]
PAIR_OPS = ["mul", "sqr", "inv", "conj", "mul_xi", "mul_const", "eq", "gather"]
# devcheck_g2.hip; the same codes in tests/hostcheck's hc_g2_op_raw
G2_OPS = ["add_x", "add_aff_x", "dbl_lo", "add_in", "add_aff_in", "psi", "mul_xabs_x", "mul_xabs_aff_x",
          "in_subgroup_aff", "clear_cofactor", "sgb_sums", "sgb_sums_complete", "sgb_fold", "sgb_fold_complete"]


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
