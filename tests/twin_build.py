"""Every test twin, stated once, and the one builder behind them.

TEST TOOLING ONLY.  A twin is a small library (or program) under
tests/<name>/ that compiles the product headers a second time, for the host
(CPU tests: the arithmetic away from the engine, most with TBG_BOUNDS_CHECK)
or for gfx950 (GPU tests: thin kernels around the device functions).  TWINS
below names each one -- sources, output, flags -- and the packages
tests/<name>/__init__.py keep only what is their own (ctypes signatures,
operation codes) on top of build() and lib() here.

One rule each for all of them:
  compiler   host twins: $ROCM_PATH/llvm/bin/clang++ (/opt/rocm by default),
             else clang++; device twins: the engine's hipcc (_native._hipcc,
             which raises: a stale device library is an error, never a skip)
  staleness  an output is stale if it is missing or older than its sources
             and declared dependencies, any charon_amd/csrc/*.h, the product
             units it names, its version script, this module, the package's
             __init__.py or, for a device twin, charon_amd/_native.py (which
             holds the device flags)
  output     written under a per-process temporary name and moved into place
             (os.replace): a failed or concurrent build never leaves a partial
             file at the output path
A device twin is built as the engine is (_native.COMMON_FLAGS, each source
with the _native.UNIT_FLAGS of the product unit it stands for, the
return-address guard on every object) and linked with -Bsymbolic and a
version script; the link is refused unless the library's defined dynamic
symbols all carry its prefix, so it and libtbls_gpu.so each call their own
code when both are loaded in one process.
"""
import ctypes
import dataclasses
import os
import subprocess
import threading
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "charon_amd", "csrc")
NATIVE = os.path.join(ROOT, "charon_amd", "_native.py")
BUILDER = os.path.abspath(__file__)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
MAX_COMPILERS = 8  # at a time, over all threads (the cap of _native.build)


@dataclasses.dataclass(frozen=True)
class Twin:
    name: str
    kind: str  # "host" or "device"
    sources: tuple
    out: str
    flags: tuple = ()  # host: everything between the compiler and the source
    deps: tuple = ()  # further files the output is built from
    # device twins: source file name -> the product unit whose _native.UNIT_FLAGS it takes
    units: dict = dataclasses.field(default_factory=dict)
    version_script: str = ""
    prefix: str = ""  # of every exported entry
    entry: str = ""  # one entry that must be among them
    variant_of: str = ""  # another build of that twin's source (tools/count_work.py)
    prebuild: bool = True  # built by build_all (__graft_entry__.build)

    def variant(self, name, out, flags):
        return dataclasses.replace(self, name=name, out=out, flags=tuple(flags), variant_of=self.name, prebuild=False)


def _t(*parts):
    return os.path.join(HERE, *parts)


_HOST = ("-O1", "-std=c++17", "-fPIC", "-shared")
_CHECKED = _HOST + ("-DTBG_BOUNDS_CHECK", "-Wno-pass-failed")  # aborts on any violated value bound
_COUNTED = _HOST + ("-DTBG_COUNT_OPS", "-Wno-pass-failed")  # counts u32 multiply-adds
_HIP_TYPES = ("-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"))  # reads the HIP headers' types only
_SANITIZED = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")


def _host(name, src=None, out=None, flags=_CHECKED, pkg=None, **kw):
    pkg = pkg or name
    return Twin(name, "host", (_t(pkg, src or name + "_host.cpp"),), _t(pkg, out or "lib%s_host.so" % name),
                tuple(flags), **kw)


def _device(name, srcs, units, prefix, entry):
    return Twin(name, "device", tuple(_t(*s.split("/")) for s in srcs), _t(name, "lib%s.so" % name), units=units,
                version_script=_t(name, name + ".map"), prefix=prefix, entry=entry)


_TWINS = [
    _host("hostcheck", "hostcheck.cpp", "libhostcheck.so"),
    _host("ctmul"),
    _host("feldman", flags=_HOST + ("-Wno-pass-failed", "-DTBG_BOUNDS_CHECK")),
    _host("feldman_work", "work_host.cpp", "libfeldman_work.so", _HOST + ("-Wno-pass-failed",) + _HIP_TYPES,
          pkg="feldman"),
    _host("frct", flags=("-O1", "-std=c++17", "-DTBG_BOUNDS_CHECK", "-Wno-pass-failed", "-fPIC", "-shared")),
    # the stand-alone sanitizer program (its own main(); #includes frct_host.cpp): run as a subprocess only
    _host("frct_main", "frct_main.cpp", "frct_main_san",
          ("-O1", "-std=c++17", "-DTBG_BOUNDS_CHECK", "-Wno-pass-failed") + _SANITIZED, pkg="frct",
          deps=(_t("frct", "frct_host.cpp"),)),
    _host("hexline"),
    _host("hlines"),
    _host("l0fused"),
    _host("l0msg"),
    _host("l0straus"),
    _host("l0tail"),
    _host("plan", flags=_HOST + _HIP_TYPES + ("-Wno-pass-failed",)),
    _host("sgbpair"),
    _host("sgbtri"),
    _host("shares", "work_host.cpp", "libshares_work.so", _HOST + ("-Wno-pass-failed",) + _HIP_TYPES),
    # devcheck.hip: the field layer; devcheck_g2.hip: the lane-pair G2 group law, a source of its own because it
    # is compiled as k_sgb.hip compiles that code; devcheck_h2c*.hip and devcheck_decode.hip #include the product
    # unit named here
    _device("devcheck", ["devcheck/devcheck.hip", "devcheck/devcheck_g2.hip", "devcheck/devcheck_h2c.hip",
                         "devcheck/devcheck_h2c_clear.hip", "devcheck/devcheck_decode.hip"],
            {"devcheck_h2c.hip": "k_hash.hip", "devcheck_h2c_clear.hip": "k_hash_clear.hip",
             "devcheck_decode.hip": "k_decode.hip"}, "dc_", "dc_h2c"),
    # (the kernel file lives beside the other device unit kernels; k_miller_hex.hip runs these steps most)
    _device("devcheck_hexline", ["devcheck/devcheck_hexline.hip"], {"devcheck_hexline.hip": "k_miller_hex.hip"},
            "dcx_", "dcx_hex_line"),
    # (k_verify.hip holds k_lines_h)
    _device("devcheck_hlines", ["devcheck_hlines/devcheck_hlines.hip"], {"devcheck_hlines.hip": "k_verify.hip"},
            "dch_", "dch_lines"),
]
TWINS = {t.name: t for t in _TWINS}
# the TBG_COUNT_OPS builds of tools/count_work.py
for _n in ("hostcheck", "hlines", "hexline", "l0fused", "l0straus"):
    TWINS[_n + "_count"] = TWINS[_n].variant(_n + "_count", _t(_n, "lib%s_count.so" % _n), _COUNTED)


def cxx():
    c = os.path.join(ROCM, "llvm", "bin", "clang++")
    return c if os.path.exists(c) else "clang++"


def _native():
    from charon_amd import _native
    return _native


def _tmp(twin):
    return twin.out + ".%d.tmp" % os.getpid()


def _objects(twin):
    return [os.path.join(os.path.dirname(twin.out), os.path.splitext(os.path.basename(s))[0] + ".o")
            for s in twin.sources]


def commands(twin):
    """The command lines build() runs for a stale `twin`, in order (a device
    twin's compile steps, one per source, then its link)."""
    if twin.kind == "host":
        return [[cxx()] + list(twin.flags) + list(twin.sources) + ["-o", _tmp(twin)]]
    nat = _native()
    hipcc = nat._hipcc()
    objs = _objects(twin)
    cmds = [[hipcc] + nat.COMMON_FLAGS + list(nat.UNIT_FLAGS.get(twin.units.get(os.path.basename(src), ""), ())) +
            ["-c", src, "-o", obj] for src, obj in zip(twin.sources, objs)]
    return cmds + [[hipcc] + nat.LINK_FLAGS + ["-Wl,-Bsymbolic", "-Wl,--version-script=" + twin.version_script] +
                   objs + ["-o", _tmp(twin)]]


def dependencies(twin):
    deps = list(twin.sources) + list(twin.deps) + [BUILDER]
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(CSRC, u) for u in twin.units.values()]
    package = os.path.join(os.path.dirname(twin.out), "__init__.py")
    if os.path.exists(package):
        deps.append(package)
    if twin.kind == "device":
        deps += [twin.version_script, NATIVE]
    return deps


def stale(twin):
    if not os.path.exists(twin.out):
        return True
    t = os.path.getmtime(twin.out)
    return any(os.path.getmtime(d) > t for d in dependencies(twin))


RAN = []  # every command line this process has run, in order
_slots = threading.BoundedSemaphore(MAX_COMPILERS)


def _run(cmd):
    with _slots:
        RAN.append(cmd)
        subprocess.check_call(cmd)


def check_exports(twin, lib):
    """Only the twin's own entries may be visible to the dynamic linker."""
    objdump = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
    if not os.path.exists(objdump):
        raise RuntimeError(f"{objdump} is missing: cannot check the exports of {lib}")
    out = subprocess.run([objdump, "-T", lib], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines() if l[:1].isalnum() and l.split()[0].strip("0123456789abcdef") == ""]
    defined = [r[-1] for r in rows if "*UND*" not in r]
    if twin.entry not in defined:
        raise RuntimeError(f"{lib}: {twin.entry} not among the dynamic symbols {defined[:5]}")
    bad = [s for s in defined if not s.startswith(twin.prefix)]
    if bad:
        raise RuntimeError(f"{lib} exports {bad[:5]} ({len(bad)} symbols besides {twin.prefix}*): these could bind "
                           "across libtbls_gpu.so")


def build(twin):
    """Build `twin` (a Twin, or the name of one in TWINS) if its output is
    stale; the output's path."""
    twin = TWINS[twin] if isinstance(twin, str) else twin
    if not stale(twin):
        return twin.out
    *compiles, link = commands(twin)  # (a host twin: one command, compile and link)
    tmp = link[-1]
    try:
        if twin.kind == "device":
            with ThreadPoolExecutor(max_workers=len(compiles)) as ex:
                list(ex.map(_run, compiles))
            for obj in _objects(twin):
                _native().check_return_address(obj)
        _run(link)
        if twin.kind == "device":
            check_exports(twin, tmp)
        os.replace(tmp, twin.out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return twin.out


def build_all(jobs=MAX_COMPILERS):
    """Build every stale twin of TWINS but tools/count_work.py's variants,
    `jobs` at a time; [(name, exception)] of those that failed."""
    def one(twin):
        try:
            build(twin)
        except Exception as e:
            return twin.name, e
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        return [r for r in ex.map(one, [t for t in TWINS.values() if t.prebuild]) if r]


_libs = {}


def lib(twin, signatures=None):
    """The twin's library, built if stale and loaded once per output;
    `signatures(lib)` sets the package's ctypes signatures on first load."""
    twin = TWINS[twin] if isinstance(twin, str) else twin
    if twin.out not in _libs:
        L = ctypes.CDLL(build(twin))
        if signatures:
            signatures(L)
        _libs[twin.out] = L
    return _libs[twin.out]
