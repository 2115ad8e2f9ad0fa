"""tests/twin_build.py, the one builder of the test twins, on a throw-away twin
in tmp_path (a three-line source exporting one function): when it builds, when
it does not, what a failed or a concurrent build leaves behind -- and the
table itself: every twin source under tests/*/ is claimed once, every path
exists, the device twins take the engine's own flag lists.
"""
import ctypes
import glob
import os
import subprocess
import sys

import pytest

from tests import twin_build as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = 'extern "C" int answer() {\n    return %d;\n}\n'


@pytest.fixture
def twin(tmp_path, monkeypatch):
    """A fresh host twin with one declared dependency, and a stand-in for the builder module."""
    (tmp_path / "answer.cpp").write_text(SOURCE % 42)
    (tmp_path / "answer.h").write_text("// a declared dependency\n")
    (tmp_path / "builder.py").write_text("# stands for tests/twin_build.py\n")
    monkeypatch.setattr(tb, "BUILDER", str(tmp_path / "builder.py"))
    return tb.Twin("answer", "host", (str(tmp_path / "answer.cpp"),), str(tmp_path / "libanswer.so"),
                   ("-O1", "-fPIC", "-shared"), deps=(str(tmp_path / "answer.h"),))


def ran(twin):
    """The commands the builder has run for this twin so far."""
    return [c for c in tb.RAN if twin.sources[0] in c]


def answer(path):
    return ctypes.CDLL(path).answer()  # (no test loads one path twice: dlopen would hand back the first load)


def test_fresh_build_loads_and_answers(twin):
    assert tb.stale(twin)
    assert tb.lib(twin).answer() == 42
    assert len(ran(twin)) == 1 and not tb.stale(twin)
    assert tb.lib(twin) is tb.lib(twin)  # loaded once per output


def test_second_build_runs_nothing(twin):
    tb.build(twin)
    n = len(tb.RAN)
    assert tb.build(twin) == twin.out
    assert len(tb.RAN) == n


@pytest.mark.parametrize("which", ["source", "dependency", "builder"])
def test_a_newer_input_rebuilds(twin, which):
    tb.build(twin)
    path = {"source": twin.sources[0], "dependency": twin.deps[0], "builder": tb.BUILDER}[which]
    future = os.path.getmtime(twin.out) + 100
    os.utime(path, (future, future))
    assert tb.stale(twin)
    tb.build(twin)
    assert len(ran(twin)) == 2


def test_commands_are_what_build_runs(twin):
    expected = tb.commands(twin)
    tb.build(twin)
    assert ran(twin) == expected
    assert expected[0][-1] != twin.out and expected[0][-1].startswith(twin.out)  # a temporary name beside it


def test_failed_compile_keeps_the_previous_library(twin, tmp_path):
    tb.build(twin)
    with open(twin.sources[0], "w") as f:
        f.write("this is not C++\n")
    future = os.path.getmtime(twin.out) + 100
    os.utime(twin.sources[0], (future, future))
    with pytest.raises(subprocess.CalledProcessError):
        tb.build(twin)
    assert answer(twin.out) == 42
    assert [f for f in os.listdir(tmp_path) if f.startswith("libanswer.so")] == ["libanswer.so"]


def test_failed_compile_leaves_no_output(twin, tmp_path):
    with open(twin.sources[0], "w") as f:
        f.write("this is not C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        tb.build(twin)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("libanswer.so")]


CHILD = """
import sys
from tests import twin_build as tb
d = sys.argv[1]
tb.BUILDER = d + "/builder.py"
twin = tb.Twin("answer", "host", (d + "/answer.cpp",), d + "/libanswer.so", ("-O1", "-fPIC", "-shared"))
tb.stale = lambda twin: True  # both children compile and move into place, whichever starts first
assert tb.lib(twin).answer() == 42
assert len(tb.RAN) == 1
"""


def test_concurrent_builds_both_load(twin, tmp_path):
    kids = [subprocess.Popen([sys.executable, "-c", CHILD, str(tmp_path)], cwd=ROOT, stderr=subprocess.PIPE, text=True)
            for _ in range(2)]
    for k in kids:
        err = k.communicate(timeout=120)[1]
        assert k.returncode == 0, err
    assert answer(twin.out) == 42
    assert os.listdir(tmp_path).count("libanswer.so") == 1
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]


def test_table_claims_every_twin_source_once():
    """Every *.cpp / *.hip under tests/*/ (tests/cabi has its own Makefile) is the
    source of exactly one twin (tools/count_work.py's variants build a twin's
    source again and are not counted) or, if of none, a declared dependency of
    exactly one; every path the table names exists."""
    files = [f for ext in ("cpp", "hip") for f in glob.glob(os.path.join(ROOT, "tests", "*", "*." + ext))
             if os.path.basename(os.path.dirname(f)) != "cabi"]
    assert len(files) >= 23  # (16 host sources and 7 device sources when this test was written)
    primary = [t for t in tb.TWINS.values() if not t.variant_of]
    for f in files:
        owners = [t.name for t in primary if f in t.sources] or [t.name for t in primary if f in t.deps]
        assert len(owners) == 1, (f, owners)
    for t in tb.TWINS.values():
        assert t.kind in ("host", "device") and tb.TWINS[t.name] is t
        for path in tb.dependencies(t):
            assert os.path.exists(path), (t.name, path)
        assert os.path.isdir(os.path.dirname(t.out))
        if t.variant_of:
            assert tb.TWINS[t.variant_of].sources == t.sources and tb.TWINS[t.variant_of].out != t.out
    outs = [t.out for t in tb.TWINS.values()]
    assert len(set(outs)) == len(outs)


def test_device_twins_take_the_engines_flags(monkeypatch):
    """The common compile flags and the link flags are _native's own lists,
    the per-unit flags those of the product unit the table names."""
    from charon_amd import _native
    hipcc = "/somewhere/hipcc"
    monkeypatch.setattr(_native, "_hipcc", lambda: hipcc)  # (nothing is run)
    device = [t for t in tb.TWINS.values() if t.kind == "device"]
    assert sorted(t.name for t in device) == ["devcheck", "devcheck_hexline", "devcheck_hlines"]
    n = len(_native.COMMON_FLAGS)
    for t in device:
        *compiles, link = tb.commands(t)
        assert len(compiles) == len(t.sources)
        for src, cmd in zip(t.sources, compiles):
            unit = t.units.get(os.path.basename(src))
            assert unit is None or os.path.exists(os.path.join(tb.CSRC, unit))
            assert cmd[0] == hipcc and cmd[1:1 + n] == _native.COMMON_FLAGS
            assert cmd[1 + n:-4] == list(_native.UNIT_FLAGS.get(unit, ())) and cmd[-4:-2] == ["-c", src]
        assert link[1:1 + len(_native.LINK_FLAGS)] == _native.LINK_FLAGS
        assert "-Wl,-Bsymbolic" in link and "-Wl,--version-script=" + t.version_script in link
        assert t.prefix and t.entry.startswith(t.prefix)
    with open(tb.__file__) as f:
        assert "--offload-arch" not in f.read()  # no copy of the list in the builder
