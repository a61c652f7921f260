"""The library's environment switches (brdf_amd/csrc/fit_switches.h) and method codes (fit_host.h: method_spec), on the CPU.

tests/cpp/fit_switches_harness.cpp is compiled here with g++ (no HIP).  Every switch of the table is read with the variable
unset and set to "0", "1", "01", "7", "-3", "999" and "", and the answer compared with the switch's documented rule, written
out below independently of the header; then the variable is changed between two reads (no reader caches)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brdf_amd", "csrc")
VALUES = [None, "0", "1", "01", "7", "-3", "999", ""]
MAX_CAND = 8              # lm_machine.h: kMaxCand
MAX_REPLICAS = 8          # resident_fit_impl.h: kReplicas
SPIN_TICKS = 200000000    # resident_fit_impl.h: kSpinBudgetTicks
BIG = 2 ** 31 - 1


def _atoi(v):
    m = re.match(r"\s*([+-]?\d+)", v)
    return int(m.group(1)) if m else 0


def _clamped(lo, hi, unset):
    return lambda v: unset if v is None else min(hi, max(lo, _atoi(v)))


def _on_unless_0(v):
    return 0 if v is not None and v[:1] == "0" else 1


def _off_unless_1(v):
    return 1 if v is not None and v[:1] == "1" else 0


def _rows(v):  # bit 0: dlevmar_dif takes the rows kernel, bit 1: dlevmar_bc_dif does
    return 0 if (v or "")[:1] == "0" else (3 if (v or "")[:1] == "1" else 1)


RULES = {
    "BRDF_HIP_RESIDENT": _on_unless_0, "BRDF_HIP_CHANNELS": _on_unless_0, "BRDF_HIP_LANE": _on_unless_0,
    "BRDF_HIP_BATCH_BIG": _on_unless_0, "BRDF_HIP_DIF_FUSED": _on_unless_0, "BRDF_HIP_SPEC_JAC": _on_unless_0,
    "BRDF_HIP_COSINES_ROWS": _on_unless_0,
    "BRDF_HIP_EXACT_POW": _off_unless_1, "BRDF_HIP_STATS_FAST": _off_unless_1,
    "BRDF_HIP_ROWS": _rows,
    "BRDF_HIP_PG_MULTI": _clamped(1, MAX_CAND, MAX_CAND), "BRDF_HIP_DIF_CHAIN": _clamped(1, MAX_CAND, MAX_CAND),
    "BRDF_HIP_BATCH_DIF_CHAIN": _clamped(1, MAX_CAND, MAX_CAND),  # unset: BRDF_HIP_DIF_CHAIN's value (its own test below)
    "BRDF_HIP_LANE_WAVES": lambda v: _atoi(v) if v is not None and _atoi(v) in (2, 4) else 1,
    "BRDF_HIP_LANE_QUORUM": _clamped(1, BIG, 24), "BRDF_HIP_LANE_MAXWAIT": _clamped(0, BIG, 6),
    "BRDF_HIP_RESIDENT_REPLICAS": _clamped(1, MAX_REPLICAS, MAX_REPLICAS),
    "BRDF_HIP_RESIDENT_SPIN_MS": lambda v: SPIN_TICKS if v is None else max(1, _atoi(v)) * 100000,
    "BRDF_HIP_RESIDENT_SABOTAGE": _clamped(-BIG, BIG, -1),
    "BRDF_HIP_RESIDENT_BACKOFF": _clamped(0, BIG, -1),  # unset (-1): the workspace's own doubling back-off
    "BRDF_HIP_RESIDENT_TRACE_EPOCH": _clamped(-BIG, BIG, 20),  # read by diagnostic builds (BRDF_STAMPS) only
    "BRDF_HIP_STEP_DUMP": lambda v: 0 if v is None else 1,       # a file name, diagnostic builds only: set or not
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("fit_switches") / "libfit_switches_harness.so"
    subprocess.run(["g++", "-O2", "-fPIC", "-std=c++17", "-Wall", "-Werror", "-shared", "-o", str(out),
                    os.path.join(ROOT, "tests", "cpp", "fit_switches_harness.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.fsw_name.restype = lib.fsw_meaning.restype = C.c_char_p
    lib.fsw_read.restype = C.c_longlong
    lib.fsw_read.argtypes = [C.c_int, C.c_int, C.c_longlong]
    return lib


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _read(lib, i):
    return lib.fsw_read(i, MAX_REPLICAS, SPIN_TICKS)


def _names(lib):
    return [lib.fsw_name(i).decode() for i in range(lib.fsw_count())]


def test_the_table_lists_every_switch_once_with_a_meaning(harness):
    names = _names(harness)
    assert sorted(names) == sorted(RULES), set(names) ^ set(RULES)
    assert all(len(harness.fsw_meaning(i)) > 10 for i in range(len(names)))
    # ... and nothing else in the library's sources reads the environment or names a switch the table does not have
    for f in sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))):
        text = open(os.path.join(CSRC, f)).read()
        if f != "fit_switches.h":
            assert "getenv" not in text, f
        assert set(re.findall(r"BRDF_HIP_[A-Z_]*[A-Z]", text)) <= set(names) | {"BRDF_HIP_LIB"}, f


def test_every_switch_follows_its_rule(harness, monkeypatch):
    names = _names(harness)
    for name in names:
        monkeypatch.delenv(name, raising=False)
    for i, name in enumerate(names):
        for value in VALUES + ["2", "4", " 5", "1x"]:
            _set(monkeypatch, name, value)
            got, want = _read(harness, i), RULES[name](value)
            print(f"{name}={value!r}: {got}")
            assert got == want, (name, value, got, want)
        monkeypatch.delenv(name)


def test_batch_dif_chain_follows_dif_chain_when_unset(harness, monkeypatch):
    names = _names(harness)
    i = names.index("BRDF_HIP_BATCH_DIF_CHAIN")
    monkeypatch.delenv("BRDF_HIP_BATCH_DIF_CHAIN", raising=False)
    for value in VALUES:
        _set(monkeypatch, "BRDF_HIP_DIF_CHAIN", value)
        assert _read(harness, i) == RULES["BRDF_HIP_DIF_CHAIN"](value), value
    monkeypatch.setenv("BRDF_HIP_DIF_CHAIN", "3")
    monkeypatch.setenv("BRDF_HIP_BATCH_DIF_CHAIN", "5")
    assert _read(harness, i) == 5 and _read(harness, names.index("BRDF_HIP_DIF_CHAIN")) == 3


def test_no_reader_caches(harness, monkeypatch):
    """a process may change a switch between two fits (the GPU tests do): unset -> "0" -> "1" -> "2" -> unset, read each time"""
    changes = (None, "0", "1", "2", None)
    for i, name in enumerate(_names(harness)):
        seen = []
        for value in changes:
            _set(monkeypatch, name, value)
            seen.append(_read(harness, i))
        assert seen == [RULES[name](v) for v in changes], (name, seen)
        assert len(set(seen)) > 1, (name, seen)  # (the answers do differ: the check is not vacuous)


def test_method_spec(harness):
    """the C ABI's BRDF_METHOD_* (0 dif, 1 bc_dif, 2 bc_der, 3 der) -> the kernels' machine (0 Dif, 1 Bc, 2 Der) + analytic"""
    want = {0: (0, 0), 1: (1, 0), 2: (1, 1), 3: (2, 1)}
    for method in range(-1, 5):
        machine, analytic = C.c_int(-7), C.c_int(-7)
        known = harness.fsw_method_spec(method, C.byref(machine), C.byref(analytic))
        assert known == (1 if method in want else 0), method
        # an unknown code travels on unchanged, for the entry points whose own check words the error
        assert (machine.value, analytic.value) == want.get(method, (method, 0)), method
