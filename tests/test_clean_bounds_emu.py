"""Sanitizer runs of `autocycler clean`'s edit (CPU only, stand-alone programs with their own main):
  clean_host.cpp alone (with gfa_writer.cpp for the text) in tests/c_client/clean_host_check.cpp, and
  kernels_clean.inc: the emulation linked into tests/c_client/clean_bounds_check.cpp with the guarded arena of csrc/device_rt.hpp
  (AC_ARENA_GUARD: exact sizes and red zones; level 2 also poisons rewound memory), from the per-level objects of `make kernel_bounds_check`,
both under the address and undefined-behaviour sanitizers.  The named cases and the boundary table of test_clean_emu.py are replayed at both
levels: exit status 0, no sanitizer report, and every result equal to the model's — the tile, key-width, multi-arm and dense rows included, with
the counts that make them those rows (check_row); a buffer sized by the links, the edited entries or n_out would be overrun at a tile's edge.
`make clean_bounds_check` in csrc builds the same programs.
Nothing is loaded into Python and nothing is preloaded."""
import fcntl
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bounds_cases as B
import clean_util as CU
import emu_lib
from test_clean_emu import K, TEXTS_MAX, boundary_cases, boundary_expected, check_row, hub_case, named_cases, run_model, run_model_fast

LEVELS = [1, 2]
# the rounds between two read-backs, from the source (test_clean_emu.py reads the same number from the library's summary)
BATCH = int(re.search(r"CLEAN_ROUNDS_PER_BATCH = (\d+);", (B.CSRC / "clean_host.hpp").read_text()).group(1))


def test_host_functions_stand_alone(tmp_path):
    root = emu_lib.ROOT
    exe = tmp_path / "clean_host_check"
    csrc = root / "autocycler_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(csrc),
                           str(root / "tests" / "c_client" / "clean_host_check.cpp"), str(csrc / "clean_host.cpp"), str(csrc / "gfa_writer.cpp"), "-o", str(exe),
                           "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "clean_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = B.GUARD_DIR / f"clean_bounds_check_l{level}"
    srcs = list(B.CSRC.glob("*.[ch]*")) + list(B.CSRC.glob("*.inc")) + [B.ROOT / "include" / "autocycler_hip.h", B.CSRC / "Makefile",
                                                                    B.ROOT / "tests" / "c_client" / "clean_bounds_check.cpp"]
    B.GUARD_DIR.mkdir(parents=True, exist_ok=True)
    with open(B.GUARD_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in srcs):
            subprocess.check_call(["make", "-j", "8", "-C", str(B.CSRC), str(Path("../../tests/_emu/guard") / exe.name)], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module", params=LEVELS, ids=lambda l: f"guard{l}")
def exe(request):
    return driver(request.param)


def seq_block(seqs):
    begin = np.zeros(max(len(seqs), 1), dtype=np.uint64)[:len(seqs)]
    if len(seqs) > 1:
        begin[1:] = np.cumsum([len(s) for s in seqs[:-1]], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), begin      # (an exact block: no byte behind the last unitig)


def add_call(calls, case, label, exp=None, facts=None):
    """exp, facts: a row of the boundary table brings its model and what check_row holds it to; the rows above TEXTS_MAX unitigs go without texts"""
    exp = run_model(case) if exp is None else exp
    nan = CU.has_nan_alive(exp)
    texts = 0 if nan or case["n"] > TEXTS_MAX else 1 if CU.is_multiset(exp) else 2
    name = label
    want_edited = CU.cleaned_text(exp, K, True) if texts >= 1 else b""
    want_final = CU.final_text(exp, K) if texts >= 2 else b""
    sb, sg = seq_block(case["seqs"])
    begin = sg.tolist()

    def check(outs, label):
        assert len(outs) == 11
        got = dict(len=np.frombuffer(outs[0], dtype="<u4").tolist(), alive=list(outs[1]), type=list(outs[3]), copy_of=np.frombuffer(outs[4], dtype="<u4").tolist(),
                   reason=list(outs[5]), links=[tuple(l) for l in np.frombuffer(outs[6], dtype="<i4").reshape(-1, 2).tolist()])
        for key in got:
            assert got[key] == exp[key], (label, key, got[key], exp[key])
        assert bytes(outs[2]) == np.asarray(exp["depth"], dtype=np.float64).tobytes(), (label, "depth")
        assert np.frombuffer(outs[7], dtype="<u8").tolist() == [begin[(c or u + 1) - 1] for u, c in enumerate(exp["copy_of"])], (label, "seq_begin")
        assert bytes(outs[8]) == want_edited and bytes(outs[9]) == want_final, (label, "texts")
        rounds = int(np.frombuffer(outs[10], dtype="<u8")[0])
        if name.startswith("chain of"):
            assert rounds == case["n"], label
        if facts is not None:
            check_row(name, case, facts, rounds, BATCH)
    calls.add("clean", [case["n"], len(case["links"]), len(case["remove"]), len(case["duplicate"]), int(case["min_depth"] is not None),
                        B.f64_bits(case["min_depth"] if case["min_depth"] is not None else 0.0), texts],
              [B.arr(np.asarray(case["links"], dtype=np.int32).reshape(-1, 2), np.int32), B.arr(case["lens"], np.uint32), B.arr(case["depths"], np.float64),
               B.arr(case["types"], np.uint8), B.arr(case["alive"], np.uint8), sb.tobytes(), sg.tobytes(), B.arr(sorted(case["remove"]), np.uint32),
               B.arr(sorted(case["duplicate"]), np.uint32)], check, label=label)


def named_calls():
    calls = B.Calls()
    for name, case in named_cases().items():
        add_call(calls, case, name)
    return calls


def boundary_calls():
    calls = B.Calls()
    for name, case in boundary_cases(BATCH).items():
        add_call(calls, case, name, *boundary_expected(BATCH, name))
    return calls


_GROUPS = {}      # (one cached list per group: the expected values are computed once and serve both levels)


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


def test_named_cases(exe, tmp_path):
    assert _calls("named", named_calls).run(exe, tmp_path) == len(named_cases())


def test_boundary_table(exe, tmp_path):
    assert _calls("boundary", boundary_calls).run(exe, tmp_path) == len(boundary_cases(BATCH))


def hub_calls():
    calls, hub = B.Calls(), hub_case(4097)
    add_call(calls, hub, "hub of degree 4097", run_model_fast(hub))
    return calls


def test_hub_of_degree_4097(exe, tmp_path):
    """not a row of the table (the device is spared its 9258 launches): a range off[2u] .. off[2u + 2] of 4097 entries and 513 batches, 6 s per level"""
    assert _calls("hub", hub_calls).run(exe, tmp_path) == 1
