"""Sanitizer runs of combine (CPU only, stand-alone programs with their own main):
  combine_host.cpp alone in tests/c_client/combine_host_check.cpp, and
  kernels_combine.inc with the flag stage of kernels_components.inc it calls: the emulation linked into tests/c_client/combine_bounds_check.cpp
  with the guarded arena of csrc/device_rt.hpp (AC_ARENA_GUARD: exact sizes and red zones; level 2 also poisons rewound memory), from the
  per-level objects of `make kernel_bounds_check`,
both under the address and undefined-behaviour sanitizers.  The named cases and the boundary table of test_combine_emu.py are replayed at both
levels: exit status 0, no sanitizer report, and every result equal to the model's.  `make combine_bounds_check` and `make combine_host_check`
in csrc build the same programs.  Nothing is loaded into Python and nothing is preloaded."""
import fcntl
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bounds_cases as B
import combine_util as CU
import emu_lib
from autocycler_amd import _capi
from test_combine_emu import RADIX_TILE, SCAN_TILE, chain_graph, link_count_graph, named_cases, one_tig, read_depth_cases

LEVELS = [1, 2]


def test_host_functions_stand_alone(tmp_path):
    root = emu_lib.ROOT
    exe = tmp_path / "combine_host_check"
    csrc = root / "autocycler_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(csrc),
                           str(root / "tests" / "c_client" / "combine_host_check.cpp"), str(csrc / "combine_host.cpp"), str(csrc / "components_host.cpp"), "-o", str(exe),
                           "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "combine_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = B.GUARD_DIR / f"combine_bounds_check_l{level}"
    srcs = list(B.CSRC.glob("*.[ch]*")) + list(B.CSRC.glob("*.inc")) + [B.ROOT / "include" / "autocycler_hip.h", B.CSRC / "Makefile",
                                                                    B.ROOT / "tests" / "c_client" / "combine_bounds_check.cpp"]
    B.GUARD_DIR.mkdir(parents=True, exist_ok=True)
    with open(B.GUARD_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in srcs):
            subprocess.check_call(["make", "-j", "8", "-C", str(B.CSRC), str(Path("../../tests/_emu/guard") / exe.name)], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module", params=LEVELS, ids=lambda l: f"guard{l}")
def exe(request):
    return driver(request.param)


def add_call(calls, texts, read_depths, label):
    models = [CU.from_gfa_text(t) for t in texts]
    exp = CU.combine_model(models, read_depths)
    forms = [CU.array_form(m) for m in models]
    sizes = [len(f["number"]) for f in forms]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    loff = np.concatenate([[0], np.cumsum([len(f["links"]) for f in forms])]).astype(np.uint64)
    flat = lambda key: [x for f in forms for x in f[key]]
    seqs = flat("seqs")
    begin = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)[:len(seqs)]
    rd = None if read_depths is None else [0.0 if x is None else x for g in read_depths for x in g]
    has = None if read_depths is None else [x is not None for g in read_depths for x in g]
    n = sum(sizes)

    def check(outs, label):
        assert len(outs) == 8
        clusters = np.frombuffer(outs[0], dtype=np.dtype(_capi.CombinedCluster))
        unitigs = np.frombuffer(outs[1], dtype=np.dtype(_capi.CombinedUnitig))
        links = np.frombuffer(outs[2], dtype="<i4").reshape(-1, 2)
        counts = np.frombuffer(outs[7], dtype="<u8").tolist()
        m = exp["metrics"]
        got = type("Got", (), dict(clusters=clusters, unitigs=unitigs, links=links,
                                   summary=dict(bases=counts[2], unitigs=counts[3], fully_resolved=bool(counts[4]), graphs=len(texts), links=len(exp["links"]))))
        CU.assert_same(got, exp, _capi.TOPOLOGY_NAMES, label)
        assert (bytes(outs[3]), bytes(outs[4]), bytes(outs[5]), bytes(outs[6])) == (exp["gfa"], exp["fasta"], exp["yaml"], exp["depth_lines"]), (label, "texts")
        assert counts[1] == (2 if n else 0) and counts[2] == m["consensus_assembly_bases"], (label, counts)
    # exact blocks: nothing behind the last element of any array (an empty array is a null pointer; the library must not need it)
    calls.add("combine", [len(texts)],
              [uoff.tobytes(), loff.tobytes(), B.arr(flat("number"), np.uint32), B.arr(flat("len"), np.uint32), B.arr(flat("depth"), np.float64), B.arr(flat("type"), np.uint8),
               B.arr(np.asarray(flat("links"), dtype=np.int32).reshape(-1, 2), np.int32), B.arr(rd, np.float64), B.arr(has, np.uint8),
               (b"".join(seqs) or b"\0") if n else b"", begin.tobytes() if n else b""], check, label=label)


def named_table():
    table = {name: (texts, None) for name, texts in named_cases().items()}
    table.update(read_depth_cases())
    return table


def boundary_table():
    table = {}
    for G in (1, 2, 63, 64, 65):
        table[f"G = {G}"] = ([one_tig(1 + g % 3, 5 + (g * 7) % 11, [(1 + g % 3, 1 + g % 3), (-(1 + g % 3), -(1 + g % 3))] if g % 2 else [], tag=g) for g in range(G)], None)
    for n in (1, 63, 64, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        table[f"{n} unitigs"] = ([one_tig(1, 2), chain_graph(n, first=3, step=2, closed=n % 2 == 0), one_tig(9, 3, [(9, -9)])], None)
    for nl in (RADIX_TILE - 3, RADIX_TILE - 2, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1):
        table[f"{nl} links"] = ([link_count_graph(nl), one_tig(1, 7)], None)
    return table


def _make(table):
    def make():
        calls = B.Calls()
        for name, (texts, rd) in table().items():
            add_call(calls, texts, rd, name)
        return calls
    return make


_GROUPS = {}      # (one cached list per group: the expected values are computed once and serve both levels)


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


def test_named_cases(exe, tmp_path):
    assert _calls("named", _make(named_table)).run(exe, tmp_path) == len(named_table())


def test_boundary_table(exe, tmp_path):
    assert _calls("boundary", _make(boundary_table)).run(exe, tmp_path) == len(boundary_table())
