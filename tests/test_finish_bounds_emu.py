"""Sanitizer runs of the finished graph (CPU only, stand-alone programs with their own main):
  finish_host.cpp alone (with gfa_writer.cpp for the text) in tests/c_client/finish_host_check.cpp, and
  kernels_finish.inc: the emulation linked into tests/c_client/finish_bounds_check.cpp with the guarded arena of csrc/device_rt.hpp
  (AC_ARENA_GUARD: exact sizes and red zones; level 2 also poisons rewound memory), from the per-level objects of `make kernel_bounds_check`,
both under the address and undefined-behaviour sanitizers.  Named cases, planted graphs and the tie-group boundary table of
test_finish_emu.py are replayed at both levels: exit status 0, no sanitizer report, and every result equal to the model's.
`make finish_bounds_check` in csrc builds the same programs."""
import fcntl
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bounds_cases as B
import emu_lib
import finish_util as F
import subset_util as S
from test_finish_emu import GROUP_SIZES, boundary_unitigs, planted_case

LEVELS = [1, 2]


def test_host_functions_stand_alone(tmp_path):
    root = emu_lib.ROOT
    exe = tmp_path / "finish_host_check"
    csrc = root / "autocycler_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(csrc),
                           str(root / "tests" / "c_client" / "finish_host_check.cpp"), str(csrc / "finish_host.cpp"), str(csrc / "gfa_writer.cpp"), "-o", str(exe),
                           "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "finish_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = B.GUARD_DIR / f"finish_bounds_check_l{level}"
    srcs = list(B.CSRC.glob("*.[ch]*")) + list(B.CSRC.glob("*.inc")) + [B.ROOT / "include" / "autocycler_hip.h", B.CSRC / "Makefile",
                                                                    B.ROOT / "tests" / "c_client" / "finish_bounds_check.cpp"]
    B.GUARD_DIR.mkdir(parents=True, exist_ok=True)
    with open(B.GUARD_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in srcs):
            subprocess.check_call(["make", "-j", "8", "-C", str(B.CSRC), str(Path("../../tests/_emu/guard") / exe.name)], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module", params=LEVELS, ids=lambda l: f"guard{l}")
def exe(request):
    return driver(request.param)


REC = np.dtype([("number", "<u4"), ("source", "<u4"), ("length", "<u8"), ("seq_off", "<u8"), ("depth", "<f8"), ("type", "u1")], align=True)
PER_GROUP = 9


def unpack(outs, group):
    """one group of the driver's outputs in the model's form, and its text and counts"""
    o = outs[PER_GROUP * group:PER_GROUP * (group + 1)]
    rec, seq = np.frombuffer(o[0], dtype=REC), bytes(o[1])
    unitigs = [(int(u["number"]), int(u["source"]), seq[int(u["seq_off"]):int(u["seq_off"]) + int(u["length"])], float(u["depth"]), int(u["type"])) for u in rec]
    pseq, poff, pent = np.frombuffer(o[4], dtype="<u4").tolist(), np.frombuffer(o[5], dtype="<u8").tolist(), np.frombuffer(o[6], dtype="<i4").tolist()
    got = dict(unitigs=unitigs, new_of_old=np.frombuffer(o[2], dtype="<u4").tolist(), links=[tuple(l) for l in np.frombuffer(o[3], dtype="<i4").reshape(-1, 2).tolist()],
               paths={s: pent[poff[i]:poff[i + 1]] for i, s in enumerate(pseq)})
    return got, bytes(o[7]), np.frombuffer(o[8], dtype="<u8").tolist()


def seq_block(seqs):
    begin = np.zeros(max(len(seqs), 1), dtype=np.uint64)[:len(seqs)]
    if len(seqs) > 1:
        begin[1:] = np.cumsum([len(s) for s in seqs[:-1]], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), begin      # (an exact block: no byte behind the last unitig)


def add_merge_call(calls, case, renumber, label):
    graph, _ = F.model_graph(**case)
    exp, _ = F.finish_model(graph, case["n"], renumber)
    exp["paths"] = {}
    text = F.save_gfa(exp, 5, use_other_colour=True)
    sb, sg = seq_block(case["seqs"])

    def check(outs, label):
        assert len(outs) == PER_GROUP
        got, got_text, _ = unpack(outs, 0)
        F.assert_model_same(got, exp, label)
        assert got_text == text, label
    calls.add("finish", [case["n"], len(case["links"]), len(case["path_ends"]), int(renumber), 0, 0],
              [B.arr(np.asarray(case["links"], dtype=np.int32).reshape(-1, 2), np.int32), B.arr(case["lens"], np.uint32), B.arr(case["alive"], np.uint8),
               B.arr(case["depths"], np.float64), B.arr(case["types"], np.uint8), sb.tobytes(), sg.tobytes(),
               B.arr(np.asarray(case["path_ends"], dtype=np.int32).reshape(-1, 2), np.int32), b"", b"", b""], check, label=label)


def planted_calls():
    """planted graphs with every kind of self link, types, alive masks and ties (those without positions: the driver gives none), renumber 0 and 1"""
    calls, rng = B.Calls(), random.Random(41)
    while len(calls.records) < 40:
        case = planted_case(rng)
        if case["fwd"] is not None:
            continue
        for renumber in (False, True):
            add_merge_call(calls, case, renumber, f"planted {len(calls.records)} renumber {int(renumber)}")
    return calls


def boundary_calls():
    """unlinked unitigs: tie groups of 1, 2, 63 ... 65 items at sizes around the sort and scan tiles, against sorted()"""
    calls = B.Calls()
    for n in (65, 257, 2049, 4097):
        for group in GROUP_SIZES:
            if group > n:
                continue
            seqs, depths = boundary_unitigs(n, group, seed=n * 100 + group)
            want = F.expected_order(seqs, depths)
            sb, sg = seq_block(seqs)

            def check(outs, label, want=want, seqs=seqs):
                got, _, counts = unpack(outs, 0)
                assert [u[1] for u in got["unitigs"]] == want and [u[2] for u in got["unitigs"]] == [seqs[s - 1] for s in want], label
                assert counts[1] == 3, label
            calls.add("finish", [n, 0, 0, 1, 0, 0], [b"", B.arr([len(s) for s in seqs], np.uint32), b"", B.arr(depths, np.float64), b"", sb.tobytes(), sg.tobytes(), b"", b"", b"", b""],
                      check, label=f"{n} unitigs, groups of {group}")
    return calls


def named_calls():
    """test_gfa_14 through the subsets: every single-sequence subset and every subset that leaves one out, renumber 0 and 1, with the P lines"""
    calls = B.Calls()
    g = S.gfa_14()
    n_seqs = len(g["paths"])
    entries = [e for p in g["paths"] for e in p]
    off = np.concatenate([[0], np.cumsum([len(p) for p in g["paths"]])])
    sb, sg = seq_block(g["seqs"])
    subsets = [[int(s == keep) for s in range(n_seqs)] for keep in range(n_seqs)] + [[int(s != out) for s in range(n_seqs)] for out in range(n_seqs)] + \
        [list(range(1, n_seqs + 1))]
    for labels in subsets:
        nc = max(1, max(labels))
        for renumber in (False, True):
            def check(outs, label, labels=labels, nc=nc, renumber=renumber):
                assert len(outs) == PER_GROUP * nc
                for c in range(1, nc + 1):
                    m = S.model_cluster(g["n"], g["links"], g["lens"], g["alive"], g["paths"], labels, c)
                    exp_plan = S.model_merge(m, g["seqs"])
                    graph, _ = F.model_graph(m["n"], m["links"], m["lens"], m["alive"], m["path_ends"], m["depth"], m["fwd"], m["rev"], None, g["seqs"])
                    exp, _ = F.finish_model(graph, g["n"], renumber, S.model_merged_paths(m, exp_plan))
                    got, text, _ = unpack(outs, c - 1)
                    F.assert_model_same(got, exp, label)
                    assert text == F.save_gfa(exp, 5, [(s, s + 1, 100 + s, f"seq_{s}", f"seq_{s}", c) for s in m["seqs"]], use_other_colour=True), label
            calls.add("finish", [g["n"], len(g["links"]), 0, int(renumber), n_seqs, nc],
                      [B.arr(np.asarray(g["links"], dtype=np.int32).reshape(-1, 2), np.int32), B.arr(g["lens"], np.uint32), B.arr(g["alive"], np.uint8), b"", b"", sb.tobytes(),
                       sg.tobytes(), b"", B.arr(entries, np.int32), B.arr(off, np.uint64), B.arr(labels, np.uint16)], check, label=f"test_gfa_14 {labels} renumber {int(renumber)}")
    return calls


_GROUPS = {}      # (one cached list per group: the expected values are computed once and serve both levels)


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


def test_named_cases(exe, tmp_path):
    assert _calls("named", named_calls).run(exe, tmp_path) > 10


def test_planted_graphs(exe, tmp_path):
    assert _calls("planted", planted_calls).run(exe, tmp_path) == 40


def test_boundary_table(exe, tmp_path):
    assert _calls("boundary", boundary_calls).run(exe, tmp_path) == 20
