"""Bounds check of kernels_subset.inc (CPU only): the emulation linked into tests/c_client/subset_bounds_check.cpp under the address and
undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (AC_ARENA_GUARD: exact sizes and red zones; level 2 also poisons
rewound memory), from the per-level objects of `make kernel_bounds_check`.  The named cases and the boundary table of test_subset_emu.py are
replayed at both levels: exit status 0, no sanitizer report, and every result equal to the model's or numpy's.  `make subset_bounds_check` in
csrc builds the same programs."""
import fcntl
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bounds_cases as B
import subset_util as S
from test_subset_emu import CLUSTER_COUNTS, ENTRY_COUNTS, boundary_case, special_cases

LEVELS = [1, 2]


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = B.GUARD_DIR / f"subset_bounds_check_l{level}"
    srcs = list(B.CSRC.glob("*.[ch]*")) + list(B.CSRC.glob("*.inc")) + [B.ROOT / "include" / "autocycler_hip.h", B.CSRC / "Makefile",
                                                                    B.ROOT / "tests" / "c_client" / "subset_bounds_check.cpp"]
    B.GUARD_DIR.mkdir(parents=True, exist_ok=True)
    with open(B.GUARD_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in srcs):
            subprocess.check_call(["make", "-j", "8", "-C", str(B.CSRC), str(Path("../../tests/_emu/guard") / exe.name)], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module", params=LEVELS, ids=lambda l: f"guard{l}")
def exe(request):
    return driver(request.param)


def unpack(outs, n_clusters, merge):
    """the driver's outputs of one call as numpy arrays"""
    rec_dt = np.dtype([("seqs", "<u4"), ("unitigs", "<u4"), ("entries", "<u8"), ("links", "<u8"), ("length", "<u8")], align=True)
    names = ("records", "unitig_off", "unitigs", "fwd", "rev", "link_off", "links", "seq_off", "seq_index", "ends_off", "path_ends", "counts")
    types = (rec_dt, "<u8", "<u4", "<u4", "<u4", "<u8", "<i4", "<u8", "<u4", "<u8", "<i4", "<u8")
    assert len(outs) == len(names) + (3 * n_clusters if merge else 0)
    d = {k: np.frombuffer(o, dtype=t) for k, t, o in zip(names, types, outs)}
    d["links"], d["path_ends"] = d["links"].reshape(-1, 2), d["path_ends"].reshape(-1, 2)
    d["merged"] = [(np.frombuffer(outs[12 + 3 * c], dtype="<i4"), np.frombuffer(outs[13 + 3 * c], dtype="<u8"), np.frombuffer(outs[14 + 3 * c], dtype="<i4"))
                   for c in range(n_clusters)] if merge else []
    return d


class FromDriver:
    """the unpacked outputs behind the accessors of autocycler_amd.Subsets that subset_util's comparisons use"""

    def __init__(self, d, n_clusters):
        self.d, self.n_clusters, self.records = d, n_clusters, d["records"]

    def _row(self, off, c):
        return slice(int(self.d[off][c - 1]), int(self.d[off][c]))

    def unitigs(self, c): return self.d["unitigs"][self._row("unitig_off", c)]
    def positions(self, c): return self.d["fwd"][self._row("unitig_off", c)], self.d["rev"][self._row("unitig_off", c)]
    def links(self, c): return self.d["links"][self._row("link_off", c)]
    def seqs(self, c): return self.d["seq_index"][self._row("seq_off", c)]
    def path_ends(self, c): return self.d["path_ends"][self._row("ends_off", c)]


def add_call(calls, n, links, lens, alive, entries, off, labels, n_clusters, merge, check, label):
    links = np.asarray(links, dtype=np.int32).reshape(-1, 2)
    calls.add("subsets", [n, len(links), len(off) - 1, n_clusters, int(merge)],
              [B.arr(links, np.int32), B.arr(lens, np.uint32), B.arr(alive, np.uint8), B.arr(entries, np.int32), B.arr(off, np.uint64), B.arr(labels, np.uint16)],
              check, label=label)


def boundary_calls():
    calls = B.Calls()
    for size in ENTRY_COUNTS:
        for nc in CLUSTER_COUNTS:
            n, links, lens, entries, off, labels = boundary_case(size, nc, seed=size * 1000 + nc)
            exp = S.expected_by_numpy(n, links, lens, entries, off, labels, nc)
            add_call(calls, n, links, lens, None, entries, off, labels, nc, False,
                     lambda outs, label, exp=exp, nc=nc: S.assert_numpy_same(FromDriver(unpack(outs, nc, False), nc), exp, label), f"{size} entries, {nc} clusters")
    for name, (n, links, lens, entries, off, labels), nc in special_cases():
        exp = S.expected_by_numpy(n, links, lens, entries, off, labels, nc)
        add_call(calls, n, links, lens, None, entries, off, labels, nc, False,
                 lambda outs, label, exp=exp, nc=nc: S.assert_numpy_same(FromDriver(unpack(outs, nc, False), nc), exp, label), name)
    return calls


def named_calls():
    """test_gfa_14: every single-sequence subset, every subset that leaves one out, all in one cluster, all labels 0 — with the merge plan and
    the merged paths of every cluster, held to the model"""
    calls = B.Calls()
    g = S.gfa_14()
    n_seqs = len(g["paths"])
    entries = [e for p in g["paths"] for e in p]
    off = np.concatenate([[0], np.cumsum([len(p) for p in g["paths"]])])
    subsets = [[int(s == keep) for s in range(n_seqs)] for keep in range(n_seqs)] + [[int(s != out) for s in range(n_seqs)] for out in range(n_seqs)] + \
        [[1] * n_seqs, [0] * n_seqs, list(range(1, n_seqs + 1))]
    for labels in subsets:
        nc = max(1, max(labels))

        def check(outs, label, labels=labels, nc=nc):
            d = unpack(outs, nc, True)
            sub = FromDriver(d, nc)
            for c in range(1, nc + 1):
                m = S.model_cluster(g["n"], g["links"], g["lens"], g["alive"], g["paths"], labels, c)
                assert sub.unitigs(c).tolist() == m["unitigs"] and sub.positions(c)[0].tolist() == [m["fwd"][u - 1] for u in m["unitigs"]], label
                assert [tuple(l) for l in sub.links(c).tolist()] == m["links"] and sub.seqs(c).tolist() == m["seqs"], label
                assert [tuple(e) for e in sub.path_ends(c).tolist()] == m["path_ends"], label
                exp = S.model_merge(m)
                members, moff, ment = d["merged"][c - 1]
                assert members.tolist() == [x for chain in exp["chains"] for x in chain], label
                want = S.model_merged_paths(m, exp)
                assert [ment[int(moff[i]):int(moff[i + 1])].tolist() for i in range(len(moff) - 1)] == [want[s] for s in m["seqs"]], label
        add_call(calls, g["n"], g["links"], g["lens"], g["alive"], entries, off, labels, nc, True, check, f"test_gfa_14 {labels}")
    return calls


_GROUPS = {}      # (one cached list per group: the expected values are computed once and serve both levels)


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


def test_named_cases(exe, tmp_path):
    assert _calls("named", named_calls).run(exe, tmp_path) == 9


def test_boundary_table(exe, tmp_path):
    assert _calls("boundary", boundary_calls).run(exe, tmp_path) == len(ENTRY_COUNTS) * len(CLUSTER_COUNTS) + 5
