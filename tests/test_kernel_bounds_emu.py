"""Bounds check of the shipped kernel and stage sources (CPU only): the emulation linked into tests/c_client/kernel_bounds_check.cpp under the
address and undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (AC_ARENA_GUARD: exact sizes and red zones; level 2
also poisons rewound memory).  Every group of calls of tests/bounds_cases.py is replayed at both levels: exit status 0, no sanitizer report,
and every result equal to the oracle's or the entry's plain-Python model.  `make kernel_bounds_check` in csrc builds the same programs."""
import pytest

import bounds_cases as B

LEVELS = [1, 2]


@pytest.fixture(scope="module", params=LEVELS, ids=lambda l: f"guard{l}")
def exe(request):
    return B.driver(request.param)


def test_guard_selfcheck(exe):
    """what the arena poisons, asked of the sanitizer (nothing is dereferenced): the last byte asked for is addressable, the byte behind it and
    the red zone are not, rewound memory is poisoned at level 2 only, reset memory at both, the pinned pool's rounding tail at both"""
    out = B.run_clean([exe, "selfcheck"])
    assert "guard selfcheck" in out.stdout and ": OK" in out.stdout, out.stdout


# (one cached list of groups: the oracle's and the models' answers are computed once and serve both levels)
_GROUPS = {}


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


@pytest.mark.parametrize("ks", [B.BUILD_KS[:5], B.BUILD_KS[5:10], B.BUILD_KS[10:]], ids=lambda ks: "k" + "_".join(map(str, ks)))
def test_host_entry_build(exe, tmp_path, ks):
    assert _calls(("build", ks), lambda: B.build_calls(ks)).run(exe, tmp_path) == len(ks) * 24


def test_host_entry_build_knobs(exe, tmp_path):
    _calls("knobs", B.knob_calls).run(exe, tmp_path)


def test_end_repair_and_device_entry(exe, tmp_path):
    _calls("device", B.device_entry_calls).run(exe, tmp_path)


def test_multi_rank_build(exe, tmp_path):
    _calls("multi", B.multi_calls).run(exe, tmp_path)


def test_distances_decompress_verify_on_gfa_handles(exe, tmp_path):
    _calls("gfa", B.gfa_calls).run(exe, tmp_path)


def test_trim(exe, tmp_path):
    _calls("trim", B.trim_calls).run(exe, tmp_path)


def test_resolve(exe, tmp_path):
    _calls("resolve", B.resolve_calls).run(exe, tmp_path)


def test_components_and_merge_plan(exe, tmp_path):
    _calls("graph", B.graph_calls).run(exe, tmp_path)


def test_cluster_tree(exe, tmp_path):
    _calls("cluster", B.cluster_calls).run(exe, tmp_path)


def test_read_depths(exe, tmp_path):
    _calls("depth", B.depth_calls).run(exe, tmp_path)
