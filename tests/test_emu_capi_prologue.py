"""What the entry points of the C ABI answer before any work starts, on the serial CPU emulation: the phase checks of a sharded build,
the refusals while a sharded build is live, and the truncating copies of the _sized getters.  The expected texts are written out
here: callers match on them, so they are part of the ABI (the entry points share one prologue and one phase-call helper)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
from autocycler_amd import _capi

K = 1      # validate_layout takes every odd k >= 1; one-base k-mers need no padding
IN_FLIGHT = "a sharded build is in flight in this process"
ANOTHER_IN_FLIGHT = "another sharded build is in flight in this process"
NULL = C.c_void_p(None)
# every phase call that needs a later phase than the first, with null buffers: the phase check answers before anything is touched
LATER_PHASE_CALLS = [
    ("ac_shard_bitmap_export", (NULL,)),
    ("ac_shard_build_novel", (NULL,)),
    ("ac_shard_sib_export", (NULL,)),
    ("ac_shard_degrees_export", (NULL,)),
    ("ac_shard_build_graph", (NULL,)),
    ("ac_shard_links_export", (NULL, NULL)),
    ("ac_shard_links_import", (NULL, NULL)),
    ("ac_shard_queries_export", (NULL,)),
    ("ac_shard_walk", (NULL,)),
    ("ac_shard_reduce_export", (NULL, NULL)),
    ("ac_shard_reduce_import", (NULL, NULL)),
    ("ac_shard_finish", (C.c_int(3), NULL)),
    ("ac_shard_paths_export", (NULL,)),
]


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(emu_lib.emu_path())


@pytest.fixture(scope="module")
def job():
    rng = np.random.default_rng(11)
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=n)) for n in (311, 257)]
    text = np.frombuffer(("$" + "$".join("." * (K - 1) + s + "." * (K - 1) for s in seqs) + "$").encode(), dtype=np.uint8).copy()
    off, p = [], 1
    for s in seqs:
        off.append(p); p += len(s) + 2 * (K - 1) + 1
    return {"seqs": seqs, "text": text, "off": off}


def shard_begin(lib, job):
    n = len(job["seqs"])
    s = C.c_void_p()
    rc = lib.ac_shard_begin(C.c_uint32(K), C.c_uint32(n), C.c_void_p(job["text"].ctypes.data), C.c_uint64(len(job["text"])), (C.c_uint64 * n)(*job["off"]),
                            (C.c_uint32 * n)(*[len(q) for q in job["seqs"]]), (C.c_uint16 * n)(*range(1, n + 1)), (C.c_uint16 * n)(*[K - 1] * n),
                            (C.c_uint16 * n)(*[K - 1] * n), C.c_uint32(n), C.c_int(0), C.byref(s))
    return rc, s


def compress_build(lib, job):
    n = len(job["seqs"])
    views = (_capi.SeqView * n)()
    keep = [("." * (K - 1) + q + "." * (K - 1)).encode() for q in job["seqs"]]
    for i, b in enumerate(keep):
        views[i].fwd, views[i].length, views[i].id = b, len(job["seqs"][i]), i + 1
    g = C.c_void_p()
    return lib.ac_compress_build(C.c_uint32(K), C.c_uint32(n), views, C.c_uint32(n), C.c_int(0), C.byref(g)), g


def test_phase_calls_name_themselves_in_the_first_phase(lib, job):
    rc, s = shard_begin(lib, job)
    assert rc == 0, lib.ac_last_error()
    try:
        for name, args in LATER_PHASE_CALLS:
            assert getattr(lib, name)(s, *args) == 1, name
            assert lib.ac_last_error().decode() == f"{name}: wrong phase"
    finally:
        lib.ac_shard_free(s)


def test_a_live_shard_refuses_other_device_users(lib, job):
    rc, s = shard_begin(lib, job)
    assert rc == 0, lib.ac_last_error()
    try:
        rc, g = compress_build(lib, job)
        assert rc == 1 and lib.ac_last_error().decode() == IN_FLIGHT
        rc, s2 = shard_begin(lib, job)
        assert rc == 1 and lib.ac_last_error().decode() == ANOTHER_IN_FLIGHT
        unitig = np.frombuffer(b"ACGTTGCATGCATGGCATCGATCGGCTA", dtype=np.uint8).copy()      # one unitig, no links
        begin, length = np.zeros(1, dtype=np.uint64), np.array([len(unitig)], dtype=np.uint32)
        graph = _capi.DepthGraph(unitig.ctypes.data, begin.ctypes.data, length.ctypes.data, 1, None, 0)
        d = C.c_void_p()
        assert lib.ac_depth_begin(C.c_uint32(11), C.byref(graph), C.c_uint32(1), C.c_int(0), C.byref(d)) == 1
        assert lib.ac_last_error().decode() == IN_FLIGHT and not d.value
    finally:
        lib.ac_shard_free(s)
    rc, g = compress_build(lib, job)
    assert rc == 0, lib.ac_last_error()
    lib.ac_free(g)


@pytest.mark.parametrize("getter,struct", [("ac_timings_get_sized", _capi.Timings), ("ac_multi_info_get_sized", _capi.MultiInfo)])
def test_sized_getters_write_no_more_than_asked(lib, job, getter, struct):
    rc, g = compress_build(lib, job)
    assert rc == 0, lib.ac_last_error()
    try:
        size, get = C.sizeof(struct), getattr(lib, getter)
        full = np.full(size + 16, 0xAB, dtype=np.uint8)
        assert get(g, C.c_void_p(full.ctypes.data), C.c_size_t(size)) == size
        assert (full[size:] == 0xAB).all()
        for out_size in (0, 4, 12, size - 8, size - 1):
            part = np.full(size + 16, 0xAB, dtype=np.uint8)
            assert get(g, C.c_void_p(part.ctypes.data), C.c_size_t(out_size)) == size
            assert (part[:out_size] == full[:out_size]).all() and (part[out_size:] == 0xAB).all(), out_size
        assert (full[:8] != 0xAB).any()      # (the getter did write)
    finally:
        lib.ac_free(g)
