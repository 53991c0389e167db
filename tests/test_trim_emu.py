"""ac_overlap_alignment / ac_trim_paths on the CPU emulation of the shipped kernels (kernels_trim.inc under the lockstep emulation of
wave_rt.hpp) against the reference's own known answers (golden/trim_kats.json) and the specification-level checker (trim_util.py).
Every comparison is equality: the arithmetic is integer.  The same cases run on the device in test_trim_gpu.py."""
import random

import pytest

import emu_lib
import parity_util
import seqgen
import trim_util as T
from autocycler_amd import AutocyclerError, graph_from_gfa, overlap_alignment, trim_path_slices
from autocycler_amd import _capi


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


KATS = T.load_kats()


def as_lists(pieces):
    return [list(p) for p in pieces]


# ---- the checker itself: (a) reproduces the reference's known answers, (b) equals (a) ------------------------------------------------
def test_checker_plain_reproduces_kats():
    for c in KATS["overlap_alignment"]:
        assert as_lists(T.overlap_alignment_plain(c["a"], c["b"], c["weights"], c["min_identity"], c["max_unitigs"], c["skip_diagonal"])) == c["expected"]
    for group, fn in (("start_end", T.start_end_slice), ("hairpin_end", T.hairpin_end_slice), ("hairpin_start", T.hairpin_start_slice)):
        for c in KATS[group]:
            st, b, e = fn(c["path"], c["weights"], c["min_identity"], c["max_unitigs"])
            assert (c["path"][b:e] if st == 1 else None) == c["expected"] and st != 2, (group, c["test"])
    for c in KATS["hairpin_start_then_end"]:
        res, _ = T.trim_paths_expected([c["path"]], c["weights"], c["min_identity"], c["max_unitigs"])
        r = res[0]["hairpin"]
        assert r["status"] == 1 and c["path"][r["begin"]:r["end"]] == c["expected"]
        assert res[0]["hairpin_start_trimmed"] == 1 and res[0]["hairpin_end_trimmed"] == 1


def test_checker_numpy_equals_plain():
    rng = random.Random(20240)
    for _ in range(300):
        p, w, mi, mu = T.random_case(rng)
        for a, b, skip in ((p, p, True), (T.reverse_path(p), p, False), (p, T.reverse_path(p), False)):
            assert T.overlap_alignment_numpy(a, b, w, mi, mu, skip) == T.overlap_alignment_plain(a, b, w, mi, mu, skip)
    for c in KATS["overlap_alignment"]:
        assert as_lists(T.overlap_alignment_numpy(c["a"], c["b"], c["weights"], c["min_identity"], c["max_unitigs"], c["skip_diagonal"])) == c["expected"]


# ---- known answers through the library ---------------------------------------------------------------------------------------------
def test_kat_overlap_alignment(emu):
    assert len(KATS["overlap_alignment"]) == 8
    for c in KATS["overlap_alignment"]:
        got = overlap_alignment(c["a"], c["b"], c["weights"], c["min_identity"], c["max_unitigs"], c["skip_diagonal"], lib_path=emu)
        assert as_lists(got) == c["expected"]


def check_kat_slices(lib_path, device=0):
    """Every trimming KAT through ac_trim_path_slices.  The library reports the two kinds a sequence is trimmed by: start-end as the
    reference's trim_path_start_end, hairpin as start-then-end.  A hairpin-end (-start) KAT is the library's hairpin result whenever the
    other side did not fire on that path, which the result says; in every case the result must be the checker's."""
    direct = 0
    for c in KATS["start_end"]:
        res, sm = trim_path_slices([c["path"]], c["weights"], c["min_identity"], c["max_unitigs"], device=device, lib_path=lib_path)
        r = res[0]["start_end"]
        assert (c["path"][r["begin"]:r["end"]] if r["status"] == 1 else None) == c["expected"] and r["status"] != 2, c["test"]
        assert r["trimmed_length"] == T.slice_length(c["path"], c["weights"], r["begin"], r["end"])
        exp, esm = T.trim_paths_expected([c["path"]], c["weights"], c["min_identity"], c["max_unitigs"])
        assert res == exp and {k: sm[k] for k in esm} == esm
        direct += 1
    for group, other in (("hairpin_end", "hairpin_start_trimmed"), ("hairpin_start", "hairpin_end_trimmed")):
        for c in KATS[group]:
            res, sm = trim_path_slices([c["path"]], c["weights"], c["min_identity"], c["max_unitigs"], device=device, lib_path=lib_path)
            exp, esm = T.trim_paths_expected([c["path"]], c["weights"], c["min_identity"], c["max_unitigs"])
            assert res == exp and {k: sm[k] for k in esm} == esm, (group, c["test"])
            if not res[0][other]:
                r = res[0]["hairpin"]
                assert (c["path"][r["begin"]:r["end"]] if r["status"] == 1 else None) == c["expected"] and r["status"] != 2, (group, c["test"])
                direct += 1
    for c in KATS["hairpin_start_then_end"]:
        res, _ = trim_path_slices([c["path"]], c["weights"], c["min_identity"], c["max_unitigs"], device=device, lib_path=lib_path)
        r = res[0]["hairpin"]
        assert r["status"] == 1 and c["path"][r["begin"]:r["end"]] == c["expected"]
        assert res[0]["hairpin_start_trimmed"] == 1 and res[0]["hairpin_end_trimmed"] == 1
        direct += 1
    return direct


def test_kat_trim_slices(emu):
    direct = check_kat_slices(emu)
    assert direct > 10 + 5 + 12      # all start-end and start-then-end KATs, and at least half of the 25 hairpin KATs compared directly


# ---- random sweep ------------------------------------------------------------------------------------------------------------------
def check_sweep(lib_path, seed, cases, device=0, n_lo=2, n_hi=120):
    rng = random.Random(seed)
    trimmed = 0
    batch = []
    for _ in range(cases):
        p, w, mi, mu = T.random_case(rng, n_lo, n_hi)
        for a, b, skip in ((p, p, True), (T.reverse_path(p), p, False)):
            assert overlap_alignment(a, b, w, mi, mu, skip, device=device, lib_path=lib_path) == T.overlap_alignment_plain(a, b, w, mi, mu, skip), (p, w, mi, mu, skip)
        res, sm = trim_path_slices([p], w, mi, mu, device=device, lib_path=lib_path)
        exp, esm = T.trim_paths_expected([p], w, mi, mu)
        assert res == exp and {k: sm[k] for k in esm} == esm, (p, w, mi, mu)
        trimmed += esm["c_se"] + esm["c_hp"]
        batch.append((p, w, mi, mu, exp[0]))
    # the same paths as ONE call per (weights, min_identity, max_unitigs) class would need equal weights: instead one batch of the cases of
    # the first case's parameters re-drawn over its weights
    p0, w0, mi0, mu0, _ = batch[0]
    U = len(w0) - 1
    many = [[rng.choice((-1, 1)) * rng.randint(1, U) for _ in range(rng.randint(1, 40))] for _ in range(8)] + [p0, p0 + T.reverse_path(p0)]
    res, sm = trim_path_slices(many, w0, mi0, mu0, device=device, lib_path=lib_path)
    exp, esm = T.trim_paths_expected(many, w0, mi0, mu0)
    assert res == exp and {k: sm[k] for k in esm} == esm
    return trimmed


@pytest.mark.parametrize("seed", range(4))
def test_random_sweep(emu, seed):
    assert check_sweep(emu, 7000 + seed, 60) > 0      # (planted overlaps: some of them must trim, or the sweep tests nothing)


@pytest.mark.parametrize("order", [1, 2])
def test_scheduling_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))
    check_sweep(emu, 7100 + order, 25)
    test_kat_overlap_alignment(emu)


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 515, 770])
def test_lane_and_strip_boundaries(emu, n):
    # one column per lane, 64 lanes per strip, four strips per band (515 / 770: a third / fourth band, which reuse the two edge buffers): path lengths around each boundary, once with the whole path in the
    # matrix and once capped right below / at a boundary
    rng = random.Random(n)
    w = [rng.choice(T.SWEEP_WEIGHTS) for _ in range(9)]
    m = n // 3
    core = [rng.choice((-1, 1)) * rng.randint(1, 8) for _ in range(n - m)]
    rep = list(core[:m]); rep[m // 2] = 9
    hp = T.reverse_path(core[-m:]); hp.insert(m // 3, 9); hp = hp[:m]
    for p in (core + rep, core + hp):
        for mu in (1000, 64, n - 1):
            for a, b, skip in ((p, p, True), (T.reverse_path(p), p, False)):
                assert overlap_alignment(a, b, w, 0.5, mu, skip, lib_path=emu) == T.overlap_alignment_numpy(a, b, w, 0.5, mu, skip), (n, mu, skip)
    p = core + rep
    res, _ = trim_path_slices([p, core + hp], w, 0.5, 1000, lib_path=emu)
    assert res == T.trim_paths_expected([p, core + hp], w, 0.5, 1000, align=T.overlap_alignment_numpy)[0]
    assert res[0]["start_end"]["status"] == 1 and res[1]["hairpin"]["status"] == 1


def test_batches_equal_one_launch(emu, monkeypatch):
    rng = random.Random(5)
    w = [rng.choice(T.SWEEP_WEIGHTS) for _ in range(7)]
    paths = []
    for _ in range(6):
        core = [rng.choice((-1, 1)) * rng.randint(1, 6) for _ in range(rng.randint(20, 70))]
        paths.append(core + core[:rng.randint(3, 15)] if rng.random() < 0.5 else core + T.reverse_path(core[-rng.randint(3, 15):]))
    whole, sm = trim_path_slices(paths, w, 0.5, 1000, lib_path=emu)
    assert sm["launches"] == 2
    monkeypatch.setenv("AC_TRIM_BATCH_BYTES", str(2 * (70 + 15 + 63) * 2 * 8))      # two jobs' worth of bit matrices
    cut, sm2 = trim_path_slices(paths, w, 0.5, 1000, lib_path=emu)
    assert sm2["launches"] > 2 and cut == whole and sm2["cells"] == sm["cells"]
    assert whole == T.trim_paths_expected(paths, w, 0.5, 1000)[0]


def test_max_unitigs_zero_disables(emu):
    p = [1, 2, 3, 4, 5, -5, -4, 1, 2]
    res, sm = trim_path_slices([p], [10] * 5, 0.5, 0, lib_path=emu)
    full = dict(status=0, begin=0, end=len(p), trimmed_length=90)
    assert res == [dict(start_end=full, hairpin=full, hairpin_start_trimmed=0, hairpin_end_trimmed=0)]
    assert (sm["c_se"], sm["c_hp"], sm["chosen"], sm["cells"]) == (0, 0, 0, 0)
    assert overlap_alignment(p, p, [10] * 5, 0.5, 0, True, lib_path=emu) == []


def test_validation_errors(emu):
    ok = [1, -2, 3]
    for mi in (-0.01, 1.01, float("nan")):
        with pytest.raises(AutocyclerError, match="min_identity"):
            overlap_alignment(ok, ok, [5, 5, 5], mi, 10, True, lib_path=emu)
        with pytest.raises(AutocyclerError, match="min_identity"):
            trim_path_slices([ok], [5, 5, 5], mi, 10, lib_path=emu)
    with pytest.raises(AutocyclerError, match="names no unitig"):
        overlap_alignment([1, 0, 3], ok, [5, 5, 5], 0.5, 10, True, lib_path=emu)
    with pytest.raises(AutocyclerError, match="names no unitig"):
        overlap_alignment(ok, [1, -4, 3], [5, 5, 5], 0.5, 10, True, lib_path=emu)
    with pytest.raises(AutocyclerError, match="names no unitig"):
        trim_path_slices([ok, [4]], [5, 5, 5], 0.5, 10, lib_path=emu)
    big = [0xFFFFFFFE, 1, 1]
    with pytest.raises(AutocyclerError, match="2\\^32"):
        overlap_alignment([1, 2, 3], [1, 2, 3], big, 0.5, 10, True, lib_path=emu)
    with pytest.raises(AutocyclerError, match="2\\^32"):
        trim_path_slices([[1, 2, 3]], big, 0.5, 10, lib_path=emu)
    assert overlap_alignment([1, 3], [1, 3], big, 0.5, 10, True, lib_path=emu) == []      # (2^32 - 1: still below)
    assert _capi.max_trim_unitigs(emu) >= 20000


def test_above_max_unitigs_fails_cleanly(emu):
    n = _capi.max_trim_unitigs(emu) + 1
    p = [1 + (i % 3) for i in range(n)]
    with pytest.raises(AutocyclerError, match="ac_trim_max_unitigs"):
        overlap_alignment(p, p, [1, 1, 1], 0.5, n, True, lib_path=emu)
    with pytest.raises(AutocyclerError, match="ac_trim_max_unitigs"):
        trim_path_slices([p], [1, 1, 1], 0.5, n, lib_path=emu)
    assert trim_path_slices([p], [1, 1, 1], 0.5, 8, lib_path=emu)[0] == T.trim_paths_expected([p], [1, 1, 1], 0.5, 8)[0]      # capped: fine


# ---- on a graph handle ---------------------------------------------------------------------------------------------------------------
def graph_paths(g):
    w = [len(g.unitig(i)[0]) for i in range(g.unitig_count)]
    return [list(g.path(s)) for s in range(g.n_seqs)], w


@pytest.mark.parametrize("seed,k", [(1, 11), (13, 21)])
def test_graph_with_real_overlaps(emu, seed, k):
    # contigs that run past their own start (s + s[:m]: what a circular replicon assembled with overlap looks like), one of them
    # with a hairpin end instead; built by the emulation, trimmed, and the slices compared with the checker on the handle's own paths
    r = random.Random(seed)
    base, fn, hd = seqgen.make_case(seed, k)
    seqs = []
    for i, s in enumerate(base):
        if len(s) < 4 * k:
            s = s + seqgen.rand_seq(r, 4 * k)
        m = max(2 * k, len(s) // 4)
        seqs.append(s + seqgen.rc(s[-m:]) if i == 1 else s + s[:m])
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=emu, repair=False)
    paths, w = graph_paths(g)
    for mi, mu in ((0.75, 5000), (0.95, 6)):
        res, sm = g.trim_paths(mi, mu)
        exp, esm = T.trim_paths_expected(paths, w, mi, mu)
        assert res == exp and {q: sm[q] for q in esm} == esm
    res, sm = g.trim_paths()      # the reference's defaults
    assert sm["c_se"] >= 1 and sm["chosen"] == 1 and sm["cells"] > 0
    g2, _, _ = graph_from_gfa(gfa, lib_path=emu)      # what `autocycler trim` itself starts from
    assert g2.trim_paths() [0] == res
