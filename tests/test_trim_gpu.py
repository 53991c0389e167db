"""ac_overlap_alignment / ac_trim_paths on the device: the reference's known answers, a slice of the random sweep, one alignment at the
reference's default size against the numpy checker, and a 24-sequence batch (two phases, with and without forced batching) against the
per-sequence results.  Every comparison is equality."""
import random

import pytest

import trim_util as T
from autocycler_amd import AutocyclerError, overlap_alignment, trim_path_slices
from autocycler_amd import _capi
from test_trim_emu import KATS, as_lists, check_kat_slices, check_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_kats():
    for c in KATS["overlap_alignment"]:
        got = overlap_alignment(c["a"], c["b"], c["weights"], c["min_identity"], c["max_unitigs"], c["skip_diagonal"])
        assert as_lists(got) == c["expected"]
    assert check_kat_slices(None) > 10 + 5 + 12


@pytest.mark.parametrize("seed", [7000, 7001])
def test_sweep_slice(seed):
    assert check_sweep(None, seed, 60) > 0


@pytest.mark.parametrize("n", [64, 65, 256, 257, 1025, 1500])
def test_strip_and_band_boundaries(n):
    rng = random.Random(n)
    for hairpin in (False, True):
        p, w = T.planted_overlap_path(rng, n, n // 4, n_unitigs=50, noise=0.05, hairpin=hairpin)
        for mu in (5000, n - 1, 64):
            for a, b, skip in ((p, p, True), (T.reverse_path(p), p, False)):
                assert overlap_alignment(a, b, w, 0.5, mu, skip) == T.overlap_alignment_numpy(a, b, w, 0.5, mu, skip), (n, hairpin, mu, skip)


@pytest.mark.parametrize("hairpin,overlap", [(False, 3000), (True, 1500), (True, 3000)])
def test_default_size_job(hairpin, overlap):
    # the reference's default cap: a path of 12 000 entries with a noisy 3 000-entry overlap, max_unitigs = 5000 -> one 5000 x 5000 matrix.
    # Its hairpin twin aligns the palindrome the mirrored entries form with their originals, twice as many pieces as entries mirrored: 1 500
    # mirrored entries give the 3 000-piece alignment; 3 000 mirrored entries are a 6 000-entry palindrome, which the cap of 5000 cuts (the
    # traceback ends on the left edge: no alignment, in the reference too).
    rng = random.Random(99 + hairpin)
    p, w = T.planted_overlap_path(rng, 12000, overlap, hairpin=hairpin)
    a, b, skip = (T.reverse_path(p), p, False) if hairpin else (p, p, True)
    got = overlap_alignment(a, b, w, 0.75, 5000, skip)
    assert got == T.overlap_alignment_numpy(a, b, w, 0.75, 5000, skip)
    fits = not (hairpin and overlap == 3000)
    assert len(got) >= 2900 if fits else got == []
    res, sm = trim_path_slices([p], w, 0.75, 5000)
    exp, esm = T.trim_paths_expected([p], w, 0.75, 5000, align=T.overlap_alignment_numpy)
    assert res == exp and {q: sm[q] for q in esm} == esm
    assert res[0]["hairpin" if hairpin else "start_end"]["status"] == (1 if fits else 0)
    k3 = min(5000, len(p) - res[0]["hairpin"]["begin"]) if res[0]["hairpin_start_trimmed"] else 5000      # the hairpin-end job runs on the start-trimmed path
    assert sm["cells"] == 2 * 5000 ** 2 + k3 ** 2 and sm["launches"] == 2


def batch_paths():
    rng = random.Random(2024)
    w = None
    paths = []
    for s in range(24):
        n = rng.choice((6000, 9000, 12000))
        overlap = rng.choice((500, 1500, 3000)) // (2 if s % 3 == 1 else 1)      # (a hairpin aligns twice the entries it mirrors)
        p, w1 = T.planted_overlap_path(random.Random(500 + s), n, overlap, hairpin=(s % 3 == 1), noise=0.02)
        if s % 3 == 2:
            p = p[: n // 2]      # no overlap left
        w = w or w1
        paths.append(p)
    return paths, w


def test_batch_of_24(monkeypatch):
    paths, w = batch_paths()
    whole, sm = trim_path_slices(paths, w, 0.75, 5000)
    assert sm["launches"] == 2 and sm["c_se"] >= 8 and sm["c_hp"] >= 8      # (8 planted overlaps of each kind)
    singles = [trim_path_slices([p], w, 0.75, 5000)[0][0] for p in paths]
    assert whole == singles
    # the bytes a launch may take for bit matrices cut to two jobs' worth: the phases run in batches
    k = 5000
    monkeypatch.setenv("AC_TRIM_BATCH_BYTES", str(2 * (k + 63) * ((k + 63) // 64) * 8))
    cut, sm2 = trim_path_slices(paths, w, 0.75, 5000)
    assert sm2["launches"] >= 16      # (16 of the sequences are longer than 5000 entries: 32 full-size jobs in phase 1, two per launch)
    assert cut == whole and sm2["cells"] == sm["cells"]
    # one of them against the numpy checker, so that "equal to each other" is also "right"
    assert whole[0] == T.trim_paths_expected([paths[0]], w, 0.75, 5000, align=T.overlap_alignment_numpy)[0][0]


def test_above_max_unitigs_fails_cleanly():
    n = _capi.max_trim_unitigs() + 1
    assert n > 20000
    p = [1 + (i % 3) for i in range(n)]
    with pytest.raises(AutocyclerError, match="ac_trim_max_unitigs"):
        overlap_alignment(p, p, [1, 1, 1], 0.5, n, True)
    with pytest.raises(AutocyclerError, match="ac_trim_max_unitigs"):
        trim_path_slices([p], [1, 1, 1], 0.5, n)


def test_largest_stated_k_runs():
    # k = 20 000 (the size the feature promises at least): a 50 MB bit matrix, 79 bands
    rng = random.Random(3)
    p, w = T.planted_overlap_path(rng, 20000, 4000, noise=0.01)
    got = overlap_alignment(p, p, w, 0.75, 20000, True)
    assert got == T.overlap_alignment_numpy(p, p, w, 0.75, 20000, True) and len(got) >= 3900
