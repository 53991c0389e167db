"""ac_path_distances / ac_resolve_bridge_paths / ac_resolve_bridges on the device: the reference's known answers, a slice of the random sweep,
the full table of strip boundaries, one larger job against the model's numpy form and one graph handle.  Every comparison is equality."""
import random

import pytest

import resolve_util as R
from autocycler_amd import path_distances
from test_resolve_emu import check_above_max_path, check_boundary_table, check_graph, check_kats, check_special_pairs, check_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_kats():
    assert check_kats(None)


@pytest.mark.parametrize("seed", [9000, 9001])
def test_sweep_slice(seed):
    jobs, bridges, _ = check_sweep(None, seed, 75)
    assert jobs > 50 and bridges > 150


def test_boundary_table():
    assert check_boundary_table(None)
    assert check_special_pairs(None)


def test_larger_job():
    # two 3000-entry paths, 5 % edits: 47 strips of 64 columns, the scratch row crossed 46 times
    rng = random.Random(41)
    w = [rng.randint(1, 5000) for _ in range(200)]
    a = R.random_path(rng, 3000, 200)
    b = R.edited_copy(rng, a, 0.05, 200)
    b = (b + R.random_path(rng, 3000, 200))[:3000]
    exp = R.global_alignment_distance_numpy(a, b, w)
    d, st = path_distances([a, b], [(0, 1), (1, 0)], w)
    assert st == [0, 0] and d == [exp, exp] and 0 < exp < sum(w[abs(u) - 1] for u in a)


def test_above_max_path_fails_cleanly():
    assert check_above_max_path(None)


def test_graph_handle():
    assert check_graph(None, 3, 11)
