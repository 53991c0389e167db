"""compress -> cluster -> trim -> resolve as one chain on the device, against planted genomes: the checks of test_chain_emu.py on the device's own
records, every record equal field for field to the one the CPU emulation gives in the same test, and the large case (more than 4 097 unitigs in
one cluster, a path of more than 3 000 entries: several scan and sort tiles in every step, a trim matrix of a dozen bands) on the device only."""
import pytest

import emu_lib
from test_chain_emu import CASES, check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()      # (host code: it needs nothing but the compiler)


@pytest.mark.parametrize("name,seed", CASES)
def test_chain_reaches_the_planted_truth(emu, name, seed):
    _, dev = check_case(name, seed, None)
    _, ref = check_case(name, seed, emu)
    assert sorted(dev) == sorted(ref)
    for key in dev:
        if key == "clusters":
            assert sorted(dev[key]) == sorted(ref[key])
            for c in dev[key]:
                for field in dev[key][c]:
                    assert dev[key][c][field] == ref[key][c][field], f"cluster {c} {field}: the device and the emulation differ"
        elif key != "lib_path":
            assert dev[key] == ref[key], f"{key}: the device and the emulation differ"


def test_large_case():
    check_case("large", 1, None)
