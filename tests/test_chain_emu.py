"""compress -> cluster -> trim -> resolve as one chain on the CPU emulation of the shipped kernels, against planted genomes (chain_util.py): the
expected values are the planted replicons, not a reading of the reference.  Every stage is checked on the way (a failure names the first stage
that broke), both entry forms (the built handle and the GFA text read again) must print the same texts, and every case asserts what it is there
to cover.  The same checks run on the device in test_chain_gpu.py, with the large case on top."""
import pytest

import chain_util as CU
import emu_lib

CASES = [("small", 1), ("small", 2), ("clean", 1), ("wide51", 1), ("wide101", 1), ("repeat_contaminant", 1), ("medium", 1), ("medium", 2), ("hairpin21", 1),
         ("hairpin21", 2), ("hairpin51", 1), ("hairpin51", 2), ("outlier", 1), ("majority", 1)]
# what becomes of the junk-tailed contig at cluster: with 5 assemblies it stays in its replicon's cluster and trim excludes it by length
JUNK_FAILS_ALONE = {"outlier": False}


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def chromosome(case, rec, of):
    return rec["clusters"][of[0]]


def cover_small(case, rec, of):
    assert len(of) == 2 and rec["fail"] == [0, 0]
    assert all(rec["clusters"][c]["chosen"] == "start_end" and len(rec["clusters"][c]["trimmed_start_end"]) >= 1 for c in of.values())
    assert sum(not c["free"] for c in case["contigs"]) >= 5      # (every assembly differs from the truth somewhere)


def cover_clean(case, rec, of):
    assert all(c["free"] and not c["overrun"] for c in case["contigs"])
    for c in of.values():
        cl = rec["clusters"][c]
        assert cl["chosen"] == "" and not cl["trimmed_start_end"] and not cl["trimmed_hairpin"] and cl["unitigs_before"] == cl["unitigs_after"]
        assert len(cl["final_segments"]) == 1 and sorted(cl["final_links"]) == [(-1, -1), (1, 1)]


def cover_wide(words):
    def cover(case, rec, of):
        assert (2 * case["k"] + 63) // 64 == words      # (two bits a base: the k-mer keys of compress take this many 64-bit words)
        assert chromosome(case, rec, of)["unitigs_before"] > 100 and len(of) == 2
    return cover


def cover_repeat_contaminant(case, rec, of):
    assert sorted(rec["fail"]) == [0, 0, CU.FAIL_TOO_FEW_ASSEMBLIES] and rec["labels"].count(0) == 1
    assert rec["empty_clusters"] and rec["empty_clusters"][0] < max(rec["labels"])      # (a cluster number in the middle is skipped)
    assert any(t for t in case["truth"] if t["seq"].count(t["seq"][len(t["seq"]) // 4:len(t["seq"]) // 4 + 200]) == 2)      # (the repeat is there)


def cover_medium(case, rec, of):
    cl = chromosome(case, rec, of)
    assert cl["unitigs_before"] > 700 and cl["longest_path"] > 512, (cl["unitigs_before"], cl["longest_path"])


def cover_hairpin(case, rec, of):
    cl = rec["clusters"][of[1]]
    u = cl["final_segments"][0][0]
    assert cl["chosen"] == "hairpin" and len(cl["trimmed_hairpin"]) == 4 and len(cl["hairpin_both"]) == 1
    assert sorted(cl["final_links"]) == sorted([(u, -u), (-u, u)])
    assert chromosome(case, rec, of)["chosen"] == "start_end"
    assert any(c["free"] and c["overrun"] == "start_end" for c in case["contigs"]) and any(c["free"] and c["overrun"].startswith("hairpin") for c in case["contigs"])


def cover_outlier(case, rec, of):
    assert sum(len(cl["excluded"]) for cl in rec["clusters"].values()) == 1 and len(chromosome(case, rec, of)["excluded"]) == 1


def cover_majority(case, rec, of):
    t = case["truth"][0]
    assert t["seq"] != t["root"] and sum(x != y for x, y in zip(t["seq"], t["root"])) == 1
    assert chromosome(case, rec, of)["final_segments"][0][1].encode() != t["root"]


def cover_large(case, rec, of):
    cl = chromosome(case, rec, of)
    assert cl["unitigs_before"] > 4097 and cl["longest_path"] > 3000, (cl["unitigs_before"], cl["longest_path"])


COVERAGE = dict(small=cover_small, clean=cover_clean, wide51=cover_wide(2), wide101=cover_wide(4), repeat_contaminant=cover_repeat_contaminant, medium=cover_medium,
                hairpin21=cover_hairpin, hairpin51=cover_hairpin, outlier=cover_outlier, majority=cover_majority, large=cover_large)


def check_case(name, seed, lib_path, device=0):
    """one case through the chain with every stage's check, then what the case is there to cover; returns (case, record)"""
    case = CU.make_case(name, seed)
    rec = CU.run_chain(case, lib_path, device)
    of = CU.check_record(case, rec, JUNK_FAILS_ALONE.get(name))
    COVERAGE[name](case, rec, of)
    print(CU.facts(case, rec))
    return case, rec


@pytest.mark.parametrize("name,seed", CASES)
def test_chain_reaches_the_planted_truth(emu, name, seed):
    check_case(name, seed, emu)


# ---- the generator and the glue's own arithmetic ----------------------------------------------------------------------------------------------
def test_generator_keeps_its_preconditions():
    for name, seed in CASES:
        case = CU.make_case(name, seed)
        assert case["filenames"] == sorted(case["filenames"]) and len(case["seqs"]) == len(case["contigs"])
        assert CU.make_case(name, seed)["seqs"] == case["seqs"]      # (a fixed seed gives the same assemblies)
    with pytest.raises(AssertionError, match="no room"):      # 60 sites 202 apart do not fit 8 000 bases
        CU.planted_case(101, [CU.CIRC(8000)], 6, 10, 1)
    with pytest.raises(AssertionError, match="no room left"):      # 3 assemblies: one diverted contig could tie a bridge, so no site is planted
        CU.planted_case(21, [CU.CIRC(3000)], 3, 1, 1)
    with pytest.raises(AssertionError, match="a k-mer would cover two sites"):
        CU.planted_case(21, [CU.CIRC(3000)], 5, 1, 1, site_gap=21)
    with pytest.raises(AssertionError, match="occurs twice outside the planted repeat"):
        CU._check_unique_kmers(5, [dict(root=b"ACGTTACGTTGG", circular=False, repeat=None)])


def test_glue_arithmetic():
    """median_isize / mad_isize (misc.rs:433-457) and the allowed range (trim.rs:236-240) on values worked by hand"""
    assert CU.median_isize([]) == 0 and CU.median_isize([5]) == 5 and CU.median_isize([4, 1, 3]) == 3 and CU.median_isize([4, 1, 3, 8]) == 3      # (3 + 4) / 2
    assert CU.mad_isize([10, 12, 14, 30]) == 2      # median 13; deviations 3, 1, 1, 17 -> (1 + 3) / 2
    assert CU.allowed_length_range([3000, 3000, 3000, 3450, 3000]) == (3000, 3000)
    assert CU.allowed_length_range([10, 12, 14, 30]) == (3, 23)
    assert CU.allowed_length_range([1, 100, 1000]) == (0, 595)      # (median 100, MAD 99: the lower end saturates at 0)
    res = lambda se, hp: [dict(start_end=dict(status=int(i < se)), hairpin=dict(status=int(i < hp))) for i in range(4)]
    assert CU.choose_trim_type(res(0, 0)) is None and CU.choose_trim_type(res(2, 2)) == "start_end" and CU.choose_trim_type(res(1, 2)) == "hairpin"
    assert CU.same_circular(b"AACGT", b"GTAAC") and CU.same_circular(b"AACGT", CU.rc(b"GTAAC")) and not CU.same_circular(b"AACGT", b"AACGA")
    assert CU.same_linear(b"AACG", b"CGTT") and not CU.same_linear(b"AACG", b"ACGA")
