"""The kernel bounds check (tests/c_client/kernel_bounds_check.cpp): call files for the replay driver and the model checks of what it hands back.

The driver is the whole CPU emulation under the address and undefined-behaviour sanitizers with the guarded arena of csrc/device_rt.hpp: it
cannot import the generators or the models, so a group of calls is written to a file here (one record per call: entry, scalars, arrays, the
environment knobs of that call), replayed there, and every call's outputs are compared here with what the oracle or the plain-Python model of
that entry gives — the guarded run is a second parity run as well as a bounds check.  Shapes are the smallest at which each kernel's indexing
can go wrong: both sides of every key-width and tile boundary, one and several blocks, empty and one-element inputs."""
import ctypes as C
import fcntl
import random
import struct
import subprocess
from pathlib import Path

import numpy as np

import components_util
import depth_util
import merge_util
import oracle_lib as O
import resolve_util
import seqgen
import trim_util
import cluster_util
import verify_model
from autocycler_amd import _capi
from verify_cases import _Gfa, same_report

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "autocycler_amd" / "csrc"
GUARD_DIR = ROOT / "tests" / "_emu" / "guard"


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = GUARD_DIR / f"kernel_bounds_check_l{level}"
    srcs = list(CSRC.glob("*.[ch]*")) + list(CSRC.glob("*.inc")) + [ROOT / "include" / "autocycler_hip.h", CSRC / "Makefile"] + \
        [ROOT / "tests" / "c_client" / n for n in ("kernel_bounds_check.cpp", "kernel_bounds_guard.cpp")]
    GUARD_DIR.mkdir(parents=True, exist_ok=True)
    with open(GUARD_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in srcs):
            subprocess.check_call(["make", "-j", "8", "-C", str(CSRC), str(Path("../../tests/_emu/guard") / exe.name)], stdout=subprocess.DEVNULL)
    return exe


SANITIZER_WORDS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "UndefinedBehaviorSanitizer")


def run_clean(cmd, timeout=900):
    """exit status 0 and no sanitizer report"""
    out = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout)
    assert not any(w in out.stderr for w in SANITIZER_WORDS), out.stderr[-6000:]
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    return out


# ---- the call file ------------------------------------------------------------------------------------------------------------------------
def _str(s):
    b = s.encode() if isinstance(s, str) else bytes(s)
    return struct.pack("<I", len(b)) + b


def f64_bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def arr(values, dtype):
    return b"" if values is None else np.ascontiguousarray(np.asarray(values, dtype=dtype)).tobytes()


class Calls:
    """One call file: add(entry, scalars, arrays, check, env) queues a call and the function that judges its outputs (a list of bytes)."""

    def __init__(self):
        self.records, self.checks = [], []

    def add(self, entry, scalars, arrays, check, env=None, label=""):
        env = env or {}
        rec = [_str(entry), struct.pack("<I", len(env))] + [_str(a) + _str(b) for a, b in env.items()]
        rec += [struct.pack("<I", len(scalars))] + [struct.pack("<q", int(v)) for v in scalars]
        rec += [struct.pack("<I", len(arrays))]
        for a in arrays:
            a = bytes(a)
            rec += [struct.pack("<Q", len(a)), a]
        self.records.append(b"".join(rec))
        self.checks.append((check, f"call {len(self.checks)} {entry} {label} {env or ''}"))

    def run(self, exe, tmp_path):
        calls, results = tmp_path / "calls.bin", tmp_path / "results.bin"
        calls.write_bytes(b"ACBC1\n" + b"".join(self.records))
        out = run_clean([exe, calls, results])
        assert f"{len(self.checks)} calls OK" in out.stdout, out.stdout[-2000:]
        raw, at = results.read_bytes(), 0
        for check, label in self.checks:
            rc, n = struct.unpack_from("<II", raw, at); at += 8
            outs = []
            for _ in range(n):
                (nb,) = struct.unpack_from("<Q", raw, at); at += 8
                outs.append(raw[at:at + nb]); at += nb
            assert rc == 0, label
            check(outs, label)
        assert at == len(raw)
        return len(self.checks)


# ---- the graph build -----------------------------------------------------------------------------------------------------------------------
EX_DIST, EX_DECOMP_DEVICE, EX_DECOMP_SEQ, EX_VERIFY = 1, 2, 4, 8
_ORACLE = {}


def _oracle(k, seqs, fn, hd, repair):
    key = (k, tuple(seqs), tuple(fn), tuple(hd), repair)
    if key not in _ORACLE:
        s = O.Seqs.from_raw(k, seqs, filenames=fn, headers=hd, repair=repair)
        gfa, st, _ = s.compress(k)
        _ORACLE[key] = (s.all(), s.assembly_count, gfa, st, O.pairwise_distances(gfa))
    return _ORACLE[key]


def _check_extras(outs, label, k, loaded, gfa, dist, extras, report_model=None):
    """outs: distances | decompress_device | decompress_seq | verify report.  The path-spelling model: a sequence is its own middle."""
    plain = [bytes(q["fwd"])[k // 2:k // 2 + q["length"]] for q in loaded]
    if extras & EX_DIST:
        got = np.frombuffer(outs[0], dtype="<f8")
        assert got.tobytes() == np.asarray(dist, dtype="<f8").tobytes(), (label, "distances")
    if extras & EX_DECOMP_DEVICE:
        assert outs[1] == b"".join(plain), (label, "decompress_device")
    if extras & EX_DECOMP_SEQ:
        assert outs[2] == b"".join(plain), (label, "decompress_seq")
    if extras & EX_VERIFY:
        names = ("failed", "first_bad_unitig", "first_bad_link", "first_bad_path_entry", "first_bad_sequence", "first_bad_base", "unitigs", "links", "path_entries",
                 "bases_checked", "self_mirror_links", "checks", "first_bad_junction")
        rep = dict(zip(names, (int(v) for v in np.frombuffer(outs[3], dtype="<u8"))))
        if report_model is not None:
            mod, detail = report_model
            lib, want = same_report(rep, mod, detail)
            assert lib == want, (label, {f: (lib[f], want[f]) for f in verify_model.FIELDS if lib[f] != want[f]})
        else:      # a built graph holds; the counts are the GFA's
            lines = gfa.split("\n")
            assert rep["failed"] == 0 and rep["checks"] == 15, (label, rep)
            assert rep["unitigs"] == sum(l[:1] == "S" for l in lines) and rep["links"] == sum(l[:1] == "L" for l in lines), (label, rep)
            assert rep["path_entries"] == sum(l.split("\t")[2].count(",") + 1 for l in lines if l[:1] == "P") and rep["bases_checked"] == sum(len(p) for p in plain), (label, rep)


def add_build(calls, k, seqs, fn, hd, repair=True, mode=0, ranks=0, extras=0, env=None):
    """mode 0: ac_compress_build, 1: ac_compress_build_multi over `ranks` emulated ranks, 2: the unrepaired text laid out, ac_end_repair_device (when
    repair) and ac_compress_build_device on it.  Everything is held to the oracle's GFA and statistics for the (repaired) sequences."""
    loaded, n_asm, gfa, st, dist = _oracle(k, seqs, fn, hd, repair)
    sent = _oracle(k, seqs, fn, hd, False)[0] if mode == 2 else loaded
    label = f"k={k} n={len(seqs)} repair={repair} mode={mode}"

    def check(outs, label):
        assert outs[0].decode() == gfa, (label, parity_first_diff(gfa, outs[0].decode()))
        got = [int(v) for v in np.frombuffer(outs[1], dtype="<u8")]
        want = [st[n] for n in ("kmers", "unitigs_pre", "links_pre", "length_pre", "unitigs_post", "links_post", "length_post")]
        assert got == want, (label, got, want)
        if mode == 2:
            off, d12 = 1, np.frombuffer(outs[3], dtype="<u2")
            for i, q in enumerate(loaded):
                plen = q["length"] + k - 1
                g = outs[2][off:off + plen]
                assert g == q["fwd"], (label, "repair of sequence", i)
                assert (int(d12[i]), int(d12[len(loaded) + i])) == (len(g) - len(g.lstrip(b".")), len(g) - len(g.rstrip(b"."))), (label, i)
                off += plen + 1
        _check_extras(outs[5:], label, k, loaded, gfa, dist, extras)

    fwd = b"".join(bytes(q["fwd"]) for q in sent)
    calls.add("build", [k, n_asm, len(sent), mode, ranks, 1 if (repair and mode == 2) else 0, extras],
              [fwd, arr([q["length"] for q in sent], "<u4"), arr([q["id"] for q in sent], "<u2"), "".join(q["filename"] + "\n" for q in sent).encode(),
               "".join(q["header"] + "\n" for q in sent).encode()], check, env, label)


def parity_first_diff(a, b):
    import parity_util
    return parity_util.first_diff(a, b)


BUILD_KS = (3, 11, 27, 29, 51, 59, 61, 91, 93, 123, 125, 251, 253, 501)      # both sides of every key-width boundary, and the wide widths
KNOB_KS = (11, 51, 125)
KNOB_SETTINGS = [{"AC_PATH_COPY": "1"}, {"AC_PATH_COPY": "1", "AC_RUN_PIECE": "150"}, {"AC_POS_CAP": "1"}, {"AC_POS_CAP": "7"},
                 {"AC_INSERT_ADAPT": "0", "AC_INSERT_GROWTH": "4"}, {"AC_HOST_REMAP": "0"}, {"AC_HOST_REMAP": "1"}, {"AC_HOST_REMAP": "2"}, {"AC_LATE_COPIES": "2"},
                 {"AC_SEQ_CODES": "0"}, {"AC_SEQ_CODES": "2"}, {"AC_TABLE_SHIFT": "0"}, {"AC_TABLE_SHIFT": "2"}]


def build_calls(ks, seeds=range(12)):
    """ac_compress_build on every kind of seqgen.make_case, end repair on and off; one case per k also with everything that runs on a built handle"""
    c = Calls()
    for k in ks:
        for seed in seeds:
            seqs, fn, hd = seqgen.make_case(seed, k)
            add_build(c, k, seqs, fn, hd, repair=True, extras=(EX_DIST | EX_DECOMP_DEVICE | EX_DECOMP_SEQ | EX_VERIFY) if seed in (2, 7) else 0)
            add_build(c, k, seqs, fn, hd, repair=False)
    return c


def synth_case(n=6, genome=60_000, plasmid=3_000, seed=99):
    from autocycler_amd import synth
    seqs, fn, hd = [], [], []
    for i, contigs in enumerate(synth.make_assemblies(n, genome=genome, plasmid=plasmid, sub=1e-3, indel=1e-4, seed=seed)):
        for header, s in contigs:
            seqs.append(s.tobytes().decode()); fn.append(f"assembly_{i:04d}.fasta"); hd.append(header)
    return seqs, fn, hd


def knob_calls():
    """the settings that move allocations: the copying walk, the position-cap retry, table regrowth, the host remap modes, late copies, sequence codes"""
    c = Calls()
    for env in KNOB_SETTINGS:
        for k in KNOB_KS:
            for seed in (1, 7, 10):
                seqs, fn, hd = seqgen.make_case(seed, k)
                add_build(c, k, seqs, fn, hd, env=env)
    seqs, fn, hd = synth_case()
    for env in ({}, {"AC_PATH_COPY": "1"}, {"AC_PATH_COPY": "1", "AC_RUN_PIECE": "150"}, {"AC_POS_CAP": "7"}, {"AC_HOST_REMAP": "2"}, {"AC_INSERT_ADAPT": "0", "AC_INSERT_GROWTH": "4"}):
        add_build(c, 51, seqs, fn, hd, env=env)
    return c


def device_entry_calls():
    """ac_end_repair_device + ac_compress_build_device on a resident text (a host pointer in the emulation).  k = 65 / 129 / 257: the repair's literal
    fills whole key words.  Sequence lengths on both sides of the 32-, 64- and 256-position words and tiles."""
    c = Calls()
    rng = random.Random(11)
    for k in (5, 21, 51, 65, 129, 131, 257):
        lens = sorted(n for n in {k, k + 1, 31, 32, 33, 63, 64, 65, 255, 256, 257} if n >= k)      # (a sequence is at least one k-mer)
        base = seqgen.rand_seq(rng, 300 + k)
        seqs = []
        for i, n in enumerate(lens):      # overlapping windows of one sequence and of its reverse complement: shared k-mers, repairable ends
            s = base[(7 * i) % 40:][:n] if n <= len(base) else seqgen.rand_seq(rng, n)
            seqs.append(s if i % 3 else seqgen.rc(s))
        fn = [f"a{i % 4}.fasta" for i in range(len(seqs))]; hd = [f"c{i}" for i in range(len(seqs))]
        add_build(c, k, seqs, fn, hd, repair=True, mode=2, extras=EX_VERIFY | EX_DECOMP_DEVICE)
        add_build(c, k, seqs, fn, hd, repair=False, mode=2)
        for seed in (2, 6, 9):
            s2, f2, h2 = seqgen.make_case(seed, k)
            add_build(c, k, s2, f2, h2, repair=True, mode=2)
    add_long_repair(c)
    return c


def repair_model(k, seqs):
    """sequence_end_repair (compress.rs:202-270) with Python's own regex engine: the first / last k - 1 bytes of a padded sequence are the pattern
    (a dot matches any byte, find_iter = leftmost non-overlapping), the haystacks are every padded sequence and its reverse complement as they were
    before any repair, the best match has the fewest dots, then the most occurrences, then the smallest bytes.  -> (repaired padded sequences, matches)"""
    import re
    from collections import Counter
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    m, h = k - 1, k // 2
    fwd = [b"." * h + s.encode() + b"." * h for s in seqs]
    hays = [x for f in fwd for x in (f, f.translate(comp)[::-1])]
    out, total = [], 0
    for f in fwd:
        ends = []
        for pat in (f[:m], f[len(f) - m:]):
            found = [x for hay in hays for x in re.findall(pat, hay, re.DOTALL)]
            total += len(found)
            freq = Counter(found)
            ends.append(min(freq, key=lambda x: (x.count(b"."), -freq[x], x)))
        out.append(ends[0] + f[m:len(f) - m] + ends[1] if len(f) >= 2 * m else None)
    return out, total


LONG_REPAIR_BASES = 1_300_000


def add_long_repair(calls):
    """One k = 3 text of 1.3 M bases over AC: the literal of every end pattern is one base, so the scan of ac_end_repair_device reports more than 2^20
    hits and repeats with a larger hit buffer (EndScanFunctor must hold its writes to the first buffer's size while the count runs past it).  The
    oracle's whole compress of this text takes minutes (its repair a fraction of a second), so: the repaired text and the surviving dots against the
    oracle's repair AND the regex model above, the number of matches against the model, and the graph ac_compress_build_device makes of the repaired
    text against the verifier with all its checks (the reference's graph, not merely a consistent one) and the path-spelling model."""
    k = 3
    r = random.Random(5)
    long_seq = "".join(r.choice("AC") for _ in range(LONG_REPAIR_BASES))
    seqs, fn, hd = [long_seq, long_seq[1000:3000]], ["x.fasta", "y.fasta"], ["long", "short"]
    sent = O.Seqs.from_raw(k, seqs, filenames=fn, headers=hd, repair=False).all()
    loaded = O.Seqs.from_raw(k, seqs, filenames=fn, headers=hd, repair=True).all()
    model, n_matches = repair_model(k, seqs)
    assert [bytes(q["fwd"]) for q in loaded] == model      # (the two references agree)
    extras = EX_VERIFY | EX_DECOMP_DEVICE | EX_DECOMP_SEQ

    def check(outs, label):
        off, d12 = 1, np.frombuffer(outs[3], dtype="<u2")
        for i, want in enumerate(model):
            g = outs[2][off:off + len(want)]
            assert g == want, (label, "repair of sequence", i)
            assert (int(d12[i]), int(d12[len(model) + i])) == (len(g) - len(g.lstrip(b".")), len(g) - len(g.rstrip(b"."))), (label, i)
            off += len(want) + 1
        assert int(np.frombuffer(outs[4], dtype="<u8")[0]) == n_matches > (1 << 20), (label, "matches", outs[4], n_matches)
        gfa = outs[0].decode()      # (only its line counts are used: what the verifier says it looked at)
        stats = [int(v) for v in np.frombuffer(outs[1], dtype="<u8")]
        assert stats[4] == sum(l[:1] == "S" for l in gfa.split("\n")) and stats[0] == 2 * stats[3], (label, stats)
        _check_extras(outs[5:], label, k, loaded, gfa, None, extras)

    calls.add("build", [k, 2, len(sent), 2, 0, 1, extras],
              [b"".join(bytes(q["fwd"]) for q in sent), arr([q["length"] for q in sent], "<u4"), arr([q["id"] for q in sent], "<u2"),
               "".join(q["filename"] + "\n" for q in sent).encode(), "".join(q["header"] + "\n" for q in sent).encode()], check, label="k=3, 1.3 M bases over AC")


def multi_calls():
    c = Calls()
    for ranks in (2, 3):
        for k, seed in ((5, 3), (11, 7), (31, 11), (51, 2), (125, 6)):
            seqs, fn, hd = seqgen.make_case(seed, k)
            add_build(c, k, seqs, fn, hd, mode=1, ranks=ranks)
            add_build(c, k, seqs, fn, hd, repair=False, mode=1, ranks=ranks)
        seqs, fn, hd = synth_case(6, 20_000, 1_000, 7)
        add_build(c, 51, seqs, fn, hd, mode=1, ranks=ranks)
    return c


# ---- hand-made GFAs: distances, decompress, the verifier ----------------------------------------------------------------------------------
def hand_gfa(U, S, k=5, seed=0):
    """U unitigs (lengths 1, 31-33, 255-257 among short ones), S paths that name unitig 1, unitig U, every 64th unitig, both strands, repeats"""
    rng = random.Random(seed * 1000 + U * 7 + S)
    special = (1, 31, 32, 33, 255, 256, 257)
    e = _Gfa("")
    e.header = f"H\tVN:Z:1.0\tKM:i:{k}"
    lens = [special[u % 7] if u % 5 == 0 or U < 70 else rng.randint(1, 9) for u in range(U)]
    lens.sort(reverse=True)      # (renumber_unitigs order: longest first)
    segs = [seqgen.rand_seq(rng, n) for n in lens]
    ents = []
    for s in range(S):
        p = [1, -U if s % 2 else U] + [u if (u // 64 + s) % 2 else -u for u in range(64, U + 1, 64)]
        p += [rng.choice((-1, 1)) * rng.randint(1, U) for _ in range(rng.choice((0, 1, 5, 40)))]
        p += p[:3]      # repeats
        if s % 4 == 3: p = [-v for v in reversed(p)]
        ents.append(p)
    e.segs = [[q, [f"DP:f:{sum(abs(x) == i + 1 for p in ents for x in p):.2f}"]] for i, q in enumerate(segs)]
    links = set()
    for p in ents:
        for a, b in zip(p, p[1:]):
            links.add((a, b)); links.add((-b, -a))
    e.links = sorted(links)
    plain = [b"".join(e.strand_seq(v).encode() for v in p) for p in ents]
    e.paths = [[str(i + 1), p, [f"LN:i:{len(plain[i])}", f"FN:Z:hand_{i % 3}.fasta", f"HD:Z:contig_{i}"]] for i, p in enumerate(ents)]
    e.resort()
    return e, plain


def gfa_calls():
    c = Calls()
    combos = [(U, S) for U in (1, 63, 64, 65) for S in (1, 2, 17, 65)] + [(4095, 2), (4096, 17), (4097, 1), (4097, 65)]
    for U, S in combos:
        k = 5
        e, plain = hand_gfa(U, S, k)
        text = e.text()
        loaded = [dict(fwd=b"." * (k // 2) + q + b"." * (k // 2), length=len(q), id=i + 1) for i, q in enumerate(plain)]
        detail = {}
        mod = verify_model.verify(verify_model.from_gfa(e), plain, k, detail)
        dist = O.pairwise_distances(text)
        extras = EX_DIST | EX_DECOMP_DEVICE | EX_DECOMP_SEQ | EX_VERIFY
        check = (lambda outs, label, k=k, loaded=loaded, text=text, dist=dist, mod=mod, detail=detail, extras=extras:
                 _check_extras(outs, label, k, loaded, text, dist, extras, (mod, detail)))
        c.add("gfa_ops", [k, len(loaded), extras], [text.encode(), b"".join(q["fwd"] for q in loaded), arr([q["length"] for q in loaded], "<u4"),
                                                    arr([q["id"] for q in loaded], "<u2")], check, label=f"U={U} S={S}")
    return c


# ---- trim ---------------------------------------------------------------------------------------------------------------------------------
TRIM_NS = (1, 63, 64, 65, 255, 256, 257, 515, 1025)


def trim_calls():
    c = Calls()
    rng = random.Random(3)
    jobs = []
    for n in TRIM_NS:
        path, w = trim_util.planted_overlap_path(rng, n, max(1, n // 5), n_unitigs=400, hairpin=bool(n % 2 == 0)) if n > 4 else ([rng.choice((-1, 1)) * 3], [5] * 400)
        jobs.append((path, w))
        for mu in sorted({max(1, n - 1), n, n + 1, 5000}):      # max_unitigs below, at and above n
            for skip, a, b in ((True, path, path), (False, trim_util.reverse_path(path), path)):
                want = trim_util.overlap_alignment_numpy(a, b, w, 0.75, mu, skip)

                def check(outs, label, want=want):
                    got = np.frombuffer(outs[0], dtype=np.dtype([("au", "<i4"), ("ai", "<u4"), ("bu", "<i4"), ("bi", "<u4")]))
                    assert [tuple(int(v) for v in r) for r in got] == [tuple(x) for x in want], label
                c.add("overlap_alignment", [n, mu, int(skip), f64_bits(0.75)], [arr(a, "<i4"), arr(b, "<i4"), arr(w, "<u4")], check, label=f"n={n} max_unitigs={mu} skip={skip}")
    # all the paths as one batch of slices, whole and with the batch cut down to two jobs per launch
    paths, w = [p for p, _ in jobs], jobs[-1][1]
    flat, off = [x for p in paths for x in p], np.cumsum([0] + [len(p) for p in paths])
    for mu in (64, 5000):
        want_res, want_sm = trim_util.trim_paths_expected(paths, w, 0.75, mu, align=trim_util.overlap_alignment_numpy)
        for env in ({}, {"AC_TRIM_BATCH_BYTES": str(2 * ((min(mu, 1025) + 1) ** 2 // 8 + 4096))}):
            def check(outs, label, want_res=want_res, want_sm=want_sm, env=env):
                res = (_capi.TrimResult * len(want_res)).from_buffer_copy(outs[0])
                assert [r.as_dict() for r in res] == want_res, label
                sm = [int(v) for v in np.frombuffer(outs[1], dtype="<u4")]
                assert sm[:3] == [want_sm["c_se"], want_sm["c_hp"], want_sm["chosen"]], (label, sm)
                if env: assert sm[3] > 2, (label, "the batch was not cut", sm)
            c.add("trim_path_slices", [len(paths), mu, f64_bits(0.75)], [arr(flat, "<i4"), arr(off, "<u8"), arr(w, "<u4")], check, env, label=f"max_unitigs={mu}")
    return c


# ---- resolve ------------------------------------------------------------------------------------------------------------------------------
RESOLVE_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 300)


def resolve_calls():
    c = Calls()
    rng = random.Random(9)
    n_unitigs = 50
    w = [rng.choice((1, 2, 10, 100, 1000, 5000)) for _ in range(n_unitigs)]
    base = resolve_util.random_path(rng, 300, n_unitigs)
    paths = [resolve_util.edited_copy(rng, base[:n], 0.1, n_unitigs)[:n] if n else [] for n in RESOLVE_LENS]
    paths = [p + resolve_util.random_path(rng, n - len(p), n_unitigs) for p, n in zip(paths, RESOLVE_LENS)]
    pairs = [(a, b) for a in range(len(paths)) for b in range(len(paths))]      # every pairing
    want = [resolve_util.global_alignment_distance_numpy(paths[a], paths[b], w) if paths[a] and paths[b] else
            sum(w[abs(u) - 1] for u in paths[a] + paths[b]) for a, b in pairs]
    flat, off = [x for p in paths for x in p], np.cumsum([0] + [len(p) for p in paths])
    for env in ({}, {"AC_RESOLVE_BATCH_BYTES": "200000"}):
        def check(outs, label, want=want):
            assert [int(v) for v in np.frombuffer(outs[0], dtype="<u4")] == want, label
            assert not any(outs[1]), label
        c.add("path_distances", [len(paths), len(pairs)], [arr(flat, "<i4"), arr(off, "<u8"), arr([a for a, _ in pairs], "<u4"), arr([b for _, b in pairs], "<u4"), arr(w, "<u4")],
              check, env)
    # bridges: random cases of the resolve sweep, and one with bridge paths of the lengths above between two anchors
    cases = [resolve_util.random_case(random.Random(s)) for s in range(6)]
    A, B = n_unitigs + 1, n_unitigs + 2
    long_paths = [[A] + p + [B] for p in paths] + [[-B] + resolve_util.reverse_path(paths[3]) + [-A]]
    cases.append((long_paths, w + [7, 9], None))
    for paths_c, w_c, cw in cases:
        anchors, bridges = resolve_util.resolve_expected(paths_c, w_c, len(w_c), cw, dist=resolve_util.global_alignment_distance_numpy)
        flat, off = [x for p in paths_c for x in p], np.cumsum([0] + [len(p) for p in paths_c])
        for env in ({}, {"AC_RESOLVE_BATCH_BYTES": "200000"}):
            def check(outs, label, anchors=anchors, bridges=bridges):
                assert [int(v) for v in np.frombuffer(outs[0], dtype="<u4")] == anchors, label
                br = (_capi.Bridge * (len(outs[1]) // C.sizeof(_capi.Bridge))).from_buffer_copy(outs[1])
                best = np.frombuffer(outs[2], dtype="<i4").tolist(); de = np.frombuffer(outs[3], dtype="<i4").tolist()
                do = np.frombuffer(outs[4], dtype="<u8").tolist(); dm = np.frombuffer(outs[5], dtype="<u4").tolist()
                got = []
                for b in br:
                    distinct = [(de[do[q]:do[q + 1]], dm[q]) for q in range(b.first_distinct, b.first_distinct + b.n_distinct)]
                    got.append(dict(start=b.start, end=b.end, depth=b.depth, status=b.status, best_path=best[b.best_off:b.best_off + b.best_len] if b.status == 0 else None,
                                    best_total=b.best_total if b.status == 0 else None, distinct_paths=distinct, conflicting=b.conflicting, culled=b.culled, cull_rank=b.cull_rank))
                assert got == bridges, label
            c.add("resolve_bridge_paths", [len(paths_c)], [arr(flat, "<i4"), arr(off, "<u8"), arr(cw, "<u4"), arr(w_c, "<u4")], check, env)
    return c


# ---- components and the merge plan ----------------------------------------------------------------------------------------------------------
GRAPH_NS = (1, 63, 64, 65, 257, 2049)


def _graph_shapes(n):
    """(name, links closed under reverse complement) over unitigs 1 .. n: a chain, a ring, chains with hairpin ends, short pieces"""
    fwd = [(u, u + 1) for u in range(1, n)]
    chain = components_util._both(fwd)
    mixed = components_util._both([(u if u % 3 else -u, (u + 1) if (u + 1) % 3 else -(u + 1)) for u in range(1, n)])
    shapes = [("chain", chain), ("mixed-strand chain", mixed), ("ring", components_util._both(fwd + [(n, 1)])),
              ("hairpins", merge_util.closed_set(fwd + [(n, -n), (-1, 1)])), ("pieces", components_util._both([(u, u + 1) for u in range(1, n) if u % 7]))]
    return [(name, list(dict.fromkeys((int(a), int(b)) for a, b in links))) for name, links in shapes]


def graph_calls():
    c = Calls()
    for n in GRAPH_NS:
        lens = merge_util.shape_lengths(n)
        seqs = [merge_util._seq_of(u + 1, lens[u]) for u in range(n)]
        begin = np.cumsum([0] + lens[:-1])
        dead_last = [1] * (n - 1) + [0]
        for name, links in _graph_shapes(n):
            for alive in (None, dead_last):
                for with_len in (True, False):
                    marked = [u % 5 == 0 for u in range(n)] if with_len else None
                    exp = components_util.model_expected(n, links, lens if with_len else None, alive, marked)

                    def check(outs, label, exp=exp, n=n):
                        o = _capi.Components.__new__(_capi.Components)
                        dt = np.dtype([("first", "<u4"), ("unitigs", "<u4"), ("length", "<u8"), ("links_all", "<u8"), ("links_one_way", "<u8"), ("open_ends", "<u4"),
                                       ("marked", "<u4"), ("circular_loop", "u1")], align=True)
                        o.records = np.frombuffer(outs[0], dtype=dt); o.component_of = np.frombuffer(outs[1], dtype="<u4")
                        o.member_off = np.frombuffer(outs[2], dtype="<u8"); o.members = np.frombuffer(outs[3], dtype="<u4"); o.flags = np.frombuffer(outs[4], dtype="u1")
                        sm = [int(v) for v in np.frombuffer(outs[5], dtype="<u8")]
                        o.summary = dict(zip(("unitigs", "components", "topology", "links_all", "links_one_way", "total_length"), sm))
                        o.topology = ("empty", "fragmented", "linear-open-open", "circular", "linear-hairpin-hairpin", "linear-open-hairpin", "other")[sm[2]]
                        components_util.assert_same(components_util.library_result(o), exp, label)
                    c.add("components", [n, len(links)], [arr(links, "<i4"), arr(lens if with_len else None, "<u4"), arr(alive, "u1"), arr(marked, "u1")], check,
                          label=f"n={n} {name} alive={alive is not None} lengths={with_len}")
                # the merge plan of the same graph, with and without sequences
                live = [l for l in links if alive is None or (abs(l[0]) != n and abs(l[1]) != n)]
                ends = [(1, -1 if name == "hairpins" else (n - 1 if alive else n))] if n > 2 else []
                for with_seqs in (True, False):
                    exp = merge_util.model_expected(n, live, lens, alive, ends, seqs=seqs if with_seqs else None)

                    def check(outs, label, exp=exp, n=n, with_seqs=with_seqs):
                        p = _capi.MergePlan.__new__(_capi.MergePlan)
                        dt = np.dtype([("number", "<u4"), ("members", "<u4"), ("length", "<u8"), ("member_off", "<u8"), ("seq_off", "<u8"), ("depth", "<f8"), ("type", "u1"),
                                       ("loop", "u1")], align=True)
                        p.chains = np.frombuffer(outs[0], dtype=dt); p.members = np.frombuffer(outs[1], dtype="<i4"); p.chain_of = np.frombuffer(outs[2], dtype="<u4")
                        p.fixed = np.frombuffer(outs[3], dtype="u1"); p.sequences = np.frombuffer(outs[4], dtype="u1"); p.links = np.frombuffer(outs[5], dtype="<i4").reshape(-1, 2)
                        sm = [int(v) for v in np.frombuffer(outs[6], dtype="<u8")]
                        p.summary = dict(zip(("chains", "merged_unitigs", "unitigs_after", "links_after", "bases_copied"), sm))
                        merge_util.assert_same(merge_util.library_result(p), exp, label, sequences=with_seqs)
                    c.add("merge_plan", [n, len(live), len(ends)],
                          [arr(live, "<i4"), arr(lens, "<u4"), arr(alive, "u1"), arr(ends if ends else None, "<i4"), b"", b"", b"", b"",
                           b"".join(seqs) if with_seqs else b"", arr(begin, "<u8") if with_seqs else b""], check, label=f"n={n} {name} alive={alive is not None} seqs={with_seqs}")
    return c


# ---- cluster ------------------------------------------------------------------------------------------------------------------------------
def cluster_calls():
    c = Calls()
    for n in (1, 2, 3, 64, 65, 257):
        for normalise in (0, 1):
            asym = cluster_util.grid_matrix(n, 65536, 40 + n)      # multiples of 2^-16: every sum is exact
            ids = list(range(3, 3 + n))
            rec = cluster_util.upgma_recurrence_numpy(cluster_util.symmetrical(asym))
            want_nodes, want_merges = cluster_util.build_nodes(ids, rec, bool(normalise)), cluster_util.id_merges(ids, rec)

            def check(outs, label, want_nodes=want_nodes, want_merges=want_merges):
                nodes = (_capi.ClusterNode * (len(outs[0]) // C.sizeof(_capi.ClusterNode))).from_buffer_copy(outs[0])
                merges = (_capi.ClusterMerge * (len(outs[2]) // C.sizeof(_capi.ClusterMerge))).from_buffer_copy(outs[2])
                assert cluster_util.same_bits([(x.id, x.left, x.right, x.distance) for x in nodes], want_nodes), label
                assert cluster_util.same_bits([(m.a, m.b, m.distance) for m in merges], want_merges), label
                assert struct.unpack("<i", outs[1])[0] == len(want_nodes) - 1, label
            c.add("cluster_tree", [n, normalise], [arr(asym, "<f8"), arr(ids, "<u2")], check, label=f"n={n} normalise={normalise}")
    return c


# ---- read depths --------------------------------------------------------------------------------------------------------------------------
def depth_calls():
    c = Calls()
    for k in (11, 31):
        rng = random.Random(100 + k)
        seqs, links, genome = depth_util.random_graph(rng, 6000, 12, 3)
        links = depth_util.both_directions(links)
        g2 = genome + genome
        # reads whose ends fall on 32- and 2048-position boundaries of the batch's text, an empty read, reads shorter than k, a foreign read
        lens = [32, 31, 33, 0, k - 1, 1, 2048 - 97, 2048, 2049, 64, k, 4096 - 1, 300]
        reads, at = [], 0
        for n in lens:
            reads.append(g2[at % 6000:at % 6000 + n]); at += 211
        reads.append(depth_util.random_seq(rng, 500))
        reads += depth_util.sample_reads(rng, genome, 30, 400)
        batches = [reads[:9], [], reads[9:]]
        chk = depth_util.Checker(k, [(seqs, links)])
        for b in batches: chk.add_reads(b)
        want_tot, want_depth = chk.totals_dict(), chk.depths(0)
        for env in ({}, {"AC_DEPTH_BATCH_BYTES": "4096"}):
            def check(outs, label, want_tot=want_tot, want_depth=want_depth):
                t = dict(zip(("reads", "rejected_reads", "read_bases", "span_bases", "span_kmers", "hits", "distinct_kmers", "repeat_kmers", "batches"),
                             (int(v) for v in np.frombuffer(outs[0], dtype="<u8"))))
                assert {n: t[n] for n in want_tot} == want_tot, (label, t, want_tot)
                d, has = np.frombuffer(outs[1], dtype="<f8"), np.frombuffer(outs[2], dtype="u1")
                got = [float(d[i]) if has[i] else None for i in range(len(d))]
                assert [None if x is None else float(x).hex() for x in got] == [None if x is None else float(x).hex() for x in want_depth], label
            arrays = [b"".join(seqs), arr(np.cumsum([0] + [len(s) for s in seqs[:-1]]), "<u8"), arr([len(s) for s in seqs], "<u4"), arr(links, "<i4")]
            for b in batches:
                arrays += [b"".join(b), arr(np.cumsum([0] + [len(r) for r in b]), "<u8")]
            c.add("depth", [k, len(seqs), len(links), len(batches)], arrays, check, env, label=f"k={k}")
    return c
