#!/usr/bin/env python3
"""Times the read tally of the read-based unitig depths (ac_depth_add_reads) on one MI355X, without torch: a random assembly, synthetic
reads sampled from it (5 % substitutions, both strands, a fifth of them foreign), host memory in, counts on the device.

    AC_NO_TORCH=1 python tools/depth_bench.py [--assembly 5000000] [--read-bases 500000000] [--read-length 10000] [--kmer 21] [--out FILE]

Reports read bases per second end to end, the device time of pass 1 + accept + pass 2 (device events), the rate of a pinned host-to-device
copy, and the probe rate as a fraction of the device's random 8-byte read ceiling at the table's size (ac_random_access_ceilings_at): one
read position is one random probe, so that ceiling — not HBM bandwidth — is what the kernel is priced against."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("AC_NO_TORCH", "1")


def make_reads(np, rs, genome, total, length):
    """one uint8 array of all reads and their offsets: stretches of the genome with substitutions, every fifth read random"""
    n = max(1, total // length)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    starts = rs.randint(0, len(genome) - length, n)
    bases = np.empty(n * length, dtype=np.uint8)
    chunk = max(1, (64 << 20) // length)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        idx = starts[a:b, None] + np.arange(length)[None, :]
        blk = genome[idx]
        m = rs.random_sample(blk.shape) < 0.05
        blk[m] = acgt[rs.randint(0, 4, int(m.sum()))]
        rev = rs.random_sample(b - a) < 0.5
        blk[rev] = comp[blk[rev][:, ::-1]]
        foreign = (np.arange(a, b) % 5) == 4
        blk[foreign] = acgt[rs.randint(0, 4, (int(foreign.sum()), length))]
        bases[a * length:b * length] = blk.reshape(-1)
    return bases, off


def upload_rate(hip, nbytes=256 << 20, repeats=5):
    """GB/s of a pinned host -> device copy (best of `repeats` after a warm-up)"""
    h, d = C.c_void_p(), C.c_void_p()
    assert hip.hipHostMalloc(C.byref(h), C.c_size_t(nbytes), 0) == 0 and hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
    C.memset(h, 1, nbytes)
    best = 0.0
    for i in range(repeats + 1):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(d, h, C.c_size_t(nbytes), 1) == 0 and hip.hipDeviceSynchronize() == 0
        dt = time.perf_counter() - t0
        if i:
            best = max(best, nbytes / dt / 1e9)
    hip.hipFree(d); hip.hipHostFree(h)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assembly", type=int, default=5_000_000)
    ap.add_argument("--read-bases", type=int, default=500_000_000)
    ap.add_argument("--read-length", type=int, default=10_000)
    ap.add_argument("--kmer", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu), small sizes only")
    ap.add_argument("--out", type=str, default=None, help="append the result line to this JSON-lines file")
    args = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi
    if args.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path, hip = emu_lib.emu_path(), None
    else:
        lib_path, hip = None, C.CDLL("libamdhip64.so.7")
    lib = _capi.load_library(lib_path)
    rs = np.random.RandomState(1)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, args.assembly)]
    bases, off = make_reads(np, rs, genome, args.read_bases, args.read_length)
    rd = _capi.ReadDepth(args.kmer, [([genome.tobytes()], [])], lib_path=lib_path)
    rd.add_reads_raw(bases[:int(off[min(len(off) - 1, 64)])], off[:min(len(off), 65)])      # warm-up: code objects, staging buffers
    runs = []
    for _ in range(args.repeats):
        before = rd.totals()
        t0 = time.perf_counter()
        rd.add_reads_raw(bases, off)
        wall = time.perf_counter() - t0
        after = rd.totals()
        runs.append(dict(wall_s=wall, device_s=after["seconds_device"] - before["seconds_device"], batches=after["batches"] - before["batches"]))
    best = min(runs, key=lambda r: r["wall_s"])
    t = rd.totals()
    positions = len(bases) + len(off) - 1
    res = dict(tool="depth_bench", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(), kmer=args.kmer, assembly_bp=args.assembly,
               read_bases=int(len(bases)), read_length=args.read_length, reads=len(off) - 1, table_slots=t["table_slots"], distinct_kmers=t["distinct_kmers"],
               accepted_share=t["reads"] / max(1, t["reads"] + t["rejected_reads"]), runs=runs,
               end_to_end_gbases_per_s=len(bases) / best["wall_s"] / 1e9, device_gbases_per_s=len(bases) / best["device_s"] / 1e9,
               probe_gops=positions / best["device_s"] / 1e9)
    if hip is not None:
        cas, rdc = C.c_double(), C.c_double()
        lib.ac_random_access_ceilings_at.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        assert lib.ac_random_access_ceilings_at(0, C.c_uint64(t["table_slots"]), C.byref(cas), C.byref(rdc)) == 0, lib.ac_last_error()
        res.update(read_ceiling_gops=rdc.value, probe_share_of_read_ceiling=res["probe_gops"] / rdc.value if rdc.value else None,
                   upload_pinned_gb_per_s=upload_rate(hip), packed_upload_bytes_per_base=0.5)
    rd.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
