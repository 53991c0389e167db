"""The model the trim-apply tests hold the library to: trim.rs:189-269 restated step by step in plain Python, on the four lists the reference
keeps (unitigs, links, positions, sequences), in its order:
  choose_trim_type (:189-226)          the counts, the winner, and per trimmed sequence remove_sequence_from_graph followed by
                                       create_sequence_and_positions with its "Position calculation mismatch" assertion (unitig_graph.rs:173)
  exclude_outliers_in_length (:229-257) median_isize / mad_isize, f64::round, `as usize`, remove_sequence_from_graph for the excluded
  clean_up_graph (:260-269)            recalculate_depths, remove_zero_depth_unitigs, merge_linear_paths, renumber_unitigs
  save_gfa(.., false) and save_metrics the text and TrimmedClusterMetrics as serde_yaml prints it
Positions are edited literally; from recalculate_depths on, the steps are those of subset_util / merge_util / finish_util, which are
imported and not edited (their position lists are checked against the edited ones first).  It shares no code with kernels_trim_apply.inc
or trim_apply_host.cpp."""
import json
import math
from pathlib import Path

import numpy as np

import finish_util as F
import merge_util as M
import subset_util as S

KATS = Path(__file__).resolve().parent / "golden" / "trim_apply_kats.json"
FORWARD, REVERSE = True, False
U64_MAX = 2 ** 64 - 1


class ModelError(Exception):
    pass


def load_kats():
    return json.loads(KATS.read_text())


# ---- misc.rs:423-457 -----------------------------------------------------------------------------------------------------------------------
def median_int(values):
    if not values:
        return 0
    v = sorted(values)
    n = len(v)
    if n % 2 == 0:
        total = v[n // 2 - 1] + v[n // 2]
        return int(total / 2) if total < 0 else total // 2      # (Rust's integer division truncates)
    return v[n // 2]


def mad_int(values):
    if not values:
        return 0
    m = median_int(values)
    return median_int([abs(v - m) for v in values])


def round_as_usize(x):
    """f64::round (half away from zero), then `as usize` (saturating, NaN = 0)"""
    if math.isnan(x):
        return 0
    r = math.floor(abs(x) + 0.5)
    r = -r if x < 0 else r
    return min(max(int(r), 0), U64_MAX)


def length_range(lengths, threshold):
    """(median, mad, min, max); the range is everything when the threshold is 0.0 (exclude_outliers_in_length returns at once)"""
    median, mad = median_int(lengths), mad_int(lengths)
    if threshold == 0.0:
        return median, mad, 0, U64_MAX
    return median, mad, round_as_usize(float(median) - float(mad) * threshold), round_as_usize(float(median) + float(mad) * threshold)


def choose_trim_type(results):
    """(kind or None, c_se, c_hp): status 2 counts as not trimmed"""
    if results is None:
        return None, 0, 0
    c_se, c_hp = sum(r["start_end"]["status"] == 1 for r in results), sum(r["hairpin"]["status"] == 1 for r in results)
    if c_se == 0 and c_hp == 0:
        return None, c_se, c_hp
    return ("start_end" if c_se >= c_hp else "hairpin"), c_se, c_hp


# ---- the graph's position lists, edited as the reference edits them ---------------------------------------------------------------------------
def remove_sequence_from_graph(positions, seq_id):
    for key in positions:
        positions[key] = [p for p in positions[key] if p[0] != seq_id]


def create_sequence_and_positions(positions, lens, seq_id, length, path):
    forward_path = [(abs(e), e > 0) for e in path]
    reverse_path = [(num, not strand) for num, strand in reversed(forward_path)]
    for p, strand in ((forward_path, FORWARD), (reverse_path, REVERSE)):
        try:
            pos = S.add_positions_from_path(positions, lens, p, strand, seq_id)
        except KeyError as e:
            raise ModelError(str(e)) from e
        if pos != length:
            raise ModelError(f"Position calculation mismatch: sequence {seq_id}")


def trim_apply_model(n, links, lens, paths, seq_lengths, results, chosen="auto", mad=5.0, alive=None, seqs=None, types=None):
    """-> dict(kind, c_se, c_hp, records [(begin, end, length, trimmed, excluded)], median, mad, min, max, kept, cluster (subset_util's model of the
    trimmed graph before the merge), model (finish_util's printed graph), lengths)"""
    if mad < 0:
        raise ModelError("--mad cannot be less than 0")
    numbers = [u for u in range(1, n + 1) if alive is None or alive[u - 1]]
    positions = {(u, s): [] for u in numbers for s in (FORWARD, REVERSE)}
    for s, p in enumerate(paths):      # load_graph: the untrimmed sequences
        create_sequence_and_positions(positions, lens, s, seq_lengths[s], p)
    kind, c_se, c_hp = choose_trim_type(results)
    if chosen != "auto":
        kind = None if chosen in ("none", None) else chosen
    records, sliced, lengths = [], [], []
    for s, p in enumerate(paths):
        r = results[s][kind] if kind is not None else None
        if r is not None and r["status"] == 1:
            if r["begin"] > r["end"] or r["end"] > len(p):
                raise ModelError(f"slice of sequence {s}")
            remove_sequence_from_graph(positions, s)
            create_sequence_and_positions(positions, lens, s, r["trimmed_length"], p[r["begin"]:r["end"]])
            records.append([r["begin"], r["end"], r["trimmed_length"], 1, 0]); sliced.append(list(p[r["begin"]:r["end"]])); lengths.append(r["trimmed_length"])
        else:
            records.append([0, len(p), seq_lengths[s], 0, 0]); sliced.append(list(p)); lengths.append(seq_lengths[s])
    median, dev, lo, hi = length_range(lengths, mad)
    for s, length in enumerate(lengths):
        if not lo <= length <= hi:
            records[s][4] = 1
            remove_sequence_from_graph(positions, s)
    kept = [s for s in range(len(paths)) if not records[s][4]]
    for s in kept:
        if not sliced[s]:
            raise ModelError(f"sequence {s} has no starting unitig")
    # clean_up_graph: recalculate_depths and remove_zero_depth_unitigs as subset_util restates them, on position lists equal to the edited ones
    labels = [0 if r[4] else 1 for r in records]
    cluster = S.model_cluster(n, links, lens, alive, sliced, labels, 1)
    for key in positions:
        assert sorted(positions[key]) == sorted(cluster["positions"][key]), key
    plan = S.model_merge(cluster, seqs)
    merged_paths = S.model_merged_paths(cluster, plan)
    graph, _ = F.model_graph(n, cluster["links"], lens, cluster["alive"], cluster["path_ends"], cluster["depth"], cluster["fwd"], cluster["rev"], types, seqs)
    model, _ = F.finish_model(graph, n, True, merged_paths)
    return dict(kind=kind, c_se=c_se, c_hp=c_hp, records=[tuple(r) for r in records], median=median, mad=dev, min=lo, max=hi, kept=kept, cluster=cluster,
                model=model, lengths=lengths, rejected=sum(r["start_end"]["status"] == 2 or r["hairpin"]["status"] == 2 for r in results or []))


def model_gfa(exp, k, ids, filenames, headers, cluster_tags=None):
    """save_gfa(&trimmed_gfa, &sequences, false): the kept sequences' P lines in input order with their new lengths"""
    metas = [(s, ids[s], exp["lengths"][s], filenames[s], headers[s], cluster_tags[s] if cluster_tags else 0) for s in exp["kept"]]
    return F.save_gfa(exp["model"], k, metas, use_other_colour=False)


def model_yaml(exp):
    """TrimmedClusterMetrics::new (metrics.rs:221-230) through serde_yaml 0.9"""
    kept = [exp["lengths"][s] for s in exp["kept"]]
    lines = [f"trimmed_cluster_size: {len(kept)}"]
    lines += ["trimmed_cluster_lengths: []"] if not kept else ["trimmed_cluster_lengths:"] + [f"- {v}" for v in kept]
    lines += [f"trimmed_cluster_median: {median_int(kept) & 0xFFFFFFFF}", f"trimmed_cluster_mad: {mad_int(kept) & 0xFFFFFFFF}"]
    return ("\n".join(lines) + "\n").encode()


# ---- helpers of the tests -----------------------------------------------------------------------------------------------------------------------
def seq_arrays(seqs):
    """unitig sequences as (all bytes + one spare, first byte per unitig)"""
    begin = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs) > 1:
        begin[1:] = np.cumsum([len(s) for s in seqs[:-1]], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8), begin


def no_trim(n_seqs):
    return [dict(start_end=dict(status=0, begin=0, end=0, trimmed_length=0), hairpin=dict(status=0, begin=0, end=0, trimmed_length=0)) for _ in range(n_seqs)]


def with_slice(results, s, kind, begin, end, length, status=1):
    results[s][kind] = dict(status=status, begin=begin, end=end, trimmed_length=length)
    return results


def path_links(paths):
    """the links a set of paths needs, one direction each (merge_util.closed_set closes them)"""
    out = []
    for p in paths:
        for a, b in zip(p, p[1:]):
            if (a, b) not in out and (-b, -a) not in out:
                out.append((a, b))
    return out
