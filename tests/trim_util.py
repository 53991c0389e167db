"""Test-side checker of ac_trim_paths / ac_overlap_alignment, written from the specification of the feature (the issue text), not from
the library: (a) overlap_alignment_plain — a triple loop over Python integers; (b) overlap_alignment_numpy — anti-diagonals of int64 for
large k.  Both hold DOUBLED scores (every score of the reference is a multiple of 0.5).  The trimming rules on top take either.

Paths are lists of signed unitig numbers; `w` maps |unitig| -> length (a dict, or a sequence indexed by number - 1)."""
import json
from pathlib import Path

import numpy as np

GAP, NONE = 0, 0xFFFFFFFF
NEG_INF = float("-inf")
KATS = Path(__file__).resolve().parent / "golden" / "trim_kats.json"


def load_kats():
    k = json.loads(KATS.read_text())
    for group in ("overlap_alignment", "start_end", "hairpin_end", "hairpin_start", "hairpin_start_then_end"):
        for c in k[group]:
            c["weights"] = {int(u): x for u, x in c["weights"].items()}
    return k


def weight_of(w, u):
    return w[abs(u)] if isinstance(w, dict) else w[abs(u) - 1]


def reverse_path(p):
    return [-u for u in reversed(p)]


def _traceback(a, b, w, n, k, right_col, up_ge_left, min_identity):
    """right_col[i] = doubled S[i][k] (i = 1..k; index 0 unused); up_ge_left(i, j) = S[i-1][j] >= S[i][j-1]."""
    best, bi = NEG_INF, 0
    for i in range(1, k + 1):
        if right_col[i] > best:
            best, bi = right_col[i], i
    if best <= 0:
        return []
    i, j, pieces = bi, k, []
    while i > 0 and j > 0:
        gi, gj = i - 1, n - k + j - 1
        if a[gi] == b[gj]:
            pieces.append((a[gi], gi, b[gj], gj)); i -= 1; j -= 1
        elif up_ge_left(i, j):
            pieces.append((a[gi], gi, GAP, NONE)); i -= 1
        else:
            pieces.append((GAP, NONE, b[gj], gj)); j -= 1
    if i > 0:
        return []
    pieces.reverse()
    matches = sum(weight_of(w, p[0]) for p in pieces if p[0] == p[2])
    len_a = sum(weight_of(w, p[0]) for p in pieces if p[0] != GAP)
    len_b = sum(weight_of(w, p[2]) for p in pieces if p[2] != GAP)
    mean = (float(len_a) + float(len_b)) / 2.0
    identity = float(matches) / mean if mean != 0.0 else float("nan")
    if identity < min_identity:
        return []
    return pieces


def overlap_alignment_plain(a, b, w, min_identity, max_unitigs, skip_diagonal):
    """(a): the matrix as the specification states it, doubled, in Python integers (-inf for the skipped cells)."""
    assert len(a) == len(b)
    n = len(a)
    k = min(max_unitigs, n)
    S = [[NEG_INF] * (k + 1) for _ in range(k + 1)]
    for i in range(k + 1):
        S[i][0] = 0; S[0][i] = 0
    for i in range(1, k + 1):
        gi = i - 1
        wa = weight_of(w, a[gi])
        for j in range(1, k + 1):
            gj = n - k + j - 1
            if skip_diagonal and gi == gj:
                continue
            wb = weight_of(w, b[gj])
            m = S[i - 1][j - 1] + (2 * wa if a[gi] == b[gj] else -(wa + wb))
            S[i][j] = max(m, S[i - 1][j] - 2 * wa, S[i][j - 1] - 2 * wb)
    return _traceback(a, b, w, n, k, [S[i][k] for i in range(k + 1)], lambda i, j: S[i - 1][j] >= S[i][j - 1], min_identity)


def overlap_alignment_numpy(a, b, w, min_identity, max_unitigs, skip_diagonal):
    """(b): the same matrix by anti-diagonals of int64; keeps the comparison bit of every cell and the right-edge column only.
    The skipped cells hold -2^61: below every finite doubled score (|score| < 2^35) also after 2 k subtractions, and never >= a finite one."""
    assert len(a) == len(b)
    n = len(a)
    k = min(max_unitigs, n)
    if k == 0:
        return []
    NEG = -(1 << 61)
    A = np.asarray(a[:k], dtype=np.int64); B = np.asarray(b[n - k:], dtype=np.int64)
    WA = np.asarray([weight_of(w, u) for u in a[:k]], dtype=np.int64); WB = np.asarray([weight_of(w, u) for u in b[n - k:]], dtype=np.int64)
    bits = np.zeros((k + 1, k + 1), dtype=np.bool_)
    right = np.full(k + 1, NEG, dtype=np.int64)

    def border(d):      # diagonal d as an array over i = 0..k: the cells of row 0 / column 0 are 0, the rest not yet known
        v = np.full(k + 1, NEG, dtype=np.int64)
        if 0 <= d <= k:
            v[0] = 0; v[d] = 0
        return v
    d2, d1 = border(0), border(1)
    for d in range(2, 2 * k + 1):
        cur = border(d)
        lo, hi = max(1, d - k), min(k, d - 1)
        i = np.arange(lo, hi + 1); j = d - i
        up = d1[i - 1]; left = d1[i]; diag = d2[i - 1]
        wa = WA[i - 1]; wb = WB[j - 1]
        m = diag + np.where(A[i - 1] == B[j - 1], 2 * wa, -(wa + wb))
        v = np.maximum(np.maximum(m, up - 2 * wa), left - 2 * wb)
        if skip_diagonal:
            v = np.where((i - 1) == (n - k + j - 1), NEG, v)
        cur[lo:hi + 1] = v
        bits[i, j] = up >= left
        if hi == k or d - k >= 1:      # the cell of column k on this diagonal: i = d - k
            ik = d - k
            if 1 <= ik <= k:
                right[ik] = cur[ik]
        d2, d1 = d1, cur
    col = [NEG_INF] + [NEG_INF if int(x) <= NEG // 2 else int(x) for x in right[1:]]
    return _traceback(a, b, w, n, k, col, lambda i, j: bool(bits[i, j]), min_identity)


# ---- the trimming rules; each returns (status, begin, end): status 0 not trimmed, 1 trimmed, 2 the reference's own check would fire ----
def start_end_slice(p, w, min_identity, max_unitigs, align=overlap_alignment_plain):
    al = align(p, p, w, min_identity, max_unitigs, True)
    if not al:
        return 0, 0, len(p)
    total = sum((weight_of(w, x[0]) if x[0] != GAP else 0) + (weight_of(w, x[2]) if x[2] != GAP else 0) for x in al)
    cum, best, best_close = 0, 0, 1.0
    for idx, x in enumerate(al):
        if x[0] != GAP:
            cum += weight_of(w, x[0])
        if x[2] != GAP:
            cum += weight_of(w, x[2])
        close = abs(0.5 - (float(cum) / float(total)))
        if x[0] == x[2] and close < best_close:
            best, best_close = idx, close
    s, e = al[best][1], al[best][3]
    if s == NONE or e == NONE or s > e:
        return 2, 0, len(p)
    return 1, s, e


def hairpin_end_slice(p, w, min_identity, max_unitigs, align=overlap_alignment_plain):
    al = align(reverse_path(p), p, w, min_identity, max_unitigs, False)
    if not al:
        return 0, 0, len(p)
    al, end = list(al), 0
    while al:
        while al and al[0][0] == GAP:
            al.pop(0)
        while al and al[-1][2] == GAP:
            al.pop()
        if not al:
            break
        last = al.pop()
        if not al or last[2] != -al[0][0]:
            return 2, 0, len(p)
        if last[0] != GAP:
            end = last[3]
        al.pop(0)
    return 1, 0, end


def hairpin_start_slice(p, w, min_identity, max_unitigs, align=overlap_alignment_plain):
    st, _, end = hairpin_end_slice(reverse_path(p), w, min_identity, max_unitigs, align)
    if st != 1:
        return st, 0, len(p)
    return 1, len(p) - end, len(p)


def slice_length(p, w, b, e):
    return sum(weight_of(w, u) for u in p[b:e])


def trim_paths_expected(paths, w, min_identity, max_unitigs, align=overlap_alignment_plain):
    """What Graph.trim_paths / trim_path_slices must return: (results, summary without the measured fields)."""
    res, c_se, c_hp = [], 0, 0
    for p in paths:
        n = len(p)
        full = dict(status=0, begin=0, end=n, trimmed_length=slice_length(p, w, 0, n))
        r = dict(start_end=dict(full), hairpin=dict(full), hairpin_start_trimmed=0, hairpin_end_trimmed=0)
        if max_unitigs > 0:
            st, b, e = start_end_slice(p, w, min_identity, max_unitigs, align)
            if st:
                r["start_end"] = dict(status=st, begin=b, end=e, trimmed_length=slice_length(p, w, b, e))
            hs, hb, he = hairpin_start_slice(p, w, min_identity, max_unitigs, align)
            status = 2 if hs == 2 else 0
            if hs == 1:
                r["hairpin_start_trimmed"] = 1
            if status != 2:
                q = p[hb:he]
                es, _, ee = hairpin_end_slice(q, w, min_identity, max_unitigs, align)
                if es == 2:
                    status = 2
                elif es == 1:
                    r["hairpin_end_trimmed"] = 1
                    he = hb + ee
            if status == 2:
                r["hairpin_start_trimmed"] = r["hairpin_end_trimmed"] = 0
                r["hairpin"] = dict(full, status=2)
            elif r["hairpin_start_trimmed"] or r["hairpin_end_trimmed"]:
                r["hairpin"] = dict(status=1, begin=hb, end=he, trimmed_length=slice_length(p, w, hb, he))
        c_se += r["start_end"]["status"] == 1
        c_hp += r["hairpin"]["status"] == 1
        res.append(r)
    chosen = 0 if c_se == 0 and c_hp == 0 else (1 if c_se >= c_hp else 2)
    return res, dict(c_se=c_se, c_hp=c_hp, chosen=chosen)


# ---- generators ---------------------------------------------------------------------------------------------------------------------
SWEEP_WEIGHTS = (1, 2, 10, 100, 1000)


def random_case(rng, n_lo=2, n_hi=120):
    """One case of the random sweep: a path of n_lo..n_hi entries over 2-12 unitigs with weights from SWEEP_WEIGHTS, with a planted start-end
    repeat or hairpin (one foreign unitig inserted) in most of them.  Returns (path, weights list, min_identity, max_unitigs)."""
    U = rng.randint(2, 12)
    w = [rng.choice(SWEEP_WEIGHTS) for _ in range(U + 1)]      # unitig U + 1 is the foreign one
    n = rng.randint(n_lo, n_hi)
    rnd = lambda m: [rng.choice((-1, 1)) * rng.randint(1, U) for _ in range(m)]
    kind = rng.randint(0, 3)
    if kind == 0 or n < 4:
        p = rnd(n)
    else:
        m = rng.randint(1, max(1, n // 3))
        core = rnd(n - m)
        rep = list(core[:m]) if kind == 1 else (reverse_path(core[-m:]) if kind == 2 else None)
        if kind == 3:
            rep = reverse_path(core[:m])
        if len(rep) > 1 and rng.random() < 0.6:
            rep.insert(rng.randint(1, len(rep) - 1), U + 1)
            rep = rep[:m] if rng.random() < 0.5 else rep
        p = (rep + core) if kind == 3 else (core + rep)
    return p, w, rng.choice((0.2, 0.5, 0.9, 0.95)), rng.choice((1, 3, 8, 1000))


def planted_overlap_path(rng, n, overlap, n_unitigs=4000, noise=0.03, hairpin=False):
    """A path of n entries whose last `overlap` entries repeat its first ones (or, hairpin: mirror the entries before them) with a share
    `noise` of substituted / dropped / inserted entries.  Returns (path, weights list)."""
    w = [rng.choice((1, 5, 20, 50, 100, 400, 1500)) for _ in range(n_unitigs)]
    rnd = lambda: rng.choice((-1, 1)) * rng.randint(1, n_unitigs)
    core = [rnd() for _ in range(n - overlap)]
    src = core[:overlap] if not hairpin else reverse_path(core[-overlap:])
    rep = []
    for u in src:
        x = rng.random()
        if x < noise / 3:
            continue
        if x < 2 * noise / 3:
            rep.append(rnd()); continue
        rep.append(u)
        if x < noise:
            rep.append(rnd())
    rep = (rep + [rnd() for _ in range(overlap)])[:overlap] if len(rep) < overlap else rep[:overlap]
    return core + rep, w
