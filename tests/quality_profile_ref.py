"""Reference of the quality profile (csrc/wn_profile.hip) with plain Python loops, and of the calibration
fit in numpy float64.  It restates the definitions; nothing here is shaped like the kernel.

Column c of an op string has reference index i_c = the number of ops before it with a code in {1, 2, 3} and query index j_c =
the number with a code in {1, 2, 4}.  lo / hi are the first / last column whose op is 1 or 2; without count_ends the columns
outside [lo, hi] (every column when there is none) are end columns and enter no table."""
import numpy as np

QUAL_ROWS, DWELL_ROWS = 94, 33
MATCH, MISMATCH, REF_GAP, QUERY_GAP = 1, 2, 3, 4


def tables(classes):
    """zeroed (q_counts, dwell_counts, confusion) as int64 arrays"""
    return (np.zeros((QUAL_ROWS, 3), dtype=np.int64), np.zeros((DWELL_ROWS, 3), dtype=np.int64),
            np.zeros((classes + 1, classes + 1), dtype=np.int64))


def profile_read(ops, ops_len, ref, ref_len, query, query_len, qual, dwell, classes, count_ends, max_ops, max_ref, max_query):
    """One read.  Returns None for a bad read, else (outcome list [query_len], ref_index list [query_len], counts (5),
    entries): entries is a list of (table, row, column) with table in "q", "d", "c"."""
    ops_len, ref_len, query_len = int(ops_len), int(ref_len), int(query_len)
    if not (0 <= ops_len <= max_ops and 0 <= ref_len <= max_ref and 0 <= query_len <= max_query):
        return None
    ops = [int(v) for v in ops[:ops_len]]
    if any(op not in (1, 2, 3, 4) for op in ops):
        return None
    if sum(op != QUERY_GAP for op in ops) != ref_len or sum(op != REF_GAP for op in ops) != query_len:
        return None
    ref = [int(v) for v in ref[:ref_len]]
    query = [int(v) for v in query[:query_len]]
    if any(not 0 <= v < classes for v in ref + query):
        return None
    if qual is not None and any(int(v) > 93 for v in qual[:query_len]):
        return None
    if dwell is not None and any(int(v) < 0 for v in dwell[:query_len]):
        return None
    aligned = [c for c, op in enumerate(ops) if op in (MATCH, MISMATCH)]
    if count_ends:
        lo, hi = 0, len(ops) - 1
    elif aligned:
        lo, hi = aligned[0], aligned[-1]
    else:
        lo, hi = len(ops), -1                                        # every column is an end column
    outcome, ref_index = [0] * query_len, [-1] * query_len
    counts, entries = [0] * 5, []
    i = j = 0
    for c, op in enumerate(ops):
        end = not lo <= c <= hi
        if op in (MATCH, MISMATCH):
            if (ref[i] == query[j]) != (op == MATCH):
                return None
            outcome[j], ref_index[j] = op, i
            counts[op - 1] += 1
            entries.append(("c", ref[i], query[j]))
            col = op - 1
        elif op == QUERY_GAP:
            outcome[j] = 4 if end else 3
            if not end:
                counts[2] += 1
                entries.append(("c", classes, query[j]))
            col = 2
        else:
            if not end:
                counts[3] += 1
                entries.append(("c", ref[i], classes))
            col = None
        if end:
            counts[4] += 1
        elif col is not None:
            if qual is not None:
                entries.append(("q", int(qual[j]), col))
            if dwell is not None:
                entries.append(("d", min(int(dwell[j]), DWELL_ROWS - 1), col))
        i += op != QUERY_GAP
        j += op != REF_GAP
    return outcome, ref_index, counts, entries


def profile(ops, ops_len, ref, ref_len, query, query_len, qual=None, dwell=None, classes=5, count_ends=False, into=None,
            max_ops=None):
    """A batch: rows of ops / ref / query (lists or 2-d arrays) with their lengths.  Returns a dict: q_counts, dwell_counts,
    confusion (int64, accumulated into `into` = (q, d, c) when given; q / d are None without qual / dwell), read_counts [B, 5]
    int32, outcome [B, M] uint8, ref_index [B, M] int32, bad."""
    B = len(ops)
    N, M = np.shape(ref)[1], np.shape(query)[1]
    max_ops = min(np.shape(ops)[1], N + M) if max_ops is None else max_ops
    q_counts, dwell_counts, confusion = tables(classes) if into is None else into
    if qual is None:
        q_counts = None
    if dwell is None:
        dwell_counts = None
    which = {"q": q_counts, "d": dwell_counts, "c": confusion}
    read_counts = np.zeros((B, 5), dtype=np.int32)
    outcome = np.zeros((B, M), dtype=np.uint8)
    ref_index = np.full((B, M), -1, dtype=np.int32)
    bad = 0
    for b in range(B):
        got = profile_read(ops[b], ops_len[b], ref[b], ref_len[b], query[b], query_len[b], None if qual is None else qual[b],
                           None if dwell is None else dwell[b], classes, count_ends, max_ops, N, M)
        if got is None:
            read_counts[b] = -1
            bad += 1
            continue
        out, idx, counts, entries = got
        outcome[b, :len(out)] = out
        ref_index[b, :len(idx)] = idx
        read_counts[b] = counts
        for name, row, col in entries:
            which[name][row, col] += 1
    return dict(q_counts=q_counts, dwell_counts=dwell_counts, confusion=confusion, read_counts=read_counts, outcome=outcome,
                ref_index=ref_index, bad=bad)


def fit(q_counts, min_count=100):
    """numpy float64: (qscale, qbias, bins_used, bases_used, q_empirical [94], NaN where a bin is unused); None for the first two
    when fewer than two bins are used"""
    t = np.asarray(q_counts, dtype=np.float64)
    n = t.sum(axis=1)
    used = n >= min_count
    q_emp = np.full(QUAL_ROWS, np.nan)
    q_emp[used] = -10.0 * np.log10((t[used, 1] + t[used, 2] + 0.5) / (n[used] + 1.0))
    if used.sum() < 2:
        return None, None, int(used.sum()), int(n[used].sum()), q_emp
    q, w, qe = np.arange(QUAL_ROWS, dtype=np.float64)[used], n[used], q_emp[used]
    q_mean, qe_mean = (w * q).sum() / w.sum(), (w * qe).sum() / w.sum()
    slope = (w * (q - q_mean) * (qe - qe_mean)).sum() / (w * (q - q_mean) ** 2).sum()
    return float(slope), float(qe_mean - slope * q_mean), int(used.sum()), int(w.sum()), q_emp


def planted_table(a, b, n=200000, q_lo=5, q_hi=40, extra=(60, 99)):
    """a q_counts table whose empirical quality follows Qe = a q + b: bins q_lo..q_hi with n bases each, round(n 10^(-(a q + b)/10))
    of them errors, a third of those insertions; and one bin `extra[0]` of `extra[1]` bases, all errors, which a fit with
    min_count = 100 must ignore"""
    t = np.zeros((QUAL_ROWS, 3), dtype=np.int64)
    for q in range(q_lo, q_hi + 1):
        err = int(round(n * 10.0 ** (-(a * q + b) / 10.0)))
        ins = err // 3
        t[q] = (n - err, err - ins, ins)
    if extra is not None:
        t[extra[0]] = (0, extra[1], 0)
    return t
