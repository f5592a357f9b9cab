"""The definition of wn_demux_scores and wn_demux_pick (include/wavenet_amd.h) on the host, in plain Python
integers: a row-major loop over (score, start) tuples, written independently of the kernel (which runs column by column on packed
words).  tests/test_demux_ref.py holds this file to a brute-force enumeration of all semi-global alignments, to an infix edit
distance and to hand-made tables."""
import numpy as np

NEG = -(1 << 30)              # -infinity
INT_MIN = -(1 << 31)
MAX_WINDOW, MAX_PATTERNS, MAX_PATTERN_LEN, MAX_COST = 512, 1024, 128, 1024


def _minus(c, cost):
    """a cell minus a cost; -infinity is clamped back"""
    return (max(c[0] - cost, NEG), c[1])


def semi_global(pattern, window, match, mismatch, go, ge):
    """(score, start, end) of `pattern` (consumed whole) against `window` (free start and end), in window coordinates.  A cell is the
    tuple (score, -start): Python's own tuple order is then the lexicographic maximum on (score, -start)."""
    P, W = len(pattern), len(window)
    assert P >= 1
    prev_H = [(0, -j) for j in range(W + 1)]                         # row 0
    prev_F = [(NEG, 0)] * (W + 1)
    for i in range(1, P + 1):
        border = (-(go + (i - 1) * ge), 0)
        H, F, E = [border], [border], (NEG, 0)
        for j in range(1, W + 1):
            E = max(_minus(H[j - 1], go), _minus(E, ge))
            f = max(_minus(prev_H[j], go), _minus(prev_F[j], ge))
            d = prev_H[j - 1]
            d = (d[0] + (match if pattern[i - 1] == window[j - 1] else mismatch), d[1])
            H.append(max(d, E, f))
            F.append(f)
        prev_H, prev_F = H, F
    score, neg_start, neg_end = max((prev_H[j][0], prev_H[j][1], -j) for j in range(W + 1))
    return score, -neg_start, -neg_end


def demux_scores_ref(labels, lengths, patterns, pattern_lengths, n_front, window, match, mismatch, go, ge, max_len=None,
                     max_pattern_len=None):
    """dict of score, start, end [B, K] int32 and bad (the poisoned entries); labels [B, >= max_len], patterns [K, >= max_pattern_len]"""
    labels, patterns = np.asarray(labels), np.asarray(patterns)
    B, K = len(lengths), len(pattern_lengths)
    max_len = labels.shape[1] if max_len is None else max_len
    max_pattern_len = patterns.shape[1] if max_pattern_len is None else max_pattern_len
    assert 0 <= ge <= go <= MAX_COST and abs(match) <= MAX_COST and abs(mismatch) <= MAX_COST and 1 <= window <= MAX_WINDOW
    score = np.full((B, K), INT_MIN, dtype=np.int64)
    start = np.full((B, K), -1, dtype=np.int64)
    end = np.full((B, K), -1, dtype=np.int64)
    bad = 0
    for b in range(B):
        n = int(lengths[b])
        row = [int(v) for v in labels[b, :n]] if 0 <= n <= max_len else None
        for k in range(K):
            P = int(pattern_lengths[k])
            if row is None or not 1 <= P <= max_pattern_len:
                bad += 1
                continue
            W = min(n, window)
            off = n - W if k >= n_front else 0
            s, st, en = semi_global([int(v) for v in patterns[k, :P]], row[off:off + W], match, mismatch, go, ge)
            score[b, k], start[b, k], end[b, k] = s, st + off, en + off
    return dict(score=score.astype(np.int32), start=start.astype(np.int32), end=end.astype(np.int32), bad=bad)


def demux_pick_ref(score, start, end, lengths, group, min_score, n_front, min_margin, require_both):
    """dict of barcode [B], trim [B, 2], hits [B, 2, 4], runner_up [B, 2], all int32"""
    score, start, end = np.asarray(score), np.asarray(start), np.asarray(end)
    B, K = score.shape
    barcode = np.full(B, -1, dtype=np.int32)
    trim = np.zeros((B, 2), dtype=np.int32)
    hits = np.full((B, 2, 4), -1, dtype=np.int32)
    runner = np.full((B, 2), INT_MIN, dtype=np.int32)
    for b in range(B):
        passes, hit = [False, False], [None, None]
        for e, ks in enumerate((range(0, n_front), range(n_front, K))):
            cands = [k for k in ks if int(score[b, k]) != INT_MIN]
            if not cands:
                continue
            kb = cands[0]
            for k in cands:                                          # ties to the lower index
                if int(score[b, k]) > int(score[b, kb]):
                    kb = k
            others = [int(score[b, k]) for k in cands if int(group[k]) != int(group[kb])]
            ru = max(others) if others else INT_MIN
            s = int(score[b, kb])
            hit[e] = kb
            hits[b, e] = (kb, s, int(start[b, kb]), int(end[b, kb]))
            runner[b, e] = ru
            passes[e] = s >= int(min_score[kb]) and (ru == INT_MIN or s - ru >= min_margin)
        if require_both:
            if passes[0] and passes[1] and int(group[hit[0]]) == int(group[hit[1]]):
                barcode[b] = int(group[hit[0]])
        elif passes[0] and (not passes[1] or int(hits[b, 0, 1]) >= int(hits[b, 1, 1])):
            barcode[b] = int(group[hit[0]])
        elif passes[1]:
            barcode[b] = int(group[hit[1]])
        t0 = int(hits[b, 0, 3]) if passes[0] else 0
        t1 = max(t0, int(hits[b, 1, 2])) if passes[1] else int(lengths[b])
        trim[b] = (t0, t1)
    return dict(barcode=barcode, trim=trim, hits=hits, runner_up=runner)


def all_semi_global(pattern, window, match, mismatch, go, ge):
    """brute force: (score, start, end) by enumerating EVERY semi-global alignment -- every start s and end e in the window and every
    way of writing pattern against window[s:e] as columns of (pattern label, window label), (pattern label, gap), (gap, window
    label) -- scoring each as a whole (a maximal run of n gap columns of one kind costs go + (n - 1) ge), and keeping the greatest
    (score, -start, -end).  Exponential: for tiny inputs only."""
    P, W = len(pattern), len(window)
    best = None

    def walk(i, j, e, score, run):
        """run: 0 none, 1 a gap in the window (pattern label against a gap), 2 a gap in the pattern"""
        nonlocal best
        if i == P and j == e:
            yield score
            return
        if i < P and j < e:
            yield from walk(i + 1, j + 1, e, score + (match if pattern[i] == window[j] else mismatch), 0)
        if i < P:
            yield from walk(i + 1, j, e, score - (ge if run == 1 else go), 1)
        if j < e and i > 0:                                          # a window label before the pattern's first is not inside [s, e)
            yield from walk(i, j + 1, e, score - (ge if run == 2 else go), 2)

    for s in range(W + 1):
        for e in range(s, W + 1):
            for sc in walk(0, s, e, 0, 0):
                cand = (sc, -s, -e)
                if best is None or cand > best:
                    best = cand
    return best[0], -best[1], -best[2]
