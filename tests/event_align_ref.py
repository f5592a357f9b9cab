"""The definition of wn_event_align (include/wavenet_amd.h) on the host: the banded minimum-cost path of the
detected events of a read over the k-mers of its known bases, with stays, steps and skips of one or two k-mers at a cost each.
`event_cost` is the definition in Python integers and nothing else computes a cost here: a row of states is a numpy object array of
Python integers.  The dynamic program walks the events in a Python loop with one int64 row per event (a path's cost stays below
2^57).  Shares no code with the kernel and none with tests/signal_align_ref.py beyond the reading of labels and model rows."""
import numpy as np

from tests.signal_align_ref import BAD_READ, INF, NO_ALIGNMENT, model_rows_ok, read_states

Q_MAX = (1 << 23) - 1
MAX_EVENT_LEN = 65536
MAX_SIGNAL = 1 << 24
MAX_MOVE = 3


def event_cost(n, s1, q2, level, weight, offset, S, max_cost):
    """min((D weight) >> S, n max_cost) + n offset, D = Q - 2 level S1 + n level^2, in Python integers"""
    n, s1, q2, level = int(n), int(s1), int(q2), int(level)
    D = q2 - 2 * level * s1 + n * level * level
    return min((D * int(weight)) >> S, n * int(max_cost)) + n * int(offset)


def cost_row(n, s1, q2, level, weight, offset, S, max_cost):
    """event_cost of one event against object arrays of model rows (Python integers element by element): int64 array"""
    n, s1, q2 = int(n), int(s1), int(q2)
    D = q2 - 2 * s1 * level + n * (level * level)
    sh = (D * weight) >> S
    return (np.minimum(sh, n * int(max_cost)) + n * offset).astype(np.int64)


def event_ok(n, s1, q2):
    n, s1, q2 = int(n), int(s1), int(q2)
    return 1 <= n <= MAX_EVENT_LEN and abs(s1) <= n * Q_MAX and 0 <= q2 <= n * Q_MAX * Q_MAX and s1 * s1 <= n * q2


def band_lo(e, N, E, W):
    return min(max(((2 * e + 1) * N) // (2 * E) - W // 2, 0), max(N - W, 0))


def max_move_of(move_cost):
    return max(m for m in range(4) if move_cost[m] >= 0)


def align_read(events, codes, model, S, max_cost, move_cost, W):
    """events: E tuples (n, S1, Q); codes: the k-mer of each of the N states; W: the band, or None for no band.  Returns (score,
    states [E]) of the minimum-cost path inside the band, ties as the definition says, or (None, None) when there is none."""
    E, N = len(events), len(codes)
    if W is None:
        W = N
    rows = np.asarray(model, dtype=np.int64)[np.asarray(codes, dtype=np.int64)]
    level, weight, offset = (np.array([int(v) for v in rows[:, c]], dtype=object) for c in range(3))
    cost = np.full(N + MAX_MOVE, INF, dtype=np.int64)                # cost[3 + j]: state j at the previous event; cost[0..3) stays INF
    back = np.zeros((E, W), dtype=np.uint8)                          # back[e, j - lo(e)]: the move that state j at e came by
    plo = 0
    for e, (n, s1, q2) in enumerate(events):
        lo = band_lo(e, N, E, W)
        hi = min(lo + W, N)
        if e == 0:
            assert lo == 0
            new = np.full(hi, INF, dtype=np.int64)
            new[0] = 0
            took = np.zeros(hi, dtype=np.uint8)
        else:
            new = np.full(hi - lo, INF, dtype=np.int64)
            took = np.zeros(hi - lo, dtype=np.uint8)
            for m in range(MAX_MOVE + 1):                            # the stay first, each larger move only if strictly cheaper
                if move_cost[m] < 0:
                    continue
                prev = cost[MAX_MOVE + lo - m:MAX_MOVE + hi - m]     # outside the previous band it holds INF
                cand = np.where(prev < INF, prev + move_cost[m], INF)
                better = cand < new
                new = np.where(better, cand, new)
                took[better] = m
        live = new < INF
        if live.any():
            new = np.where(live, new + cost_row(n, s1, q2, level[lo:hi], weight[lo:hi], offset[lo:hi], S, max_cost), INF)
        cost[MAX_MOVE + plo:MAX_MOVE + lo] = INF                     # the states that left the band
        cost[MAX_MOVE + lo:MAX_MOVE + hi] = new
        back[e, :hi - lo] = took
        plo = lo
    score = int(cost[MAX_MOVE + N - 1])
    if score >= INF:
        return None, None
    states = np.empty(E, dtype=np.int32)
    s = N - 1
    for e in range(E - 1, -1, -1):
        states[e] = s
        s -= int(back[e, s - band_lo(e, N, E, W)])
    assert s == 0 and states[0] == 0
    return score, states


def band_hits_of(states, N, W):
    E = len(states)
    hits = 0
    for e, s in enumerate(states.tolist()):
        lo = band_lo(e, N, E, W)
        if (s == lo and lo > 0) or (s == lo + W - 1 and lo + W < N):
            hits += 1
    return hits


def starts_of(states, ev_starts, N, max_states):
    """starts[j] = the first sample of the first event at or beyond state j (a skipped state begins where its successor does)"""
    E = len(states)
    T = int(ev_starts[E])
    starts = np.full(max_states + 1, T, dtype=np.int32)
    j = 0
    for e, s in enumerate(states.tolist()):
        while j <= s:
            starts[j] = ev_starts[e]
            j += 1
    assert j == N
    return starts


def move_counts_of(states):
    return np.bincount(np.diff(np.asarray(states, dtype=np.int64)), minlength=4).astype(np.int32)


def event_align_ref(n_events, ev_starts, ev_sum, ev_sumsq, labels, label_lengths, model, move_cost, k=5, first=0, weight_shift=32,
                    max_cost=None, band=512, max_states=None):
    """What wn_event_align writes: a dict of starts [B, max_states + 1] int32, score [B] object (Python integers), band_hits [B]
    int32, moves [B, 4] int32, states [B, max_events] int32 and bad (the count).  band=None: no band."""
    B, M = len(n_events), ev_starts.shape[1] - 1
    n_lab = labels.shape[1]
    model = np.asarray(model, dtype=np.int64)
    max_cost = (1 << 31) - 1 if max_cost is None else int(max_cost)
    if max_states is None:
        max_states = max(n_lab - (k - 1) - 2 * first, 1)
    top_move = max_move_of(move_cost)
    starts = np.full((B, max_states + 1), -1, dtype=np.int32)
    states = np.full((B, M), -1, dtype=np.int32)
    moves = np.full((B, 4), -1, dtype=np.int32)
    score, hits, bad = [BAD_READ] * B, np.full(B, -1, dtype=np.int32), 0
    for b in range(B):
        E, ll = int(n_events[b]), int(label_lengths[b])
        N = ll - (k - 1) - 2 * first
        if not (0 <= E <= M and 0 <= ll <= n_lab and N <= max_states):
            bad += 1
            continue
        if E < 1 or N < 1 or N - 1 > top_move * (E - 1):
            score[b], hits[b], moves[b] = NO_ALIGNMENT, 0, 0
            continue
        codes = read_states(labels[b], ll, k, first)
        es = [int(v) for v in ev_starts[b, :E + 1]]
        events = [(es[e + 1] - es[e], int(ev_sum[b, e]), int(ev_sumsq[b, e])) for e in range(E)]
        if codes is None or not model_rows_ok(model, codes) or es[0] < 0 or es[E] > MAX_SIGNAL or not all(event_ok(*ev) for ev in events):
            bad += 1
            continue
        sc, st = align_read(events, codes, model, weight_shift, max_cost, move_cost, band)
        if sc is None:
            score[b], hits[b], moves[b] = NO_ALIGNMENT, 0, 0
            continue
        score[b] = sc
        hits[b] = 0 if band is None else band_hits_of(st, N, band)
        states[b, :E] = st
        moves[b] = move_counts_of(st)
        starts[b] = starts_of(st, es, N, max_states)
    return {"starts": starts, "score": np.array(score, dtype=object), "band_hits": hits, "moves": moves, "states": states, "bad": bad}


def rescore(events, codes, model, S, max_cost, move_cost, states):
    """the cost of ANY assignment of a state to every event, in Python integers; None if it uses a forbidden move"""
    model = np.asarray(model, dtype=np.int64)
    total = 0
    for e, (ev, s) in enumerate(zip(events, states)):
        level, weight, offset = (int(v) for v in model[codes[int(s)]])
        total += event_cost(ev[0], ev[1], ev[2], level, weight, offset, S, max_cost)
        if e:
            m = int(s) - int(states[e - 1])
            if not 0 <= m <= MAX_MOVE or move_cost[m] < 0:
                return None
            total += move_cost[m]
    return total


def events_of(q, ev_starts):
    """the (n, S1, Q) rows of quantised samples q cut at ev_starts, in Python integers"""
    out = []
    for s0, s1 in zip(ev_starts[:-1], ev_starts[1:]):
        seg = [int(v) for v in q[int(s0):int(s1)]]
        out.append((len(seg), sum(seg), sum(v * v for v in seg)))
    return out
