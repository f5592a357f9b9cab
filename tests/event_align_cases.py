"""Inputs of the event_align tests, built once (seeded numpy), with their references from tests/event_align_ref.py cached per case.
A case is a batch of event tables (n_events, ev_starts, ev_sum, ev_sumsq -- what wn_event_detect writes) beside the labels they
are aligned to.  Reads are drawn from the integer pore model of tests/signal_align_cases.py (random bases, a dwell per k-mer,
every sample its k-mer's level plus Gaussian noise, quantised at F = 12); their event boundaries are the true k-mer boundaries
with some DROPPED (a missed boundary: the next event skips) and some ADDED inside a dwell (a spurious one: the next event stays),
by a rule per case, so that each case reaches the shape it is for whatever a detector would do.  tests/test_event_align_ref.py
holds the reference to things it shares no code with; tests/test_gpu_event_align.py runs the cases on the device."""
import collections
import functools

import numpy as np

from tests import event_align_ref as R
from tests import signal_align_cases as SC
from tests.signal_align_ref import read_states

Case = collections.namedtuple("Case", "n_events ev_starts ev_sum ev_sumsq labels label_lengths model kw truth")
F, S, COST_BITS = SC.F, SC.S, SC.COST_BITS
EVENT_TILE = 256                        # csrc/wn_eventalign.hip: kEaTile, the events staged into LDS at a time
QMAX = (1 << 23) - 1
MOVES = (503, 122, 412, 824)            # round(-ln p 2^8) of (0.14, 0.62, 0.20, 0.04)
ALL_FREE = (0, 0, 0, 0)


def kw_of(k=5, first=0, band=64, moves=MOVES, weight_shift=S, max_cost=None):
    return dict(k=k, first=first, band=band, move_cost=tuple(moves), weight_shift=weight_shift, max_cost=max_cost)


def pack(reads, labels, label_lengths, model, kw, pad=2, truth=None, max_events=None):
    """reads: per read (ev_starts list of E + 1 entries, [(n, S1, Q)] * E).  Rows past a read's events: starts T_b, sums 0"""
    B = len(reads)
    M = (max(max(len(ev) for _, ev in reads), 1) + pad) if max_events is None else max_events
    n_events = np.array([len(ev) for _, ev in reads], dtype=np.int32)
    ev_starts = np.zeros((B, M + 1), dtype=np.int32)
    ev_sum, ev_sumsq = np.zeros((B, M), dtype=np.int64), np.zeros((B, M), dtype=np.int64)
    for b, (st, ev) in enumerate(reads):
        ev_starts[b, :len(st)] = st
        ev_starts[b, len(st):] = st[-1]
        for e, (_, s1, q2) in enumerate(ev):
            ev_sum[b, e], ev_sumsq[b, e] = s1, q2
    return Case(n_events, ev_starts, ev_sum, ev_sumsq, np.asarray(labels, dtype=np.int32), np.asarray(label_lengths, dtype=np.int32),
                np.asarray(model, dtype=np.int64), kw, truth)


def quantised_read(rng, codes, dwells, means, stdvs):
    which = np.repeat(np.asarray(codes, dtype=np.int64), dwells)
    x = (means[which] + stdvs[which] * rng.standard_normal(len(which))).astype(np.float32)
    return np.rint(x.astype(np.float64) * 2.0 ** F).astype(np.int64)


def cut(rng, dwells, drop, split, run=2):
    """event boundaries from the true ones: each true boundary is dropped with probability `drop` (never more than `run` in a row,
    so that no event spans more than run + 1 states), each dwell of two samples or more gets a spurious boundary with probability
    `split`, and with that probability again a second and a third.  Returns ev_starts"""
    edges = np.concatenate([[0], np.cumsum(dwells)])
    keep, dropped = [0], 0
    for j in range(1, len(dwells)):
        if dropped < run and rng.random() < drop:
            dropped += 1
        else:
            keep.append(int(edges[j]))
            dropped = 0
    for j, n in enumerate(dwells):
        reps = 0
        while n >= 2 + reps and rng.random() < split and reps < 3:
            keep.append(int(edges[j]) + 1 + int(rng.integers(0, n - 1)))
            reps += 1
    return sorted(set(keep)) + [int(edges[-1])]


def build(seed, n_states, k=5, first=0, band=64, drop=0.28, split=0.14, run=2, dwell=(3, 12), moves=MOVES, labels=None, pad=2, **more):
    """n_states: the states of each read.  Returns the Case; truth holds per read (q, ev_starts, dwell edges)"""
    rng = np.random.default_rng(seed)
    means, stdvs, tab = SC.table(k)
    B = len(n_states)
    ll = np.array([n + (k - 1) + 2 * first for n in n_states], dtype=np.int32)
    if labels is None:
        labels = rng.integers(1, 5, size=(B, int(ll.max()) + 1)).astype(np.int32)
    reads, truth = [], []
    for b, n in enumerate(n_states):
        codes = read_states(labels[b], int(ll[b]), k, first)
        dwells = rng.integers(dwell[0], dwell[1], size=n)
        q = quantised_read(rng, codes, dwells, means, stdvs)
        st = cut(rng, dwells, drop, split, run)
        reads.append((st, R.events_of(q, st)))
        truth.append((q, st, np.concatenate([[0], np.cumsum(dwells)])))
    return pack(reads, labels, ll, tab, kw_of(k=k, first=first, band=band, moves=moves, **more), pad=pad, truth=truth)


def exact_events(seed, E, N, k=5, first=0, band=64, moves=MOVES, **more):
    """a read of exactly E events over N states, N - 1 <= 3 (E - 1) + 1: the N - 1 state advances are spread over the E - 1 event
    boundaries as evenly as they go (each 0..3, the surplus one on the last boundary if N - 1 = 3 (E - 1) + 1, where no alignment
    exists); an event covers the states it advances over, 4 samples each, and a stay repeats its state"""
    rng = np.random.default_rng(seed)
    means, stdvs, tab = SC.table(k)
    ll = N + (k - 1) + 2 * first
    labels = rng.integers(1, 5, size=(1, ll + 1)).astype(np.int32)
    codes = read_states(labels[0], ll, k, first)
    adv = [((e + 1) * (N - 1)) // (E - 1) - (e * (N - 1)) // (E - 1) for e in range(E - 1)] if E > 1 else []
    if E == 1:
        per_event = [list(range(N))]
    else:
        per_event = [[0]]
        at = 0
        for a in adv:
            per_event.append(list(range(at + 1, at + a + 1)) if a else [at])
            at += a
    st, which = [0], []
    for states in per_event:
        for s in states:
            which += [codes[s]] * 4
        st.append(len(which))
    which = np.asarray(which, dtype=np.int64)
    x = (means[which] + stdvs[which] * rng.standard_normal(len(which))).astype(np.float32)
    q = np.rint(x.astype(np.float64) * 2.0 ** F).astype(np.int64)
    return pack([(st, R.events_of(q, st))], labels, [ll], tab, kw_of(k=k, first=first, band=band, moves=moves, **more))


# ---- the case worked by hand (tests/test_event_align_ref.py): k = 1, F = 0, a sample costs d^2
HAND_MODEL = SC.HAND_MODEL
HAND_KW = kw_of(k=1, first=0, band=64, moves=(3, 1, 2, 40), weight_shift=16)


def hand_case():
    """levels 10, 20, 30, 40 for the bases 1..4; labels 1 2 3 4; three events: (10, 10), (20, 30: one missed boundary), (40)"""
    q = [10, 10, 20, 30, 40]
    st = [0, 2, 4, 5]
    return pack([(st, R.events_of(q, st))], [[1, 2, 3, 4]], [4], HAND_MODEL, HAND_KW)


def homopolymer_case():
    """constant events over one repeated base: every path costs its moves only, and with all moves free every path ties"""
    reads = []
    for E in (30, 10, 4):
        st = list(range(0, 3 * E + 1, 3))
        reads.append((st, R.events_of([20] * (3 * E), st)))
    return pack(reads, np.full((3, 10), 2), [10, 10, 10], HAND_MODEL, dict(HAND_KW, move_cost=ALL_FREE))


def limit_case():
    """the numeric limits of an event: n = 65536 samples of +-(2^23 - 1) against the level of the other sign (D just under 2^64),
    weight 2^31 - 1; one read per S in {16, 32, 63} and max_cost on both sides of the quotient"""
    model = np.array([[-QMAX, (1 << 31) - 1, (1 << 30) - 1], [QMAX, (1 << 31) - 1, -(1 << 30) + 1], [0, 1, 0], [5, 1 << 16, 0]], dtype=np.int64)
    n = 65536
    reads, labels = [], []
    for lab, sign in (([1, 2, 3], 1), ([2, 1, 4], -1)):
        ev = [(n, sign * n * QMAX, n * QMAX * QMAX), (n, -sign * n * QMAX, n * QMAX * QMAX), (3, 15, 77)]
        reads.append(([0, n, 2 * n, 2 * n + 3], ev))
        labels.append(lab)
    return [pack(reads, labels, [3, 3], model, kw_of(k=1, band=64, moves=(7, 0, 5, 9), weight_shift=s, max_cost=mc))
            for s, mc in ((16, None), (32, None), (63, None), (16, 1), (32, 4095), (63, 4194302), (63, 4194303), (63, 4194304))]


def pressed_case(band):
    """400 constant events over 200 states of one repeated base, a free stay and a step at 1: every path without a skip costs 199,
    and the tie rule (the stay first) makes the traced path reach every state as EARLY as the band lets it -- along the band's
    upper edge once the diagonal j = e has left the band"""
    E, N = 400, 200
    st = list(range(0, 2 * E + 1, 2))
    return pack([(st, R.events_of([20] * (2 * E), st))], np.full((1, N), 2), [N], HAND_MODEL, dict(HAND_KW, band=band, move_cost=(0, 1, 5, 9)))


BAD_READS = ("good", "events_above", "events_negative", "label_length_above", "label_length_negative", "states_above", "label_0", "label_5",
             "good_labels_outside_the_window", "n_0", "n_65537", "starts_decrease", "sum_above", "sumsq_negative", "sum_squared_above",
             "weight_0", "start_negative", "good_garbage_past_the_events", "good_last")
BAD_GOOD = {n for n in BAD_READS if n.startswith("good")}
BAD_K, BAD_FIRST = 5, 2


@functools.lru_cache(maxsize=None)
def bad_batch():
    """every fault once, between good reads: 30 states, k = 5, first = 2"""
    case = build(22, [30] * len(BAD_READS), k=BAD_K, first=BAD_FIRST, pad=4)
    ne, es, s1, q2 = case.n_events.copy(), case.ev_starts.copy(), case.ev_sum.copy(), case.ev_sumsq.copy()
    labels, ll, model = case.labels.copy(), case.label_lengths.copy(), case.model.copy()
    r = BAD_READS.index
    M = es.shape[1] - 1
    ne[r("events_above")], ne[r("events_negative")] = M + 1, -1
    ll[r("label_length_above")], ll[r("label_length_negative")] = labels.shape[1] + 1, -1
    ll[r("states_above")] = labels.shape[1]                          # one label more than the others: 31 states
    labels[r("label_0"), BAD_FIRST] = 0                              # the first label of the window
    labels[r("label_5"), ll[r("label_5")] - BAD_FIRST - 1] = 5       # the last one
    b = r("good_labels_outside_the_window")
    labels[b, BAD_FIRST - 1], labels[b, ll[b] - BAD_FIRST] = 0, 7
    b = r("n_0")
    es[b, 4] = es[b, 3]
    s1[b, 3] = q2[b, 3] = 0
    b = r("n_65537")
    es[b, 6:] += 65537 - (es[b, 6] - es[b, 5])
    b = r("starts_decrease")
    es[b, 5] = es[b, 4] - 1
    b, e = r("sum_above"), 2
    n = int(es[b, e + 1] - es[b, e])
    s1[b, e], q2[b, e] = n * QMAX + 1, n * QMAX * QMAX
    q2[r("sumsq_negative"), 0] = -1
    b, e = r("sum_squared_above"), ne[r("sum_squared_above")] - 1     # the last event: S^2 = n Q + 1
    n = int(es[b, e + 1] - es[b, e])
    s1[b, e], q2[b, e] = 2 * n + 1, (4 * n * n + 4 * n) // n         # (2 n + 1)^2 = n (4 n + 4) + 1
    es[r("start_negative"), 0] = -1
    b = r("good_garbage_past_the_events")
    s1[b, ne[b]:], q2[b, ne[b]:] = -(1 << 62), -5
    own = set(read_states(labels[r("weight_0")], int(ll[r("weight_0")]), BAD_K, BAD_FIRST))
    for b, name in enumerate(BAD_READS):
        if name in BAD_GOOD:
            own -= set(read_states(labels[b], int(case.label_lengths[b]), BAD_K, BAD_FIRST))
    model[min(own), 1] = 0                                            # a k-mer only the faulty read uses
    return Case(ne, es, s1, q2, labels, ll, model, case.kw, None), 30  # max_states: one below the 31 of `states_above`


def _cases():
    c = {"hand": hand_case(), "homopolymer": homopolymer_case()}
    c["noisy"] = build(1, [150, 160, 151, 175], k=5, first=2)        # fewer events than states, as a detector leaves them
    c["one_event"] = exact_events(2, 1, 1)
    c["one_state"] = exact_events(3, 40, 1)                          # all stays
    c["all_double_skips"] = exact_events(4, 50, 3 * 49 + 1)
    c["one_state_too_many"] = exact_events(5, 50, 3 * 49 + 2)        # no alignment
    for E in (EVENT_TILE - 1, EVENT_TILE, EVENT_TILE + 1, 2 * EVENT_TILE):
        c["tile_%d" % E] = exact_events(6 + E, E, (E * 11) // 10)
    c["every_slot_reused"] = build(7, [300], drop=0.05, split=0.38, band=64)      # N = 300, E = 442
    c["three_rearm"] = exact_events(8, 210, 610, band=64)            # N = 2.9 E, N > W
    for W in (64, 512, 576, 2048):
        c["threads_w%d" % W] = build(9, [2200], drop=0.6, split=0.02, band=W, dwell=(2, 5))
    c["pressed_w64"], c["pressed_w2048"] = pressed_case(64), pressed_case(2048)
    # without the stay a read needs E <= N, without skips E >= N: more boundaries dropped than added, and the other way round
    for name, mv, drop, split in (("no_stay", (-1, 122, 412, 824), 0.3, 0.05), ("no_skip", (503, 122, -1, -1), 0.02, 0.4),
                                  ("no_double_skip", (503, 122, 412, -1), 0.2, 0.2), ("no_single_skip", (503, 122, -1, 824), 0.2, 0.2)):
        c["forbid_" + name] = build(11, [120, 90], moves=mv, drop=drop, split=split)
    for i, lim in enumerate(limit_case()):
        c["limit_%d" % i] = lim
    for k, first in ((1, 0), (1, 2), (5, 0), (5, 2), (6, 0), (6, 2)):
        c["form_k%d_first%d" % (k, first)] = build(20 + 3 * k + first, [100, 37, 64], k=k, first=first)
    return c


CASES = _cases()


def call_ref(case, band="kw", max_states=None):
    kw = dict(case.kw)
    if band != "kw":
        kw["band"] = band
    return R.event_align_ref(case.n_events, case.ev_starts, case.ev_sum, case.ev_sumsq, case.labels, case.label_lengths, case.model,
                             max_states=max_states, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    return call_ref(CASES[name])


@functools.lru_cache(maxsize=None)
def bad_reference():
    case, max_states = bad_batch()
    return call_ref(case, max_states=max_states)


# ---- the gap this tool closes (tests/test_event_align_ref.py, case 6; the GPU composition): noisy reads whose detected events are
# fewer than their k-mers.  k = 3, a table of pairwise distinct levels, gamma dwells of mean 10 (shape 4, as the timing reads of
# DESIGN.md section 7k; at shape 2 a sixth of the dwells are below the detector's short window and runs of four missed boundaries,
# which no path of moves <= 3 follows, occur in most reads of 150 states), Gaussian noise.  Seed and sigma were picked on the CPU
GAP_K, GAP_SEED, GAP_SIGMA, GAP_READS, GAP_STATES, GAP_SHAPE = 3, 3, 1.5, 8, 150, 4.0


@functools.lru_cache(maxsize=None)
def gap_reads(sigma=GAP_SIGMA, seed=GAP_SEED):
    """dict: signal [B, L] float32 (noisy), clean [B, L] float32 (the same reads without noise), signal_lengths, labels, label_lengths,
    means, stdvs, edges (per read the true first sample of every state, and T)"""
    rng = np.random.default_rng(seed)
    means = 60.0 + 0.75 * rng.permutation(4 ** GAP_K)                # steps of 0.75 at the least, quarter units: exact
    stdvs = np.full(4 ** GAP_K, max(sigma, 0.25))
    B, n = GAP_READS, GAP_STATES
    ll = np.full(B, n + GAP_K - 1, dtype=np.int32)
    labels = rng.integers(1, 5, size=(B, n + GAP_K - 1)).astype(np.int32)
    for b in range(B):
        for i in range(GAP_K, labels.shape[1]):                      # no base four times in a row: consecutive 3-mers differ
            if (labels[b, i - GAP_K:i] == labels[b, i]).all():
                labels[b, i] = labels[b, i] % 4 + 1
    rows, edges = [], []
    for b in range(B):
        codes = read_states(labels[b], int(ll[b]), GAP_K, 0)
        dwells = np.maximum(rng.gamma(GAP_SHAPE, 10.0 / GAP_SHAPE, size=n).astype(np.int64), 1)
        clean = np.repeat(means[codes], dwells)
        rows.append((clean, clean + sigma * rng.standard_normal(len(clean))))
        edges.append(np.concatenate([[0], np.cumsum(dwells)]))
    L = max(len(c) for c, _ in rows) + 3
    signal, clean = np.zeros((B, L), dtype=np.float32), np.zeros((B, L), dtype=np.float32)
    for b, (c, x) in enumerate(rows):
        clean[b, :len(c)], signal[b, :len(x)] = c, x
    return dict(signal=signal, clean=clean, signal_lengths=np.array([len(c) for c, _ in rows], dtype=np.int32), labels=labels,
                label_lengths=ll, means=means, stdvs=stdvs, edges=edges)


def gap_model(fx):
    """the integer table of the gap reads' Gaussian model at F = 12, S = 40, as tests/signal_align_cases.table writes it"""
    model = np.empty((4 ** GAP_K, 3), dtype=np.int64)
    model[:, 0] = np.rint(fx["means"] * 2.0 ** F)
    model[:, 1] = np.rint(2.0 ** (S + COST_BITS) / (2.0 * (fx["stdvs"] * 2.0 ** F) ** 2))
    model[:, 2] = np.rint(2.0 ** COST_BITS * np.log(fx["stdvs"] * 2.0 ** F))
    return model
