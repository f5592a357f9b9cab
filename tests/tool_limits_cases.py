"""Inputs that hold event detection (csrc/wn_eventdetect.hip), event alignment (csrc/wn_eventalign.hip), demultiplexing
(csrc/wn_demux.hip) and read mapping (csrc/wn_readmap.hip) at the window, halo and size limits their kernels state, each built once
from fixed seeds with numpy only; the references are those of tests/event_detect_ref.py, tests/event_align_ref.py, tests/demux_ref.py
and tests/readmap_ref.py.  tests/test_tool_limits_ref.py asserts on the CPU, from the references alone, that every case reaches what
it exists for; tests/test_gpu_tool_limits.py runs them on the device.  Where a seed was searched for, it was
searched on the CPU against the reference, and the condition it was searched for is asserted in tests/test_tool_limits_ref.py."""
import functools

import numpy as np

from tests import demux_cases as DC
from tests import demux_ref as DR
from tests import event_align_cases as EA
from tests import event_align_ref as EAR
from tests import event_detect_cases as ED
from tests import readmap_cases as RC
from tests import readmap_ref as RR
from tests import signal_align_cases as SC
from tests.signal_align_ref import read_states

QMAX = (1 << 23) - 1

# ================================================================================================================ event alignment
TRACE, WIN_BYTES, MAX_MOVE = 64, 49, 3          # csrc/wn_eventalign.hip: kEaTrace, kEaWinBytes, kEaMaxMove


def event_trace_windows(states):
    """the index arithmetic of the kernel's trace loop over a reference path (the state of every event): per chunk of 64 events,
    last chunk first, (e0, nf, g0, lowest byte, highest byte, s_end & 3) with g0 = max(s_end - 191, 0) >> 2 the first backpointer
    byte of the window and (s >> 2) - g0 the byte read for an event in state s; the window holds the bytes 0..48"""
    states = [int(s) for s in states]
    E = len(states)
    out = []
    for e0 in range((E - 1) // TRACE * TRACE, -1, -TRACE):
        nf = min(TRACE, E - e0)
        s_end = states[e0 + nf - 1]
        g0 = max(s_end - (MAX_MOVE * TRACE - 1), 0) >> 2
        rel = [(s >> 2) - g0 for s in states[e0:e0 + nf]]
        out.append((e0, nf, g0, min(rel), max(rel), s_end & 3))
    return out


def moved_read(seed, adv, k=5):
    """a read as tests/event_align_cases.exact_events builds it (4 samples per state), with the E - 1 state advances given one by
    one: an event covers the states it advances over, and a stay repeats its state.  Returns (ev_starts, events, labels, ll)"""
    rng = np.random.default_rng(seed)
    means, stdvs, _ = SC.table(k)
    N = 1 + sum(adv)
    ll = N + (k - 1)
    labels = rng.integers(1, 5, size=ll + 1).astype(np.int32)
    codes = read_states(labels, ll, k, 0)
    per_event, at = [[0]], 0
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
    q = np.rint(x.astype(np.float64) * 2.0 ** EA.F).astype(np.int64)
    return st, EAR.events_of(q, st), labels, ll


def batch_of_reads(reads, band, k=5, pad=2):
    """reads: (ev_starts, events, labels, ll) each, under the table of tests/signal_align_cases.table(k)"""
    width = max(len(r[2]) for r in reads)
    labels = np.ones((len(reads), width), dtype=np.int32)
    for b, r in enumerate(reads):
        labels[b, :len(r[2])] = r[2]
    return EA.pack([(r[0], r[1]) for r in reads], labels, [r[3] for r in reads], SC.table(k)[2], EA.kw_of(k=k, band=band), pad=pad)


STEEP_E = (65, 66, 67, 68, 129, 193)
STEEP_BANDS = (64, 2048)
STEEP_D = (0, 1, 2, 3)
# the seed of the read (E, d): the first of 100 E + d, + 1000, + 2000, ... whose reference path is the planted one (a second path
# through the d leading events, such as the moves 1, 3 in place of 2, 2, costs about the same before the noise is drawn)
STEEP_SEED_STEP = 1000
STEEP_TRIES = {(65, 3, 2): 1, (66, 2, 2): 2, (67, 3, 2): 2, (68, 2, 2): 1, (129, 3, 2): 1, (193, 3, 2): 1, (129, 1, 0): 1, (129, 2, 0): 108,
               (129, 3, 0): 36}


def steep_adv(E, d, lead=2):
    return [lead] * d + [3] * (E - 1 - d)


def steep_seed(E, d, lead=2):
    return 100 * E + d + (50 if lead == 0 else 0) + STEEP_SEED_STEP * STEEP_TRIES.get((E, d, lead), 0)


@functools.lru_cache(maxsize=None)
def steep_read(E, d, lead=2):
    return moved_read(steep_seed(E, d, lead), steep_adv(E, d, lead))


@functools.lru_cache(maxsize=None)
def event_align_case(name):
    """steep_E<E>_w<band>: the four reads d = 0..3 of E events, d leading moves of 2 and moves of 3 after them; stays_w<band>: E =
    129 with d = 1..3 stays in front instead; mixed_w<band>: steep reads of several E beside a short noisy one; largest_low_moves
    and largest_top_moves: events of 65536 samples at the largest costs, T_b = 2^24, and a read that ends at 2^24 + 1"""
    kind, _, band = name.rpartition("_w")
    if kind.startswith("steep_E"):
        return batch_of_reads([steep_read(int(kind[7:]), d) for d in STEEP_D], int(band))
    if kind == "stays":
        return batch_of_reads([steep_read(129, d, 0) for d in (1, 2, 3)], int(band))
    if kind == "mixed":
        noisy = EA.build(77, [40], k=5, first=0)
        short = (noisy.ev_starts[0, :noisy.n_events[0] + 1].tolist(),
                 [(int(noisy.ev_starts[0, e + 1] - noisy.ev_starts[0, e]), int(noisy.ev_sum[0, e]), int(noisy.ev_sumsq[0, e]))
                  for e in range(int(noisy.n_events[0]))], noisy.labels[0], int(noisy.label_lengths[0]))
        return batch_of_reads([steep_read(129, 1), short, steep_read(68, 2), steep_read(193, 3), steep_read(129, 2, 0), steep_read(65, 0)], int(band))
    return largest_case(name)


LARGEST_E, LARGEST_N = 256, 65536
LARGEST_MOVES = {"largest_low_moves": (7, 0, 5, 9), "largest_top_moves": ((1 << 30) - 1,) * 4}
LARGEST_READS = ("dearest", "cheapest", "plain", "one_sample_too_many")


def largest_case(name):
    """E = N = 256 events of n = 65536 samples: T_b = 2^24 exactly, under the model rows of tests/event_align_cases.limit_case.
    `dearest`: every sample at 2^23 - 1 against the level -(2^23 - 1) at weight 2^31 - 1, clamped to 2^31 - 1 a sample, offset
    2^30 - 1; `cheapest`: every sample on its level, offset -(2^30 - 1); `plain`: samples of 6 against the level 5 at weight 2^16;
    `one_sample_too_many`: the dearest read with a 257th event of one sample, which ends at 2^24 + 1 -- a bad read"""
    model = EA.limit_case()[0].model
    n, E = LARGEST_N, LARGEST_E
    st = list(range(0, n * E + 1, n))
    top = [(n, n * QMAX, n * QMAX * QMAX)] * E
    reads = [(st, top), (st, top), (st, [(n, 6 * n, 36 * n)] * E), (st + [n * E + 1], top + [(1, QMAX, QMAX * QMAX)])]
    labels = [[1] * E, [2] * E, [4] * E, [1] * E]
    return EA.pack(reads, labels, [E] * 4, model, EA.kw_of(k=1, band=64, moves=LARGEST_MOVES[name], weight_shift=16), pad=0)


EVENT_ALIGN = (["steep_E%d_w%d" % (E, W) for W in STEEP_BANDS for E in STEEP_E] + ["stays_w%d" % W for W in STEEP_BANDS] +
               ["mixed_w%d" % W for W in STEEP_BANDS] + list(LARGEST_MOVES))


@functools.lru_cache(maxsize=None)
def event_align_reference(name):
    return EA.call_ref(event_align_case(name))


def planted_moves(name):
    """[stays, steps, skips, double skips] of every read of a steep case, as planted; None for a read that is not steep"""
    kind, _, band = name.rpartition("_w")
    if kind.startswith("steep_E"):
        E = int(kind[7:])
        return [[0, 0, d, E - 1 - d] for d in STEEP_D]
    if kind == "stays":
        return [[d, 0, 0, 128 - d] for d in (1, 2, 3)]
    if kind == "mixed":
        return [[0, 0, 1, 127], None, [0, 0, 2, 65], [0, 0, 3, 189], [2, 0, 0, 126], [0, 0, 0, 64]]
    return None


# ================================================================================================================ event detection
# w_0 = w_1 = 16 and r_0 = 64.  Whether i is a boundary depends, through the merge rule, on the short peaks of [i - 16, i + 16];
# whether s is a short peak on the short scores of [s - 64, s + 64]; the score of j on the samples [j - 16, j + 16).  So the samples
# that can decide position i are [i - 96, i + 95]: the reach is 96 to the left and 95 to the right, and the kernel's halo of 96
# samples a side covers both.
REACH_KW = dict(ED.HAND_KW, windows=(16, 16), thresholds=(6.0, 3.0), radii=(64, 2), min_var=4.0)
REACH_LEFT, REACH_RIGHT = 96, 95
REACH_T = 1700
REACH_SEAMS = (256, 768, 1536)
REACH_CHUNKS = (256, None, 1024, 16384)


def reach_read(side, i, bump=None):
    """right: a step of +2 at i (a long peak, below the short threshold) and steps of -10 at i + 16 and i + 80, whose short scores
    tie: the earlier one is the short peak and merges the long peak at i away.  One less on sample i + 95, the last of the window
    of i + 80, breaks the tie the other way: i + 16 is no short peak any more and i is a boundary.
    left: steps of +10 at i - 80 and i - 16 and a step of -2 at i: i - 80 wins the tie, i - 16 is no short peak and i is a boundary.
    One more on sample i - 96, the first of the window of i - 80, lowers that step: i - 16 is the short peak and i is merged away.
    The small step goes against the large ones, so that the windows which hold both score less than the one at i: with steps of
    one sign the long peak sits at i + 1 (right) or i - 1 (left) and the deciding sample only 94 or 95 away from it"""
    x = np.full(REACH_T, 40.0)
    if side == "right":
        x[i:], x[i + 16:], x[i + 80:] = 42.0, 32.0, 22.0
    else:
        x[i - 80:], x[i - 16:], x[i:] = 50.0, 60.0, 58.0
    if bump is not None:
        x[bump] += -1.0 if side == "right" else 1.0
    return x


def reach_pairs():
    """[(side, seam, i, deciding sample, the sample one beyond it)]: the decided position on the last position before each seam
    and on the first after it"""
    out = []
    for seam in REACH_SEAMS:
        for i in (seam - 1, seam):
            out.append(("right", seam, i, i + REACH_RIGHT, i + REACH_RIGHT + 1))
            out.append(("left", seam, i, i - REACH_LEFT, i - REACH_LEFT - 1))
    return out


@functools.lru_cache(maxsize=None)
def reach_case():
    """three reads a pair: 3 p the plain read, 3 p + 1 the one altered at the reach, 3 p + 2 the one altered one sample beyond it"""
    reads = []
    for side, _, i, at, beyond in reach_pairs():
        reads += [reach_read(side, i), reach_read(side, i, at), reach_read(side, i, beyond)]
    return ED.batch_of(reads, dict(REACH_KW))


@functools.lru_cache(maxsize=None)
def reach_reference():
    return ED.call_ref(reach_case())


REACH_INT16_PAIRS = (4, 7)              # of reach_pairs(): to the right of position 767 and to the left of 768


@functools.lru_cache(maxsize=None)
def reach_int16():
    """(Case, raw int16, scale_shift, reference) of two pairs in the int16 form: v = raw / 2 + 3 is the integer it was"""
    case = reach_case()
    rows = [3 * p + u for p in REACH_INT16_PAIRS for u in range(3)]
    sub = ED.Case(case.signal[rows], case.signal_lengths[rows], case.kw, None)
    raw = np.rint((sub.signal.astype(np.float64) - 3.0) * 2.0).astype(np.int16)
    ss = np.tile(np.array([[0.5, 3.0]], dtype=np.float32), (len(rows), 1))
    return sub, raw, ss, ED.call_ref(sub, signal=raw, scale_shift=ss), rows


SUMS_EVENTS = 66                        # whole events before the last one: more than the 64 a wave takes


def sums_case(M):
    """constant reads of +-(2^23 - 1) under max_event_len = M in {32, 33}: 66 forced events of M samples (a lane sums an event of
    32, the wave one of 33) and a last event of 1, 31, 32 or 33 samples"""
    lasts = [n for n in (1, 31, 32, 33) if n <= M]
    reads = [np.full(SUMS_EVENTS * M + last, float(sign * QMAX)) for sign in (1, -1) for last in lasts]
    return ED.batch_of(reads, dict(ED.HAND_KW, windows=(3, 0), max_event_len=M), pad=0), lasts


@functools.lru_cache(maxsize=None)
def sums_reference(M):
    return ED.call_ref(sums_case(M)[0])


# =================================================================================================================== read mapping
K16_SEED, K16_REF, K16_READS, K16_LEN, K16_ERRORS = 6, 3000, 8, 300, 0.04
K16_W = (1, 10)


@functools.lru_cache(maxsize=None)
def k16():
    """a seeded 3000-base reference and 8 reads of 300 bases with 4 % errors, odd reads on the reverse strand: at k = 16 a quarter
    of the canonical codes have bit 31 set"""
    rng = np.random.default_rng(K16_SEED)
    ref = RC.random_bases(rng, K16_REF)
    reads = []
    for b in range(K16_READS):
        start = int(rng.integers(0, K16_REF - K16_LEN + 1))
        seq = RC.mutate(rng, ref[start:start + K16_LEN], K16_ERRORS)
        reads.append(RR.revcomp(seq) if b & 1 else seq)
    return ref, reads


@functools.lru_cache(maxsize=None)
def k16_index(w):
    return RR.index_ref(k16()[0], 16, w)


@functools.lru_cache(maxsize=None)
def k16_results(w):
    return [RR.map_read_ref(read, k16_index(w), k=16, w=w) for read in k16()[1]]


# ---- the longest read and max_occ = 64: k = 1, w = 1, so every base is a minimizer; A and T share the canonical code 0, C and G 1
OCC_CAPS = (32768, 1000)
OCC_REF_KEPT, OCC_REF_DROPPED = 64, 65
OCC_H = {32768: 1024, 1000: 64}         # chain_anchors' h on those rows; 32768 dense anchors: ~250 share a reference position


@functools.lru_cache(maxsize=None)
def occ():
    """the reference: 64 bases A / T (the code 0 has exactly max_occ entries) and 65 bases C / G (65: dropped whole).  The reads:
    `dense` 65535 bases A / T -- 64 hits at every position, 65535 * 64 anchors, the most a read can have; `sparse` 65535 bases C / G
    but for 300 A / T, the first and the last base among them -- all kept at 32768, so that among its reverse-strand anchors q' =
    n - 1 - q reaches 65534 and 0; `shorter` 65534 bases, C / G first; `two_tiles` 257 bases A / T"""
    rng = np.random.default_rng(64)
    at = lambda n: (1 + 3 * rng.integers(0, 2, size=n)).astype(np.int32)
    cg = lambda n: (2 + rng.integers(0, 2, size=n)).astype(np.int32)
    ref = np.concatenate([at(OCC_REF_KEPT), cg(OCC_REF_DROPPED)])
    rng.shuffle(ref)
    sparse = cg(65535)
    where = np.concatenate([[0, 65534], rng.choice(np.arange(1, 65534), size=298, replace=False)])
    sparse[where] = at(300)
    shorter = np.concatenate([cg(300), at(65234)])
    return [int(v) for v in ref], dict(dense=at(65535), sparse=sparse, shorter=shorter, two_tiles=at(257))


OCC_READS = ("dense", "sparse", "shorter", "two_tiles")


@functools.lru_cache(maxsize=None)
def occ_index():
    return RR.index_ref(occ()[0], 1, 1)


def fast_anchors_k1(labels, index, max_occ, cap):
    """tests/readmap_ref.anchors_ref at k = w = 1 in whole arrays: (the kept anchors [(s, r, q')] in enumeration order, n_minimizers,
    truncated, the true anchor total).  Every base 1..4 is a minimizer: canon min(v - 1, 4 - v), on the reverse strand for v in {3, 4}"""
    v = np.asarray(labels, dtype=np.int64)
    n = len(v)
    valid = (v >= 1) & (v <= 4)
    canon = np.minimum(v - 1, 4 - v)
    hits = {c: [(p, s) for cc, p, s in index if cc == c] for c in (0, 1)}
    per = np.zeros(n, dtype=np.int64)
    for c in (0, 1):
        if len(hits[c]) <= max_occ:
            per[valid & (canon == c)] = len(hits[c])
    total = int(per.sum())
    ends = np.cumsum(per)
    last = int(np.searchsorted(ends, min(total, cap), side="left")) + 1 if total else 0     # positions that hold a kept anchor
    out = []
    for q in np.flatnonzero(per[:last]).tolist():
        s_read = 1 if v[q] >= 3 else 0
        for p, s_ref in hits[int(canon[q])]:
            s = s_read ^ s_ref
            out.append((s, p, q if s == 0 else n - 1 - q))
    return out[:cap], int(valid.sum()), 1 if total > cap else 0, total


def fast_chain_strand(anchors, k, h, max_dist, bandwidth, gap_base, gap_log):
    """tests/readmap_ref.chain_strand_ref with the h predecessors of an anchor in whole arrays: the same (f, pred, root, count)"""
    n = len(anchors)
    r = np.array([a[0] for a in anchors], dtype=np.int64)
    q = np.array([a[1] for a in anchors], dtype=np.int64)
    f = np.zeros(n, dtype=np.int64)
    pred, root, count = [-1] * n, list(range(n)), [1] * n
    for i in range(n):
        lo = max(0, i - h)
        dr, dq = r[i] - r[lo:i], q[i] - q[lo:i]
        dd = np.abs(dr - dq)
        ok = (dr > 0) & (dr <= max_dist) & (dq > 0) & (dq <= max_dist) & (dd <= bandwidth)
        f[i] = 16 * k
        if not ok.any():
            continue
        gap = np.where(dd > 0, gap_base * dd + gap_log * (np.frexp(dd.astype(np.float64))[1] - 1), 0)      # frexp: the bit length
        cand = np.where(ok, f[lo:i] + 16 * np.minimum(np.minimum(dr, dq), k) - gap, -(1 << 62))
        j = len(cand) - 1 - int(np.argmax(cand[::-1]))               # of equal candidates the nearest
        if cand[j] > 16 * k:                                         # the fresh start wins a tie
            f[i], pred[i], root[i], count[i] = cand[j], lo + j, root[lo + j], count[lo + j] + 1
    return [int(v) for v in f], pred, root, count


def fast_chain_ref(sorted_anchors, n, k, **kw):
    """tests/readmap_ref.chain_ref over fast_chain_strand (the plain function's own code with the strand loop swapped)"""
    plain = RR.chain_strand_ref
    RR.chain_strand_ref = fast_chain_strand
    try:
        return RR.chain_ref(sorted_anchors, n, k, **kw)
    finally:
        RR.chain_strand_ref = plain


@functools.lru_cache(maxsize=None)
def occ_results(cap):
    """per read a dict: keys (the kept anchors sorted, packed), n_anchors, n_minimizers, truncated, total, and chain: the row of
    tests/readmap_ref.chain_ref over the kept anchors at h = OCC_H[cap], by fast_chain_ref"""
    ref, reads = occ()
    out = []
    for name in OCC_READS:
        anchors, n_min, truncated, total = fast_anchors_k1(reads[name], occ_index(), 64, cap)
        rows = sorted(anchors)
        out.append(dict(keys=[RR.pack(a) for a in rows], rows=rows, n_anchors=len(rows), n_minimizers=n_min, truncated=truncated, total=total,
                        chain=fast_chain_ref(rows, len(reads[name]), 1, h=OCC_H[cap])))
    return out


# ---- the full window of predecessors
WINDOW_H = (1024, 1000)
WINDOW_ANCHORS, WINDOW_SEED = 1400, 10
WINDOW_KW = dict(max_dist=4000, bandwidth=12, gap_base=3, gap_log=2)
WINDOW_K = 15


@functools.lru_cache(maxsize=None)
def window_anchors():
    """1400 distinct seeded anchors of the forward strand: 28 reference positions 100 apart with 50 read positions each, so that a
    window of 1024 predecessors spans 20 reference positions, and a bandwidth of 12 that leaves most anchors no near predecessor"""
    rng = np.random.default_rng(WINDOW_SEED)
    rows = set()
    while len(rows) < WINDOW_ANCHORS:
        rows.add((0, 100 * int(rng.integers(0, 28)), int(rng.integers(0, 3000))))
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def window_reference(h):
    return RR.chain_ref(window_anchors(), 20000, WINDOW_K, h=h, **WINDOW_KW)


def reach_anchors(d):
    """d + 1 anchors: the last chains to the first and to nothing else, and the first is d positions before it (the construction
    of tests/test_gpu_readmap.py)"""
    return [(0, 0, 0)] + [(0, 1 + t, 10000 - t) for t in range(d - 1)] + [(0, d + 10, 20)]


WINDOW_REACH = (999, 1000, 1001, 1023, 1024, 1025)
WINDOW_REACH_KW = dict(max_dist=5000, bandwidth=2000, gap_base=0, gap_log=0)     # the last anchor lies d - 10 off the first one's diagonal


# ================================================================================================================= demultiplexing
DX_FRONT, DX_REAR, DX_WINDOW = 513, 511, 16
DX_PLANTS = ((70, 134), (75, 139), (3, 67))     # read b begins with the pattern planted at both indices of DX_PLANTS[b]


@functools.lru_cache(maxsize=None)
def demux_case():
    """kDxMaxPatterns = 1024: 513 front and 511 rear patterns of 1 to 12 labels, three reads.  Read b begins with a pattern of 12
    labels that stands at two front indices: 70 and 134 in two groups (one lane of the pick's strided loop, two of its rounds: the
    pick is 70 and the runner-up ties with it), 75 and 139 in ONE group (the runner-up is another group's best), 3 and 67 in two
    groups (the pick lies below 64, its equal above)"""
    rng = np.random.default_rng(1024)
    front, rear = DC._mixed(rng, DX_FRONT, 1, 12), DC._mixed(rng, DX_REAR, 1, 12)
    reads = []
    for (lo, hi), n in zip(DX_PLANTS, (40, 30, 13)):
        plant = DC._rand(rng, 12)
        front[lo], front[hi] = plant, list(plant)
        reads.append(plant + DC._rand(rng, n - 12))
    group = list(range(DX_FRONT)) + list(range(DX_REAR))
    group[139] = group[75]
    return DC._case(reads, front, rear, DX_WINDOW, group=group)


@functools.lru_cache(maxsize=None)
def demux_reference():
    case = demux_case()
    return DR.demux_scores_ref(case.labels, case.lengths, case.patterns, case.pattern_lengths, case.n_front, case.window, *case.costs)


DX_PICKS = ((0, 1, 0.0), (1, 2, 1.0), (1, 1, 0.0))     # (min_fraction as num / den, min_margin)


def demux_pick_reference(num, den, margin, require_both=False):
    case, ref = demux_case(), demux_reference()
    return DR.demux_pick_ref(ref["score"], ref["start"], ref["end"], case.lengths, case.group, DC.min_scores(case, num, den), case.n_front,
                             int(2 * margin), require_both)
