"""The definition of wn_signal_map_reference and wn_signal_map (include/wavenet_amd.h) on the host: the minimum-cost stay / step
path of the samples of a read through consecutive states of a reference, start free and end free, with the origin of every cell
carried beside its cost.  Samples are quantised as wn_kmer_events does (tests/kmer_events_ref.quantise) and cost what
wn_signal_align charges (tests/signal_align_ref.cost_row); every number after the quantisation is an integer.  The dynamic program
walks the samples in a Python loop with one numpy row per sample; the block table and the runner-up are plain loops."""
import numpy as np

from tests.kmer_events_ref import kmer_index
from tests.signal_align_ref import BAD_READ, INF, OFFSET_LIMIT, Q_LIMIT, cost_row, read_samples

NO_MAPPING = (1 << 63) - 1              # LLONG_MAX
GRANULE = 64                            # WN_MAP_GRANULE


def join_strands(bases):
    """bases + [0] + reverse complement; 1..4 become 5 - base, anything else stays"""
    bases = [int(v) for v in bases]
    return bases + [0] + [5 - v if 1 <= v <= 4 else v for v in reversed(bases)]


def prepare(ref, model, k):
    """(codes [M] int64, the k-mer of every state or -1 for a wall; the faults counted in *bad).  A label outside 0..4 counts once
    where it stands; a state whose window lies in 1..4 and whose model row is out of range counts once; both make walls."""
    ref = [int(v) for v in ref]
    model = np.asarray(model, dtype=np.int64)
    M = len(ref) - k + 1
    bad = sum(1 for v in ref if v < 0 or v > 4)
    codes = np.full(M, -1, dtype=np.int64)
    for j in range(M):
        window = ref[j:j + k]
        if any(v < 1 or v > 4 for v in window):
            continue
        code = kmer_index(window)
        level, weight, offset = (int(v) for v in model[code])
        if weight < 1 or abs(level) >= Q_LIMIT or abs(offset) >= OFFSET_LIMIT:
            bad += 1
            continue
        codes[j] = code
    return codes, bad


def last_row(q, codes, model, S, max_cost):
    """(D [M] int64 with INF, O [M] int64) after the last sample of q (at least one)"""
    model = np.asarray(model, dtype=np.int64)
    open_ = codes >= 0
    rows = model[np.where(open_, codes, 0)]
    level, weight, offset = rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()
    level[~open_], weight[~open_], offset[~open_] = 0, 1, 0            # a wall's row is never used
    M = len(codes)
    D = np.where(open_, cost_row(q[0], level, weight, offset, S, max_cost), INF)
    O = np.arange(M, dtype=np.int64)
    for t in range(1, len(q)):
        step = np.concatenate([[INF], D[:-1]])
        step_o = np.concatenate([[-1], O[:-1]])
        took = step < D                                              # the step replaces the stay only if strictly smaller
        m = np.where(took, step, D)
        O = np.where(took, step_o, O)
        D = np.where(open_ & (m < INF), m + cost_row(q[t], level, weight, offset, S, max_cost), INF)
    return D, O


def block_table(D):
    """(block_cost list of Python integers, block_end list) of a last row"""
    cost, end = [], []
    for g0 in range(0, len(D), GRANULE):
        cells = [int(v) for v in D[g0:g0 + GRANULE]]
        low = min(cells)
        if low >= INF:
            cost.append(NO_MAPPING)
            end.append(-1)
        else:
            cost.append(low)
            end.append(g0 + cells.index(low))
    return cost, end


def runner_up_of(block_cost, end, T):
    """the minimum over the blocks that lie wholly T or more states from `end`; NO_MAPPING if there is none"""
    best = NO_MAPPING
    for g, c in enumerate(block_cost):
        if GRANULE * g + GRANULE - 1 <= end - T or GRANULE * g >= end + T:
            best = min(best, c)
    return best


def signal_map_ref(signal, signal_lengths, ref, model, k, frac_bits=12, weight_shift=32, max_cost=None, scale_shift=None):
    """signal [B, L] float32 or int16; ref [R] integers; model [4^k, 3] integers.  Returns a dict: score, runner_up [B] object
    (Python integers), end, start [B] int32, block_cost [B, G] object, block_end [B, G] int32, end_cost [B, M] object, bad (reads),
    ref_bad (the faults of the reference)."""
    B, L = signal.shape
    max_cost = (1 << 31) - 1 if max_cost is None else int(max_cost)
    codes, ref_bad = prepare(ref, model, k)
    M = len(codes)
    G = (M + GRANULE - 1) // GRANULE
    score, runner = [BAD_READ] * B, [BAD_READ] * B
    end, start = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    block_cost = np.full((B, G), BAD_READ, dtype=object)
    block_end = np.full((B, G), -1, dtype=np.int32)
    end_cost = np.full((B, M), BAD_READ, dtype=object)
    bad = 0
    for b in range(B):
        T = int(signal_lengths[b])
        if not 0 <= T <= L:
            bad += 1
            continue
        q = None if T == 0 else read_samples(signal[b], T, None if scale_shift is None else scale_shift[b], frac_bits)
        if T > 0 and q is None:
            bad += 1
            continue
        score[b] = runner[b] = NO_MAPPING
        block_cost[b, :] = NO_MAPPING
        end_cost[b, :] = NO_MAPPING
        if T == 0:
            continue
        D, O = last_row(q, codes, model, weight_shift, max_cost)
        end_cost[b, :] = [int(v) if v < INF else NO_MAPPING for v in D]
        bc, be = block_table(D)
        block_cost[b, :], block_end[b, :] = bc, be
        low = min(bc)
        if low == NO_MAPPING:
            continue
        e = be[bc.index(low)]
        score[b], end[b], start[b] = low, e, int(O[e])
        runner[b] = runner_up_of(bc, e, T)
    return {"score": np.array(score, dtype=object), "end": end, "start": start, "runner_up": np.array(runner, dtype=object),
            "block_cost": block_cost, "block_end": block_end, "end_cost": end_cost, "bad": bad, "ref_bad": ref_bad}


def strand_of(end, R, both_strands=True):
    return -1 if end < 0 else int(both_strands and end > R)


def ref_span_of(start, end, R, k, both_strands=True):
    """forward-strand half-open base coordinates of a mapping in the joined sequence"""
    if end < 0:
        return (-1, -1)
    if strand_of(end, R, both_strands) == 0:
        return (start, end + k)
    s, e = start - (R + 1), end - (R + 1)
    return (R - e - k, R - s)
