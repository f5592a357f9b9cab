"""The inputs that tests/test_leftalign_ref.py (CPU) and tests/test_gpu_leftalign.py share, each built once.

short_rows(): every op string of 1 to 7 columns over {aligned, 3, 4} with two random labelings from a two-letter alphabet (an
aligned column is op 1 or 2 as its labels say).

The repeat-planted run: a seeded random reference of 2000 bases into which ten exact repeats are written -- five homopolymers of 5
to 8, three 2-mers x 4 or 5, a 3-mer x 3 and a 4-mer x 3, every unit primitive, the base before the repeat different from the
unit's last label and the base after it from its first, so that the repeat is exactly k copies -- at least 100 bases from either
end and from each other.  The sample genome deletes or inserts one unit (of a homopolymer: one or two copies) at the RIGHT end of
each repeat; the expected records are on the LEFTMOST placement, anchored on the base before the repeat.  48 reads of 300 to 500
bases on alternating strands, at least 5 deep between the outermost edits, windows widened by a flank of 8; error-free and with 2 %
substitutions.

The seeds are CONDITIONS, not measurements (tests/test_leftalign_ref.py asserts all three): (i) the host chain pairwise_align_ref
-> leftalign_ref -> pileup_ref -> call_consensus_ref -> variants_ref returns the sample as the consensus and exactly the planted
records in both runs; (ii) the same chain WITHOUT the left-alignment fails that in the error-free run; (iii) every read settles
within the default max_passes."""
import functools
import itertools

import numpy as np

from tests import leftalign_ref as L
from tests import pairwise_align_ref as A
from tests import pileup_cases as C
from tests import pileup_ref as P

PLANT_SEED = 2
NOISE_SEED = 0
PLANT_REF = 2000
PLANT_READS = 48
PLANT_FLANK = 8
NOISE = 0.02
# (unit length, copies (lo, hi), units edited (lo, hi))
SITES = ((1, (5, 8), (1, 2)),) * 5 + ((2, (4, 5), (1, 1)),) * 3 + ((3, (3, 3), (1, 1)), (4, (3, 3), (1, 1)))
SHORT_SEED = 11
SHORT_MAX = 7


def label_row(shape, rng, alphabet=(1, 2)):
    """(ops, a, b) of a shape over {0 aligned, 3, 4} with random labels: an aligned column is op 1 or 2 as its labels say"""
    a = [int(rng.choice(alphabet)) for v in shape if v != 4]
    b = [int(rng.choice(alphabet)) for v in shape if v != 3]
    ops, i, j = [], 0, 0
    for v in shape:
        if v == 0:
            ops.append(1 if a[i] == b[j] else 2)
        else:
            ops.append(v)
        i += v != 4
        j += v != 3
    return ops, a, b


@functools.lru_cache(maxsize=None)
def short_rows():
    """[(ops, a, b)]: every shape of 1..SHORT_MAX columns, two labelings each"""
    rng = np.random.default_rng(SHORT_SEED)
    out = []
    for n in range(1, SHORT_MAX + 1):
        for shape in itertools.product((0, 3, 4), repeat=n):
            out += [label_row(shape, rng), label_row(shape, rng)]
    return out


def batch(rows_):
    """[(ops, a, b)] -> (ops rows uint8, ops_len, a rows, a lengths, b rows, b lengths)"""
    ops, ops_len = C.rows([r[0] for r in rows_], dtype=np.uint8)
    a, a_len = C.rows([r[1] for r in rows_])
    b, b_len = C.rows([r[2] for r in rows_])
    return ops, ops_len, a, a_len, b, b_len


def _primitive(unit):
    return not any(len(unit) % p == 0 and unit == unit[:p] * (len(unit) // p) for p in range(1, len(unit)))


def _plant(rng):
    """reference, sample, origin (the reference position of every sample base; an inserted base has its predecessor's) and the
    records [(pos, kind, ref labels, alt labels)] on the leftmost placement, sorted by position"""
    ref = [int(v) for v in rng.integers(1, 5, size=PLANT_REF)]
    order = [SITES[int(k)] for k in rng.permutation(len(SITES))]
    edits = []
    for k, (u, copies, units) in enumerate(order):
        p = 150 + 170 * k + int(rng.integers(0, 41))
        while True:
            unit = [int(v) for v in rng.integers(1, 5, size=u)]
            if _primitive(unit):
                break
        n_copies, n_units = int(rng.integers(copies[0], copies[1] + 1)), int(rng.integers(units[0], units[1] + 1))
        kind = "del" if rng.random() < 0.5 else "ins"
        end = p + u * n_copies
        ref[p:end] = unit * n_copies
        ref[p - 1] = unit[-1] % 4 + 1                                # the repeat is exactly n_copies copies
        ref[end] = unit[0] % 4 + 1
        edits.append((p, end, kind, unit * n_units))
    assert edits[0][0] >= 100 and edits[-1][1] <= PLANT_REF - 100 and all(y[0] - x[1] >= 100 for x, y in zip(edits, edits[1:]))
    sample, origin, records, at = [], [], [], 0
    for p, end, kind, change in edits:
        n = len(change)
        if kind == "del":                                            # the last n bases of the repeat are gone
            sample += ref[at:end - n]
            origin += range(at, end - n)
            records.append((p - 1, "del", tuple(ref[p - 1:p + n]), (ref[p - 1],)))
        else:                                                        # n more bases after the repeat
            sample += ref[at:end] + change
            origin += list(range(at, end)) + [end - 1] * n
            records.append((p - 1, "ins", (ref[p - 1],), (ref[p - 1],) + tuple(change)))
        at = end
    sample += ref[at:]
    origin += range(at, PLANT_REF)
    return ref, sample, origin, records, edits


@functools.lru_cache(maxsize=None)
def repeat_planted(noisy=False, seed=PLANT_SEED):
    """dict: ref, sample, records, reads (lists of labels as sequenced), strand, window [(lo, length)], labels, lengths"""
    rng = np.random.default_rng(seed)
    ref, sample, origin, records, edits = _plant(rng)
    S = len(sample)
    spans = []
    for b in range(PLANT_READS):
        n = int(rng.integers(300, 501))
        if b < 6:
            start = 0
        elif b < 12:
            start = S - n
        else:
            start = int(round((b - 12) * (S - 500) / (PLANT_READS - 13))) + int(rng.integers(-10, 11))
            start = min(max(start, 0), S - n)
        spans.append((start, start + n))
    rng.shuffle(spans)
    cover = np.zeros(S, dtype=np.int64)
    for s, e in spans:
        cover[s:e] += 1
    lo_edit, hi_edit = origin.index(edits[0][0] - 1), S - 1 - origin[::-1].index(edits[-1][1])
    assert cover[lo_edit:hi_edit + 1].min() >= 5, int(cover[lo_edit:hi_edit + 1].min())
    noise = np.random.default_rng(NOISE_SEED)
    reads, strand, window = [], [], []
    for b, (s, e) in enumerate(spans):
        seq = list(sample[s:e])
        if noisy:
            for t in range(len(seq)):
                if noise.random() < NOISE:
                    seq[t] = (seq[t] - 1 + int(noise.integers(1, 4))) % 4 + 1
        strand.append(b & 1)
        reads.append(C.revcomp(seq) if b & 1 else seq)
        lo, hi = max(origin[s] - PLANT_FLANK, 0), min(origin[e - 1] + 1 + PLANT_FLANK, PLANT_REF)
        window.append((lo, hi - lo))
    labels, lengths = C.rows(reads)
    return dict(ref=ref, sample=sample, records=records, reads=reads, strand=strand, window=window, labels=labels, lengths=lengths)


def host_chain(run, ops_rows, ops_len, left):
    """pileup_ref -> call_consensus_ref -> variants_ref over op rows, after leftalign_ref if `left`: dict ops, aligned (None
    without), pile, calls, variants"""
    lo, n_ref = [w[0] for w in run["window"]], [w[1] for w in run["window"]]
    aligned = None
    if left:
        windows, _ = C.rows([C.window_labels(run["ref"], w[0], w[1], s) for w, s in zip(run["window"], run["strand"])])
        aligned = L.left_align_ref(ops_rows, ops_len, windows, n_ref, run["labels"], run["lengths"], run["strand"])
        ops_rows = aligned.ops
    pile = P.pileup_ref(ops_rows, ops_len, lo, n_ref, run["strand"], run["labels"], run["lengths"], len(run["ref"]))
    calls = P.call_consensus_ref(pile, run["ref"])
    return dict(ops=ops_rows, aligned=aligned, pile=pile, calls=calls, variants=P.variants_ref(run["ref"], calls, pile))


@functools.lru_cache(maxsize=None)
def repeat_host(noisy=False, left=True, seed=PLANT_SEED):
    """the host chain on the repeat-planted windows, with or without the left-alignment"""
    run = repeat_planted(noisy, seed)
    ops = [A.align(C.window_labels(run["ref"], lo, n, s), read).ops for (lo, n), s, read in zip(run["window"], run["strand"], run["reads"])]
    ops_rows, ops_len = C.rows([list(o) for o in ops], dtype=np.uint8)
    return dict(host_chain(run, ops_rows, ops_len, left), ops_len=ops_len, raw_ops=ops_rows)
