"""The inputs that tests/test_realign_ref.py (CPU), tests/test_realign_abi.py and tests/test_gpu_realign.py share, each built once: the
hand rows of the composition and of the windows, the read-end family, random valid op pairs, and the realignment of the PLANTED
PHASED run of tests/phase_cases.py (PLANT_SEED 2, NOISE_SEED 0) through the host chain.

The conditions of the planted run (tests/test_realign_ref.py asserts them on the host chain, tests/test_gpu_realign.py on the
device's tables), in both variants: every read with a heterozygous site in its window picks its planted haplotype, by at least
MIN_DELTA half units; every other read ties; haplotag tags exactly the same reads with the same hp; the observations at sites that
show NEITHER called allele fall from NEITHER_BEFORE to NEITHER_AFTER; alleles, flags, ins_copies and ins_len of the calls are the
same before and after, and no gq drops.  They hold for the committed seeds of tests/phase_cases.py as they stand."""
import functools

import numpy as np

from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import leftalign_ref as L
from tests import pairwise_align_ref as A
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import pileup_ref as P
from tests import realign_ref as RR

DECIDED = 143                                 # reads with a heterozygous site in their window, of 160
MIN_DELTA = 20                                # half units
NEITHER_BEFORE = {False: 3, True: 17}         # by `noisy`
NEITHER_AFTER = {False: 0, True: 8}
LOWER_SCORE = {False: 3, True: 6}             # reads whose lifted score is below their own alignment's; equal for the rest

# ---- the composition by hand: (what, A, Hh, reference window, read, the result) -----------------------------------------------------
LIFT_ROWS = [
    ("a and g: compared afresh, whatever the two rows say", [1, 2, 1], [2, 1, 2], [1, 2, 3], [1, 2, 4], [1, 1, 2]),
    ("a only: the read's label against a gap", [1, 1, 1], [1, 4, 1], [1, 2], [1, 3, 2], [1, 4, 1]),
    ("g only: the reference's label against a gap", [1, 3, 1], [1, 1, 1], [1, 2, 3], [1, 3], [1, 3, 1]),
    ("neither: the column vanishes", [1, 3, 1], [1, 4, 1], [1, 2], [1, 2], [1, 1]),
    ("3s before 4s in one slot", [1, 4, 4, 1], [1, 3, 3, 1], [1, 2, 2, 3], [1, 4, 4, 3], [1, 3, 3, 4, 4, 1]),
    ("trailing runs, the 3s first", [1, 4, 4], [1, 3], [2, 2], [2, 3, 3], [1, 3, 4, 4]),
    ("leading runs", [4, 1], [3, 3, 1], [1, 1, 2], [4, 2], [3, 3, 4, 1]),
    ("an empty read", [3, 3], [1, 3, 2], [1, 2, 3], [], [3, 3, 3]),
    ("an empty haplotype: an all-deleted window", [4, 4], [3, 3, 3], [1, 2, 3], [4, 4], [3, 3, 3, 4, 4]),
    ("a vanishing column between runs", [4, 3, 4, 1], [3, 4, 3, 2], [1, 2, 3], [4, 4, 3], [3, 4, 3, 4, 1]),
]
LIFT_BAD = [
    ("an op outside 1..4 in A", [1, 5, 1], [1, 1, 1], [1, 2, 3], [1, 2, 3]),
    ("an op 0 in Hh", [1, 1, 1], [1, 0, 1], [1, 2, 3], [1, 2, 3]),
    ("A holds a haplotype label too few", [1, 1], [1, 1, 1], [1, 2, 3], [1, 2]),
    ("A holds a haplotype label too many", [1, 1, 3, 1], [1, 1, 1], [1, 2, 3], [1, 2, 3]),
    ("A does not consume the read", [1, 1, 1], [1, 1, 1], [1, 2, 3], [1, 2, 3, 4]),
    ("Hh does not consume the window", [1, 1, 1], [1, 1, 1], [1, 2, 3, 4], [1, 2, 3]),
    ("Hh consumes more than the window", [1, 1, 1], [1, 1, 1, 3], [1, 2, 3], [1, 2, 3]),
]

# ---- the windows by hand: a reference of 12 with every rule inside ------------------------------------------------------------------
WINDOW_REF = [1, 2, 3, 4, 1, 7, 3, 4, 1, 2, 3, 4]                    # the label at 5 is no base
WINDOW_MAX_INS = 3


def window_calls():
    """haplotype 0: a substitution at 1, positions 3..4 deleted, the no-base label kept at 5, insertions after 0 (1 base), after 6
    (max_ins bases, the last of them no base) and after 11; haplotype 1: the reference with position 8 deleted and the no-base label
    called as a base"""
    call = np.array([WINDOW_REF, WINDOW_REF], dtype=np.uint8)
    call[0][1], call[0][3], call[0][4] = 4, 0, 0
    call[1][8], call[1][5] = 0, 2
    ins_len = np.zeros((2, 12), dtype=np.uint8)
    ins_bases = np.zeros((2, 12, WINDOW_MAX_INS), dtype=np.uint8)
    for p, bases in ((0, [3]), (6, [1, 1, 7]), (11, [2, 2])):
        ins_len[0][p] = len(bases)
        ins_bases[0][p][:len(bases)] = bases
    return RR.HapCalls(call, ins_len, ins_bases)


# ---- the read-end family ------------------------------------------------------------------------------------------------------------
END_REF = [1, 3, 2, 4, 1, 2, 4, 3, 1, 4, 2, 3, 4, 1, 3, 2, 1, 4, 3, 2, 4, 2, 1, 3, 4, 3, 1, 2, 4, 1,
           2, 3, 1, 4, 2, 1, 3, 4, 2, 3, 1, 2, 4, 3, 2, 1, 4, 1, 3, 2]
END_AT = 30                                   # END_REF[29:33] = 1, 2, 3, 1: no shift of the gap gives the same sequence
END_EDITS = (("del", 1, []), ("del", 2, []), ("ins", 2, [4, 4]))
END_FLANK = 4


def end_case(kind, n, inserted, past, strand):
    """a read of haplotype 0, which carries the edit at END_AT, from position 6 to `past` bases behind the edit, on `strand`; haplotype 1
    is the reference -> dict hcalls, read, lo, length, window (read orientation)"""
    R = len(END_REF)
    call = np.array([END_REF, END_REF], dtype=np.uint8)
    ins_len = np.zeros((2, R), dtype=np.uint8)
    ins_bases = np.zeros((2, R, 2), dtype=np.uint8)
    if kind == "del":
        call[0][END_AT:END_AT + n] = 0
        seq, end = END_REF[6:END_AT] + END_REF[END_AT + n:END_AT + n + past], END_AT + n + past
    else:
        ins_len[0][END_AT], ins_bases[0][END_AT] = n, inserted
        seq, end = END_REF[6:END_AT + 1] + inserted + END_REF[END_AT + 1:END_AT + 1 + past], END_AT + 1 + past
    lo, hi = 6 - END_FLANK, end + END_FLANK
    return dict(hcalls=RR.HapCalls(call, ins_len, ins_bases), read=C.revcomp(seq) if strand else seq, lo=lo, length=hi - lo,
                window=C.window_labels(END_REF, lo, hi - lo, strand))


def end_support(case, ops, kind, n, strand):
    """what pileup_ref counts for the edit from one op row: the deletions at END_AT (all n positions: 1), or the insertions of length n"""
    ops_rows, ops_len = C.rows([list(ops)], dtype=np.uint8)
    labels, lengths = C.rows([case["read"]])
    pile = P.pileup_ref(ops_rows, ops_len, [case["lo"]], [case["length"]], [strand], labels, lengths, len(END_REF), max_ins=2)
    if kind == "del":
        return min(int(pile.counts[END_AT + t][strand][4]) for t in range(n))
    return int(pile.ins_lengths[END_AT][n - 1])


# ---- random valid pairs of rows -----------------------------------------------------------------------------------------------------

def random_pair(rng, n_hh, p=(0.45, 0.15, 0.2, 0.2), extra=0.2, labels=3):
    """(A, Hh, reference window, read) that compose: Hh has n_hh random columns; A holds Hh's haplotype labels as random ops 1..3
    with op-4 columns strewn between at rate `extra`; labels 1..`labels`, so that matches are common"""
    hh = [int(v) for v in rng.choice([1, 2, 3, 4], size=n_hh, p=p)]
    a = []
    for _ in range(sum(v != 3 for v in hh)):
        while rng.random() < extra:
            a.append(4)
        a.append(int(rng.choice([1, 2, 3], p=[0.6, 0.2, 0.2])))
    while rng.random() < extra:
        a.append(4)
    ref = [int(v) for v in rng.integers(1, labels + 1, size=sum(v != 4 for v in hh))]
    read = [int(v) for v in rng.integers(1, labels + 1, size=sum(v != 3 for v in a))]
    return a, hh, ref, read


def pair_batch(pairs, pick=None, H=1):
    """pairs of random_pair / the hand rows as lift_ref's arguments: every pair lies on haplotype pick[b], the other haplotype's rows
    hold garbage -> (a_ops [H][B][.], a_len, Windows, pick, ref rows, ref_len, read rows, read_len)"""
    B = len(pairs)
    pick = [0] * B if pick is None else pick
    wa, wh = max(1, max(len(p[0]) for p in pairs)), max(1, max(len(p[1]) for p in pairs))
    a_ops, a_len = np.full((H, B, wa), 9, dtype=np.uint8), np.full((H, B), -7, dtype=np.int32)
    h_ops, h_len, lengths = np.full((H, B, wh), 9, dtype=np.uint8), np.full((H, B), -7, dtype=np.int32), np.full((H, B), -7, dtype=np.int32)
    for b, (a, hh, _, _) in enumerate(pairs):
        h = pick[b] if 0 <= pick[b] < H else 0
        a_ops[h][b], h_ops[h][b] = 0, 0
        a_ops[h][b][:len(a)], h_ops[h][b][:len(hh)] = a, hh
        a_len[h][b], h_len[h][b], lengths[h][b] = len(a), len(hh), sum(v != 3 for v in hh)
    ref, ref_len = C.rows([p[2] for p in pairs])
    read, read_len = C.rows([p[3] for p in pairs])
    windows = RR.Windows(np.zeros((H, B, wh), dtype=np.int32), lengths, h_ops, h_len, np.ones(B, dtype=np.int8), 0)
    return a_ops, a_len, windows, pick, ref, ref_len, read, read_len


# ---- random haplotypes and reads drawn from them ------------------------------------------------------------------------------------

def random_calls(rng, R, H=2, max_ins=3, rate=0.05, odd=0.02, deleted=(), inserted=()):
    """(reference labels, HapCalls): a random reference with a share `odd` of labels that are no base (7); every haplotype differs
    from it by substitutions and deletions at `rate` each and carries insertions of 1..max_ins labels at `rate`; haplotype 0 is
    deleted at the positions `deleted` and carries max_ins labels after the positions `inserted`"""
    reference = np.where(rng.random(R) < odd, 7, rng.integers(1, 5, size=R)).astype(np.int32)
    call = np.tile(reference, (H, 1)).astype(np.uint8)
    ins_len = np.zeros((H, R), dtype=np.uint8)
    ins_bases = np.zeros((H, R, max_ins), dtype=np.uint8)
    for h in range(H):
        u = rng.random(R)
        call[h][u < rate] = rng.integers(1, 5, size=int((u < rate).sum()))
        call[h][(u >= rate) & (u < 2 * rate)] = 0
        if max_ins:
            at = np.flatnonzero(rng.random(R) < rate)
            ins_len[h][at] = rng.integers(1, max_ins + 1, size=len(at))
    call[0][list(deleted)] = 0
    if max_ins:
        ins_len[0][list(inserted)] = max_ins
    for h in range(H):
        for p in np.flatnonzero(ins_len[h]):
            ins_bases[h][p][:ins_len[h][p]] = np.where(rng.random(ins_len[h][p]) < odd, 7, rng.integers(1, 5, size=ins_len[h][p]))
    return [int(v) for v in reference], RR.HapCalls(call, ins_len, ins_bases)


def drawn_reads(rng, reference, hcalls, spans, noise=0.03):
    """spans [(lo, n, strand, haplotype)] -> (reads, the reference windows in read orientation): a read is its haplotype over the
    window as sequenced on its strand, with substitutions at `noise`; a read without a label gets one"""
    reads, windows = [], []
    for lo, n, strand, h in spans:
        labels, _ = RR.window_rows(hcalls.call[h], hcalls.ins_len[h], hcalls.ins_bases[h], reference, lo, n, strand, hcalls.ins_bases.shape[2])
        read = [int(rng.integers(1, 5)) if rng.random() < noise else v for v in labels] or [1]
        reads.append(read)
        windows.append(C.window_labels(reference, lo, n, strand))
    return reads, windows


# ---- the planted run ----------------------------------------------------------------------------------------------------------------

def windows_of(run):
    """(lo, ref_lengths, the windows in read orientation) of a planted run"""
    lo, n = [w[0] for w in run["window"]], [w[1] for w in run["window"]]
    return lo, n, [C.window_labels(run["ref"], a, k, s) for a, k, s in zip(lo, n, run["strand"])]


def recall(run, ops_rows, ops_len, lo, ref_lengths, sites):
    """pile, calls and the observations at `sites` of given op rows, as the host chain of tests/phase_cases.py makes them"""
    args = (ops_rows, ops_len, lo, ref_lengths, run["strand"], run["labels"], run["lengths"])
    pile = P.pileup_ref(*args, PC.PLANT_REF, qual=run["qual"], min_qual=PC.MIN_QUAL)
    ev = G.evidence_ref(K.weights(), *args, PC.PLANT_REF, qual=run["qual"], min_qual=PC.MIN_QUAL)
    calls = G.call_genotypes_ref(pile, ev.evidence, run["ref"], K.weights(), alt_prior=K.ALT_PRIOR)
    observed = H.links_ref(sites, *args, qual=run["qual"], min_qual=PC.MIN_QUAL, reach=1).observed
    return dict(pile=pile, evidence=ev, calls=calls, observed=observed)


def left_aligned(run, lifted, refs):
    """the lifted rows through tests/leftalign_ref.py, as rows"""
    rows = [L.left_align_row(list(lifted.ops[b][:lifted.ops_len[b]]), refs[b], run["reads"][b], run["strand"][b])[0] for b in range(len(refs))]
    return C.rows([list(r) for r in rows], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def planted_realigned(noisy=False):
    """the host chain of tests/phase_cases.py, then haplotype_calls -> realign -> left_align -> pile, evidence, calls: dict hcalls,
    realigned (a realign_ref.Realigned), ops, ops_len (left-aligned), before and after (recall's dicts)"""
    run, host = PC.planted(noisy), PC.planted_host(noisy)
    lo, n, refs = windows_of(run)
    hcalls = RR.haplotype_calls_ref(host["calls"], host["sites"], host["chain"])
    realigned = RR.realign_ref(refs, n, run["reads"], lo, run["strand"], hcalls, run["ref"])
    ops_rows, ops_len = left_aligned(run, realigned.lifted, refs)
    return dict(hcalls=hcalls, realigned=realigned, ops=ops_rows, ops_len=ops_len, before=recall(run, host["ops"], host["ops_len"], lo, n, host["sites"]),
                after=recall(run, ops_rows, ops_len, lo, n, host["sites"]))


def check_conditions(run, host, realigned, before, after, noisy, own_scores=None, windows=None, exact=True):
    """the conditions of the planted run on a Realigned (or the device's lists under the same names) and recall's dicts before and
    after; windows: (lo, ref_lengths) where they are not the planted ones (the device's mapping) -- with exact=False the two figures
    that belong to the planted windows, NEITHER_BEFORE and LOWER_SCORE, are printed and not asserted: the figure after realignment
    is, and that it fell"""
    lo, n = windows_of(run)[:2] if windows is None else windows
    in_window = [any(a <= p < a + k for p in host["sites"].pos) for a, k in zip(lo, n)]
    lower = None if own_scores is None else [b for b, (s, o) in enumerate(zip(realigned.lifted.score, own_scores)) if int(s) < int(o)]
    print("planted run, noisy %s: %d reads with a site in their window, %d tagged, least delta %s, neither %d -> %d, lower scores at %s"
          % (noisy, sum(in_window), sum(v != 0 for v in realigned.hp), min([d for d in realigned.delta if d] or [None]),
             sum(o[2] for o in before["observed"]), sum(o[2] for o in after["observed"]), lower))      # every figure before it is asserted
    assert sum(in_window) == DECIDED
    assert [v != 0 for v in realigned.hp] == in_window and list(realigned.hp) == list(host["tags"].hp)
    assert [d == 0 for d in realigned.delta] == [not w for w in in_window]
    assert min(d for d, w in zip(realigned.delta, in_window) if w) == MIN_DELTA
    n_before, n_after = sum(o[2] for o in before["observed"]), sum(o[2] for o in after["observed"])
    assert n_after == NEITHER_AFTER[noisy] and n_before > n_after and (n_before == NEITHER_BEFORE[noisy] or not exact)
    for name in ("alleles", "flags", "ins_copies", "ins_len"):
        assert np.array_equal(getattr(before["calls"], name), getattr(after["calls"], name)), name
    assert not (np.asarray(after["calls"].gq)[host["sites"].pos] < np.asarray(before["calls"].gq)[host["sites"].pos]).any()
    if own_scores is not None and exact:
        assert len(lower) == LOWER_SCORE[noisy] and all(int(s) <= int(o) for s, o in zip(realigned.lifted.score, own_scores))
