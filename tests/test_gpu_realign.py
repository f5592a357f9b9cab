"""GPU: haplotype_calls / haplotype_windows / lift_alignment / realign (csrc/wn_realign.hip through wavenet_speech_amd/realign.py)
against the reference of tests/realign_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality;
tests/test_realign_ref.py holds the reference itself on the CPU, and the shared inputs are built once in tests/realign_cases.py.
The quadratic host aligner is never run here: where an alignment is needed the reference is fed with the device's own
pairwise_align rows.  Every shape is tiny but one: T = 256 positions, columns or slots is the tile of both kernels."""
import types

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import pairwise_align_ref as A
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import realign_cases as RC
from tests import realign_ref as RR
from tests.gpu_calls import assert_evidence as _assert_evidence, assert_genotypes as _assert_genotypes, assert_pile as _assert_pile, capture as _capture
from tests.gpu_util import DEV, assert_equal_arrays as _assert_equal, dev as _dev, i32 as _i32, no_stale_flags, strided as _strided, u8 as _u8  # noqa: F401

pytestmark = pytest.mark.gpu
T = 256
WINDOW_FIELDS = (("labels", torch.int32), ("lengths", torch.int32), ("ops", torch.uint8), ("ops_len", torch.int32), ("used", torch.int8))
LIFT_FIELDS = ("matches", "mismatches", "gaps", "length", "ops_len")


def _reported(what, text, n):
    """the bad rows of the last call are reported once, in the function's name"""
    if n:
        with pytest.raises(RuntimeError, match="wavenet_speech_amd.%s: %d %s" % (what, n, text)):
            W.check_device_flags()
    W.check_device_flags()


def _hcalls_dev(hc):
    return W.HaplotypeCalls(_u8(hc.call), _u8(hc.ins_len), _u8(hc.ins_bases))


def _assert_rows(got, want, what):
    """a device tensor against the reference's rows, which may be narrower or wider: equal where both have columns, zero beyond"""
    got, want = got.cpu().numpy(), np.asarray(want)
    w = min(got.shape[-1], want.shape[-1])
    _assert_equal(got[..., :w], want[..., :w], what)
    assert not got[..., w:].any() and not want[..., w:].any(), "%s: columns beyond %d" % (what, w)


def _windows_both(hc, reference, lo, n, strand, cap):
    """every field must equal the reference's exactly, the zeros behind the lengths included -> (HaplotypeWindows, reference Windows)"""
    want = RR.haplotype_windows_ref(hc, reference, lo, n, strand, cap)
    got = W.haplotype_windows(_hcalls_dev(hc), _i32(reference), _i32(lo), _i32(n), _i32(strand), max_hap_ops=cap)
    _reported("haplotype_windows", "read\\(s\\) whose window does not fit", want.bad)
    for name, dtype in WINDOW_FIELDS:
        assert getattr(got, name).dtype == dtype, name
        _assert_equal(getattr(got, name).cpu().numpy(), getattr(want, name), name)
    return got, want


def _assert_lifted(got, want, what=""):
    """a PairwiseAlignment of lift_alignment against the reference's Lifted: ops with their zero tails, counts, and the score in half units"""
    assert got.ops.dtype == torch.uint8 and got.score.dtype == torch.float32 and all(getattr(got, n).dtype == torch.int32 for n in LIFT_FIELDS)
    _assert_rows(got.ops, want.ops, what + "ops")
    for name in LIFT_FIELDS:
        _assert_equal(getattr(got, name).cpu().numpy().astype(np.int64), np.asarray(getattr(want, name), dtype=np.int64), what + name)
    _assert_equal((got.score.cpu().numpy().astype(np.float64) * 2).astype(np.int64), np.asarray(want.score, dtype=np.int64), what + "score")


def _lift_both(args, max_ops, views=False, costs=A.EMBOSS, free=True):
    """RC.pair_batch's arguments through the reference and the kernel -> (PairwiseAlignment, reference Lifted)"""
    a_ops, a_len, windows, pick, ref, ref_len, read, read_len = args
    want = RR.lift_ref(*args, max_ops=max_ops, costs=costs, free=free)
    place = (lambda a: _strided(a, False)) if views else _dev
    alignments = [W.PairwiseAlignment(None, None, None, None, None, place(a_ops[h]), _i32(a_len[h])) for h in range(len(a_ops))]
    hap_ops = _u8(windows.ops)
    if views:
        wide = torch.zeros(hap_ops.shape[0], hap_ops.shape[1], hap_ops.shape[2] + 5, dtype=torch.uint8, device=DEV)
        wide[:, :, 2:2 + hap_ops.shape[2]] = hap_ops
        hap_ops = wide[:, :, 2:2 + hap_ops.shape[2]]
    win = W.HaplotypeWindows(None, _i32(windows.lengths), hap_ops, _i32(windows.ops_len), _dev(windows.used))
    got = W.lift_alignment(alignments, win, _i32(pick), place(ref), _i32(ref_len), place(read), _i32(read_len), match=costs[0] / 2, mismatch=costs[1] / 2,
                           gap_open=costs[2] / 2, gap_extend=costs[3] / 2, end_gaps_free=free, max_ops=max_ops)
    _reported("lift_alignment", "read\\(s\\) whose rows do not compose", want.bad)
    _assert_lifted(got, want)
    return got, want


# ---- haplotype_windows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 2])
def test_windows_at_the_tile_edges_on_both_strands(H):
    rng = np.random.default_rng(11 + H)
    R = 2 * T + 88
    edges = (0, 1, T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, R - 2 * T - 1, R - T - 1, R - T, R - 2, R - 1)
    reference, hc = RC.random_calls(rng, R, H=H, deleted=edges[::2] + (R - 1,), inserted=edges[1::2] + (0, R - 1))
    sizes = (1, T - 1, T, T + 1, 2 * T + 1)
    lo = [0 if at_start else R - n for n in sizes for at_start in (True, False)] + [7, 300]      # windows at 0, windows that end at R, two inside
    n = [n for n in sizes for _ in (0, 1)] + [T, 40]
    for strand in ([0] * len(lo), [1] * len(lo), [b & 1 for b in range(len(lo))]):
        got, want = _windows_both(hc, reference, lo, n, strand, (2 * T + 1) * 4)
        assert want.used.tolist() == [1] * len(lo) and want.ops_len.max() > 2 * T + 1 > want.lengths.min() >= 0
    assert (want.ops == 3).any() and (want.ops == 4).any() and (want.ops == 2).any() and (want.labels == 7).any()
    # capacity exactly at the need, and one below: the widest read is bad on every haplotype, its neighbours are written
    need = int(want.ops_len.max())
    got, at = _windows_both(hc, reference, lo, n, strand, need)
    assert at.used.tolist() == [1] * len(lo)
    got, below = _windows_both(hc, reference, lo, n, strand, need - 1)
    widest = [b for b in range(len(lo)) if want.ops_len[:, b].max() == need]
    assert below.used.tolist() == [-1 if b in widest else 1 for b in range(len(lo))] and below.bad == len(widest) >= 1
    assert not below.lengths[:, widest].any() and not got.labels[:, widest].any().item()


def test_windows_by_hand_and_without_insertions():
    hc = RC.window_calls()
    got, want = _windows_both(hc, RC.WINDOW_REF, [0, 0, 0, 6, 6, 3], [12, 12, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1], 16)
    assert got.labels[0, 1, :14].tolist() == [1, 2, 3, 4, 1, 7, 4, 4, 2, 7, 2, 1, 2, 4]             # the values of tests/test_realign_ref.py
    assert got.ops[0, 1].tolist() == [1, 1, 1, 1, 1, 4, 4, 4, 1, 1, 3, 3, 1, 2, 4, 1] and got.ops_len[0, 5].item() == 2 and got.lengths[0, 5].item() == 0
    bare = RR.HapCalls(hc.call, np.zeros_like(hc.ins_len), hc.ins_bases[:, :, :0])                    # max_ins 0: no ins_bases at all
    _windows_both(bare, RC.WINDOW_REF, [0, 2], [12, 9], [1, 0], 12)
    flat = RR.HapCalls(np.array([[1, 2, 3, 4] * 8], dtype=np.uint8), np.zeros((1, 32), dtype=np.uint8), np.zeros((1, 32, 1), dtype=np.uint8))
    got = W.haplotype_windows(_hcalls_dev(flat), [1, 2, 3, 4] * 8, [3], [20], [1])                   # lists, and the default capacity R * (1 + max_ins)
    assert tuple(got.labels.shape) == (1, 1, 64) and got.ops[0, 0, :20].tolist() == [1] * 20 and got.lengths.tolist() == [[20]]
    W.check_device_flags()


def test_skipped_reads_beside_bad_ones():
    rng = np.random.default_rng(4)
    reference, hc = RC.random_calls(rng, 300, inserted=(10,))
    over = RR.HapCalls(hc.call, hc.ins_len, hc.ins_bases[:, :, :2])                                   # max_ins 2 beside ins_len 3 at position 10
    #        skipped: unmapped (with a window that would be bad), ref_lengths 0 | bad: strand, lo, the end, a negative length | good | ins_len above max_ins
    lo = [-5, 0, 0, -1, 200, 20, 40, 0, 10, 11]
    n = [400, 0, 50, 50, 101, -3, 60, 300, 1, 50]
    strand = [-1, 1, 2, 0, 1, 0, 1, 0, 0, 1]
    got, want = _windows_both(hc, reference, lo, n, strand, 1200)
    assert want.used.tolist() == [0, 0, -1, -1, -1, -1, 1, 1, 1, 1] and want.bad == 4
    got, want = _windows_both(over, reference, lo, n, strand, 1200)
    assert want.used.tolist() == [0, 0, -1, -1, -1, -1, 1, -1, -1, 1] and want.bad == 6                # checked at the window's last position too


# ---- lift_alignment, on hand-given and random valid rows: no aligner ----------------------------------------------------------------

def test_the_composition_by_hand_and_every_bad_row_between_valid_rows():
    good, bad = [r[1:5] for r in RC.LIFT_ROWS], [r[1:] for r in RC.LIFT_BAD]
    pairs = [p for pair in zip(good, bad) for p in pair] + good[len(bad):]
    for H, pick in ((1, None), (2, [b % 2 for b in range(len(pairs))]), (2, [(b // 2) % 2 for b in range(len(pairs))])):
        got, want = _lift_both(RC.pair_batch(pairs, pick, H=H), 8)
        assert want.bad == len(bad) and [n == 0 for n in want.ops_len.tolist()[:2 * len(bad)]] == [False, True] * len(bad)
    for b, r in enumerate(RC.LIFT_ROWS[:len(bad)]):
        assert got.ops[2 * b, :len(r[5])].tolist() == r[5], r[0]
    args = RC.pair_batch(pairs, [b % 2 for b in range(len(pairs))], H=2)
    _lift_both(args, 8, views=True)                                                                   # rows as views into wider tensors
    _lift_both(args, 8, costs=(4, -6, 9, 3), free=False)                                              # the end runs cost too
    _lift_both(args, 8, costs=(1, -1, 2, 0))
    got, want = _lift_both(args, 5)                                                                   # one valid row needs 6 columns
    assert want.bad == len(bad) + 1
    # a pick outside [0, H), a bad window and a skipped one, each once
    used = np.ones(len(pairs), dtype=np.int8)
    used[0], used[2] = 0, -1
    pick = [b % 2 for b in range(len(pairs))]
    pick[4], pick[6] = 2, -1
    got, want = _lift_both(args[:2] + (args[2]._replace(used=used), pick) + args[4:], 8)
    assert want.bad == len(bad) + 3 and want.score[0] == 0 and want.score[2] == RR.POISON and want.ops_len[4] == want.ops_len[6] == 0


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1, 4 * T + 1])
def test_random_valid_rows_at_the_tile_edges(n):
    rng = np.random.default_rng(n)
    pairs = [RC.random_pair(rng, n) for _ in range(3)]
    pairs.append(RC.random_pair(rng, n, p=(0.1, 0.1, 0.7, 0.1), extra=0.6))                           # long runs of 3s and of 4s
    pairs.append(RC.random_pair(rng, n, p=(0.05, 0.05, 0.1, 0.8), extra=0.05))                        # a haplotype far longer than the window
    a = [3] * n                                                                                       # the slots themselves at the tile edge: n haplotype labels
    pairs.append((a, [4] * (n - 1) + [1], [2], []))                                                   # an empty read; one column survives
    pairs.append(([4] * n, [3] * n, [1] * n, [2] * n))                                                # an empty haplotype: n 3s, then n 4s
    widest = max(len(p[2]) + len(p[3]) for p in pairs)
    got, want = _lift_both(RC.pair_batch(pairs, [b % 2 for b in range(len(pairs))], H=2), widest, views=n == T + 1)
    assert want.bad == 0 and want.length.max() > n and want.ops_len[-2] == 1 and want.ops_len[-1] == 2 * n
    for b, p in enumerate(pairs):
        assert A.replay(p[2], p[3], want.ops[b][:want.ops_len[b]]) == (p[2], p[3])


def test_a_run_of_778_reference_labels_across_tiles():
    rng = np.random.default_rng(778)
    hh = [1] * 250 + [3] * 778 + [2] * 3 + [4] * 300 + [1] * 5 + [3] * 700
    a = [1] * 100 + [4] * 600 + [int(v) for v in rng.choice([1, 2, 3], size=458)] + [4] * 290
    ref = [int(v) for v in rng.integers(1, 4, size=sum(v != 4 for v in hh))]
    read = [int(v) for v in rng.integers(1, 4, size=sum(v != 3 for v in a))]
    assert sum(v != 4 for v in a) == sum(v != 3 for v in hh) == 558
    got, want = _lift_both(RC.pair_batch([(a, hh, ref, read), RC.random_pair(rng, 40)]), len(ref) + len(read))
    row = want.ops[0][:want.ops_len[0]].tolist()
    # 250 shared columns and the 600 4s before haplotype label 100, then the run; in the last slot the 3s come before the 4s
    assert want.bad == 0 and row[100:700] == [4] * 600 and row[850:850 + 778] == [3] * 778 and row[-990:] == [3] * 700 + [4] * 290


def test_one_row_at_the_haplotype_and_query_limits():
    rng = np.random.default_rng(65535)
    L, M = 65535, 8192
    a = np.full(L, 3, dtype=np.uint8)
    a[rng.choice(L, size=M, replace=False)] = 1
    hh = np.where(rng.random(L) < 0.9, 1, 4).astype(np.uint8)                                         # every column holds a haplotype label
    ref = [int(v) for v in rng.integers(1, 4, size=int((hh == 1).sum()))]
    read = [int(v) for v in rng.integers(1, 4, size=M)]
    got, want = _lift_both(RC.pair_batch([(a.tolist(), hh.tolist(), ref, read), RC.random_pair(rng, 30)]), L + M)
    assert want.bad == 0 and want.ops_len[0] == len(ref) + M - int(((a == 1) & (hh == 1)).sum()) > L - M and want.matches[0] > 1000


# ---- realign: the steps together ----------------------------------------------------------------------------------------------------

def _steps(hcalls, reference, lo, ref_len, strand, labels, lengths, cap):
    """haplotype_windows and pairwise_align once per haplotype: what realign runs before it lifts, for the device's own rows"""
    windows = W.haplotype_windows(hcalls, reference, lo, ref_len, strand, max_hap_ops=cap)
    return windows, [W.pairwise_align(windows.labels[h], windows.lengths[h], labels, lengths) for h in range(int(windows.ops.shape[0]))]


def _assert_realigned(r, hc, reference, lo, n, strand, reads, refs, windows, alignments, what=""):
    """a Realignment against the reference fed with the device's own rows of the reads against the haplotypes -> the reference's"""
    rows = [a.ops.cpu().numpy() for a in alignments]
    lens = [a.ops_len.cpu().tolist() for a in alignments]
    want = RR.realign_ref(refs, n, reads, lo, strand, hc, reference, align=lambda h, b, hap, read: rows[h][b][:lens[h][b]])
    for name, _ in WINDOW_FIELDS:
        _assert_rows(getattr(windows, name), getattr(want.windows, name), what + "windows." + name)
    for h, a in enumerate(alignments):                                                               # the scores are the rows' own
        assert (a.score.cpu().numpy() * 2).astype(np.int64).tolist() == [s[h] for s in want.scores], what + "scores"
    assert r.pick.dtype == torch.int32 and r.hp.dtype == torch.uint8 and r.delta.dtype == r.scores.dtype == torch.float32
    assert r.pick.cpu().tolist() == want.pick and r.hp.cpu().tolist() == want.hp, what + "pick, hp"
    assert (r.delta.cpu().numpy() * 2).astype(np.int64).tolist() == want.delta and (r.scores.cpu().numpy() * 2).astype(np.int64).tolist() == want.scores
    _assert_lifted(r.alignment, want.lifted, what)
    return want


def _small_batches():
    """two batches of 8 reads drawn from random haplotypes over one reference, of equal shapes: host lists and device tensors"""
    rng = np.random.default_rng(2)
    reference, hc = RC.random_calls(rng, 400, max_ins=2, rate=0.04)
    out = []
    for _ in range(2):
        spans = [(int(rng.integers(0, 320)), int(rng.integers(30, 80)), b & 1, (b >> 1) & 1) for b in range(8)]
        spans[0], spans[1] = (0, 70, 0, 0), (330, 70, 1, 1)                                         # windows at 0 and at R
        reads, refs = RC.drawn_reads(rng, reference, hc, spans)
        out.append(dict(lo=[s[0] for s in spans], n=[s[1] for s in spans], strand=[s[2] for s in spans], reads=reads, refs=refs,
                        ref_rows=C.rows(refs, width=80)[0], labels=C.rows(reads, width=160)[0], lengths=[len(r) for r in reads]))
    return reference, hc, out


def _tensors_of(result):
    return [result.pick, result.hp, result.delta, result.scores] + [t for t in result.alignment]


def test_two_identical_runs_and_one_graph_replayed_on_a_second_batch():
    reference, hc, batches = _small_batches()
    hcalls, ref_dev = _hcalls_dev(hc), _i32(reference)
    static = {k: _i32(batches[0][k]) for k in ("lo", "n", "strand", "ref_rows", "labels", "lengths")}

    def fill(batch):
        for k, t in static.items():
            t.copy_(torch.from_numpy(np.asarray(batch[k], dtype=np.int32)))

    def step():
        return W.realign(static["ref_rows"], static["n"], static["labels"], static["lengths"], static["lo"], static["strand"], hcalls, ref_dev)

    eager = []
    for k, batch in enumerate(batches):
        fill(batch)
        r = step()
        windows, alignments = _steps(hcalls, ref_dev, static["lo"], static["n"], static["strand"], static["labels"], static["lengths"], 80 * 3)
        want = _assert_realigned(r, hc, reference, batch["lo"], batch["n"], batch["strand"], batch["reads"], batch["refs"], windows, alignments, "batch %d " % k)
        assert want.lifted.bad == 0 and set(want.hp) >= {1, 2} and any(4 in row for row in want.lifted.ops.tolist())
        again = step()
        assert all(torch.equal(u, v) for u, v in zip(_tensors_of(r), _tensors_of(again))), "two runs differ"      # bitwise
        eager.append([t.clone() for t in _tensors_of(r)])
    assert not all(torch.equal(u, v) for u, v in zip(*eager))
    fill(batches[0])
    graph, captured = _capture(step)                                                                 # windows, pairwise_align twice, pick, lift: one graph
    for k, batch in enumerate(batches):
        fill(batch)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(_tensors_of(captured), eager[k])), "replay %d" % k
    W.check_device_flags()


def test_one_haplotype_from_a_consensus():
    """a polishing round: reads against the one haplotype of call_consensus, lifted back; every pick is 0 and no read is tagged"""
    reference, hc, batches = _small_batches()
    one = RR.HapCalls(hc.call[:1], hc.ins_len[:1], hc.ins_bases[:1])
    batch = batches[0]
    calls = W.ConsensusCalls(_u8(one.call[0]), _u8(one.ins_len[0]), _u8(one.ins_bases[0]), None, None, None, None)
    hcalls = W.haplotype_calls(calls)
    args = [_i32(batch[k]) for k in ("lo", "n", "strand", "labels", "lengths", "ref_rows")]
    r = W.realign(args[5], args[1], args[3], args[4], args[0], args[2], hcalls, _i32(reference))
    windows, alignments = _steps(hcalls, _i32(reference), args[0], args[1], args[2], args[3], args[4], 80 * 3)
    want = _assert_realigned(r, one, reference, batch["lo"], batch["n"], batch["strand"], batch["reads"], batch["refs"], windows, alignments)
    assert want.pick == [0] * 8 and want.hp == [0] * 8 and want.delta == [0] * 8 and tuple(r.scores.shape) == (8, 1)
    W.check_device_flags()


# ---- the closed loop on the planted runs --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "planted_windows"])
@pytest.mark.parametrize("noisy", [False, True])
def test_closed_loop_on_the_planted_phased_runs(noisy, mapped):
    """map -> pairwise_align -> left_align -> pileup + pileup_evidence -> call_genotypes -> phase -> haplotype_calls -> realign ->
    left_align -> pileup + pileup_evidence -> call_genotypes.  Every table equals the reference fed with the device's rows, and the
    conditions of tests/realign_cases.py hold on the device's tables.  Two of their figures belong to the windows: the observations
    that show neither allele BEFORE realignment, and the reads whose lifted score is lower.  On the planted windows (mapped False)
    they are the host chain's, 3 -> 0 and 17 -> 8, 3 and 6 reads, and are asserted; on the windows map_reads returns, which differ
    from the planted ones by a few bases at the ends of some reads, the device shows 4 -> 0 and 18 -> 8, 4 and 8 reads: there the
    figure AFTER realignment is asserted (0 and 8, the host's) and that it fell."""
    run = PC.planted(noisy)
    labels, lengths, qual = _dev(run["labels"]), _dev(run["lengths"]), _dev(run["qual"])
    index = W.read_index(_i32(run["ref"]), k=11, w=5)
    if mapped:
        m = W.map_reads(labels, lengths, index)
        lo, _ = m.window(C.PLANT_FLANK)
        ref_rows, ref_len = m.labels(C.PLANT_FLANK)
        strand = m.strand
        assert strand.cpu().tolist() == run["strand"]
    else:
        lo, ref_len, strand = _i32([v[0] for v in run["window"]]), _i32([v[1] for v in run["window"]]), _i32(run["strand"])
        ref_rows = _dev(C.rows(RC.windows_of(run)[2])[0])
    w = W.genotype_weights(K.SCALE)

    def tables(alignment):
        aln = W.left_align(alignment, ref_rows, ref_len, labels, lengths, strand).alignment
        reads = (aln, lo, ref_len, strand, labels, lengths)
        pile = W.pileup(*reads, index.R, qual=qual, min_qual=PC.MIN_QUAL)
        ev = W.pileup_evidence(*reads, index.R, w, qual=qual, min_qual=PC.MIN_QUAL)
        return reads, pile, ev, W.call_genotypes(pile, ev, index, w)

    reads, pile, ev, calls = tables(W.pairwise_align(ref_rows, ref_len, labels, lengths))
    sites = W.phase_sites(calls)
    phasing = W.phase_chain(W.phase_links(*reads, sites, qual=qual, min_qual=PC.MIN_QUAL, reach=PC.REACH), sites)
    tags = W.haplotag(*reads, sites, phasing, qual=qual, min_qual=PC.MIN_QUAL)
    hcalls = W.haplotype_calls(calls, sites, phasing)
    r = W.realign(ref_rows, ref_len, labels, lengths, lo, strand, hcalls, index)
    cap = int(ref_rows.shape[1]) * (1 + int(hcalls.ins_bases.shape[2]))
    windows, alignments = _steps(hcalls, index, lo, ref_len, strand, labels, lengths, cap)
    reads2, pile2, ev2, calls2 = tables(r.alignment)
    W.check_device_flags()
    # the reference, fed with the device's calls, windows and rows
    host_sites = H.Sites(sites.pos.cpu().tolist(), [tuple(a) for a in sites.alleles.cpu().tolist()], sites.site_of.cpu().tolist())
    chain = H.Chain(*[t.cpu().tolist() for t in phasing])
    hc = RR.haplotype_calls_ref(G.Calls(*[None if t is None else t.cpu().numpy() for t in calls]), host_sites, chain)
    for name in ("call", "ins_len", "ins_bases"):
        assert getattr(hcalls, name).dtype == torch.uint8
        _assert_equal(getattr(hcalls, name).cpu().numpy(), getattr(hc, name), "hcalls." + name)
    lo_h, n_h = lo.cpu().tolist(), ref_len.cpu().tolist()
    refs = [row[:n].tolist() for row, n in zip(ref_rows.cpu().numpy(), n_h)]
    want = _assert_realigned(r, hc, run["ref"], lo_h, n_h, run["strand"], run["reads"], refs, windows, alignments)
    assert want.lifted.bad == 0 and want.windows.bad == 0
    before = RC.recall(run, reads[0].ops.cpu().numpy(), reads[0].ops_len.cpu().numpy(), lo_h, n_h, host_sites)
    after = RC.recall(run, reads2[0].ops.cpu().numpy(), reads2[0].ops_len.cpu().numpy(), lo_h, n_h, host_sites)
    for got_tables, host in (((pile, ev, calls), before), ((pile2, ev2, calls2), after)):       # every table equals the reference on the device's ops
        _assert_pile(got_tables[0], host["pile"])
        _assert_evidence(got_tables[1], host["evidence"])
        _assert_genotypes(got_tables[2], host["calls"])
    # the conditions, on the device's tables
    own = reads[0].ops.cpu().numpy()
    own_scores = [A.rescore(row[:k], *A.EMBOSS, True) for row, k in zip(own, reads[0].ops_len.cpu().tolist())]
    device = types.SimpleNamespace(hp=want.hp, delta=want.delta, lifted=want.lifted)              # equal to the device's: asserted above
    RC.check_conditions(run, dict(sites=host_sites, tags=types.SimpleNamespace(hp=tags.hp.cpu().tolist())), device, before, after, noisy,
                        own_scores=own_scores, windows=(lo_h, n_h), exact=not mapped)
