"""GPU: minimizers / read_index / seed_anchors / chain_anchors / map_reads (csrc/wn_readmap.hip through wavenet_speech_amd.readmap)
against the reference of tests/readmap_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality,
ties included; tests/test_readmap_ref.py holds the reference itself on the CPU, and the planted run is built once in
tests/readmap_cases.py.  Every shape is tiny."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import readmap_cases as C
from tests import readmap_ref as R
from tests.gpu_labels import INT_MIN, PAD, assert_index as _assert_index, assert_seeds as _assert_seeds
from tests.gpu_util import DEV, dev as _dev

pytestmark = pytest.mark.gpu


# ---- sketch -------------------------------------------------------------------------------------------------------------------

def _sketch_ref(seqs, k, w, width):
    code, flag = np.zeros((len(seqs), width), dtype=np.int64), np.zeros((len(seqs), width), dtype=np.uint8)
    for b, s in enumerate(seqs):
        for p, c, strand in R.minimizers_ref(s, k, w):
            code[b, p], flag[b, p] = c, 1 + strand
    return code, flag


def _assert_sketch(got, seqs, k, w, width):
    code, flag = _sketch_ref(seqs, k, w, width)
    assert got.code.dtype == torch.int32 and got.flag.dtype == torch.uint8 and tuple(got.code.shape) == (len(seqs), width)
    assert np.array_equal(got.flag.cpu().numpy(), flag)
    assert np.array_equal(got.code.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, code)


def _edge_sequences(k, w):
    rng = np.random.default_rng(100 * k + w)
    rnd = lambda n: C.random_bases(rng, n)
    broken = rnd(90)
    broken[20], broken[55] = 0, 5                                    # each break invalidates exactly k k-mers
    seqs = [rnd(130), broken, [1, 4] * 40, [2, 3] * 40 + [1],        # ATAT.. and GCGC..: every even k-mer is a palindrome
            [1] * 70, [4] * 70,                                      # homopolymers: all hashes equal, ties to the smallest position
            rnd(max(k - 1, 0)), rnd(k), [],                          # shorter than k, exactly one k-mer, empty
            rnd(k - 1 + w - 1), rnd(k - 1 + w), rnd(k - 1 + w + 1)]  # n_k = w - 1, w, w + 1
    return seqs


@pytest.mark.parametrize("k,w", [(1, 1), (1, 64), (2, 3), (15, 10), (16, 1), (16, 64), (7, 64)])
def test_sketch_edges(k, w):
    seqs = _edge_sequences(k, w)
    labels, lengths = C.rows(seqs)
    _assert_sketch(W.minimizers(_dev(labels), _dev(lengths), k=k, w=w), seqs, k, w, labels.shape[1])
    W.check_device_flags()


def test_sketch_breaks_and_homopolymer_by_hand():
    """a break invalidates exactly k k-mers (w = 1: every valid k-mer is a minimizer); a homopolymer's minimizers are the window starts"""
    labels = _dev(np.array([[1, 1, 2, 0, 2, 1, 1, 0, 0], [1] * 9], dtype=np.int32))
    got = W.minimizers(labels, [7, 9], k=2, w=1)
    assert got.flag[0].tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 0]
    got = W.minimizers(labels, [7, 9], k=3, w=4)
    assert got.flag[1].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0] and got.code[1].tolist() == [0] * 9
    pos, codes, strands, counts = W.minimizers(labels, [7, 9], k=2, w=1).compact()
    assert counts.tolist() == [4, 8] and pos[0].tolist() == [0, 1, 4, 5, -1, -1, -1, -1] and codes[0, :4].tolist() == [0, 1, 4, 0]
    assert strands[0, :4].tolist() == [0, 0, 0, 0]
    W.check_device_flags()


def test_sketch_poisoned_lengths():
    seqs = [C.random_bases(np.random.default_rng(3), 60)] * 3
    labels, _ = C.rows(seqs)
    W.check_device_flags()
    got = W.minimizers(_dev(labels), [60, -1, 61], k=5, w=4)
    code, flag = _sketch_ref([seqs[0], [], []], 5, 4, 60)
    assert np.array_equal(got.flag.cpu().numpy(), flag)
    with pytest.raises(RuntimeError, match="2 row\\(s\\) with a length outside \\[0, 60\\]"):
        W.check_device_flags()
    W.check_device_flags()


def test_sketch_forms_of_the_rows():
    """strided rows are read in place; int64 labels; a list of lengths"""
    rng = np.random.default_rng(4)
    seqs = [C.random_bases(rng, n) for n in (77, 120, 5)]
    labels, lengths = C.rows(seqs)
    B, L = labels.shape
    wide = torch.full((B, L + 7), 2, dtype=torch.int32, device=DEV)
    wide[:, :L] = _dev(labels)
    view = wide[:, :L]
    assert not view.is_contiguous()
    for lab, n in ((view, _dev(lengths)), (_dev(labels).long(), _dev(lengths).long()), (_dev(labels), lengths.tolist())):
        _assert_sketch(W.minimizers(lab, n, k=6, w=5), seqs, 6, 5, L)
    W.check_device_flags()


def test_sketch_seams():
    """no output depends on the chunk: 3000 bases at chunk 64, 256 and the library's own; lengths around every chunk size"""
    rng = np.random.default_rng(5)
    long = C.random_bases(rng, 3000)
    long[1023:1026] = [0, 1, 0]
    seqs = [long] + [long[:n] for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)]
    labels, lengths = C.rows(seqs)
    code, flag = _sketch_ref(seqs, 15, 10, 3000)
    for chunk in (64, 256, None, 2048, 1):
        got = W.minimizers(_dev(labels), _dev(lengths), chunk=chunk)
        assert np.array_equal(got.flag.cpu().numpy(), flag), chunk
        assert np.array_equal(got.code.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, code), chunk
    wide = [long[:n] for n in (300, 63, 64, 65)]                     # the widest window: a halo of 63 + 8 on either side of a chunk
    labels, lengths = C.rows(wide)
    for chunk in (64, None):
        _assert_sketch(W.minimizers(_dev(labels), _dev(lengths), k=9, w=64, chunk=chunk), wide, 9, 64, 300)
    W.check_device_flags()


# ---- seeds --------------------------------------------------------------------------------------------------------------------

def test_seeds_max_occ_on_both_sides():
    """a k-mer with exactly max_occ entries in the index is kept, one with max_occ + 1 is dropped whole (w = 1: every valid k-mer is a
    minimizer; the copies are separated by breaks)"""
    x, y = [1, 2, 3, 1, 1, 4], [2, 2, 1, 4, 3, 1]
    ref = (x + [0]) * 3 + (y + [0]) * 4 + [1, 3, 3, 2, 4, 4, 1]
    got, want = _assert_seeds(ref, [x, y, x + y, R.revcomp(y + x)], 6, 1, 3, 16)
    assert [n for n, _, _ in want] == [3, 0, 3, 3] and got.strand[3, :4].tolist() == [1, 1, 1, -1]
    got, want = _assert_seeds(ref, [x, y, x + y], 6, 1, 4, 16)
    assert [n for n, _, _ in want][:2] == [3, 4]
    got, want = _assert_seeds(ref, [x, y], 6, 1, 2, 16)
    assert [n for n, _, _ in want] == [0, 0] and got.keys.eq(PAD).all()
    W.check_device_flags()


def test_seeds_cap_on_both_sides_and_the_kept_prefix():
    rng = np.random.default_rng(6)
    unit = C.random_bases(rng, 40)
    ref = unit + [0] + unit + [0] + C.random_bases(rng, 50)
    read = unit[3:38]
    total = len(R.anchors_ref(read, R.index_ref(ref, 5, 2), 5, 2, 8, 32768)[0])
    assert total > 8
    for cap, trunc in ((total, 0), (total - 1, 1), (total + 1, 0), (1, 1)):
        got, want = _assert_seeds(ref, [read, R.revcomp(read)], 5, 2, 8, cap)
        assert want[0] == (min(cap, total), want[0][1], trunc)
    W.check_device_flags()


def test_seeds_no_hit_and_the_reverse_strand_ends():
    """a read without a hit is the unmapped row; a reverse-strand read has anchors at q = 0 (q' = n - k) and at q = n - k (q' = 0)"""
    rng = np.random.default_rng(8)
    ref = C.random_bases(rng, 300)
    other = C.random_bases(np.random.default_rng(9), 80)
    rev = R.revcomp(ref[100:160])
    got, want = _assert_seeds(ref, [other, rev, ref[100:160], [], ref[:7]], 12, 1, 8, 64, width=90)
    assert want[0][0] == 0 and want[3] == (0, 0, 0) and want[4] == (0, 0, 0)
    n, k = 60, 12
    assert got.strand[1, :want[1][0]].eq(1).all() and got.query_pos[1, 0] == 0 and got.query_pos[1, want[1][0] - 1] == n - k
    assert got.ref_pos[1, 0] == 100 and got.ref_pos[1, want[1][0] - 1] == 160 - k and got.strand[2, :want[2][0]].eq(0).all()
    m = W.chain_anchors(got)
    assert [t[0].item() for t in m[:8]] == [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN] and m.mapped.tolist() == [False, True, True, False, False]
    assert [t[1].item() for t in m[1:6]] == [1, 100, 160, 0, 60] and [t[2].item() for t in m[1:6]] == [0, 100, 160, 0, 60]
    W.check_device_flags()


def test_seeds_many_tiles_and_an_empty_index():
    """reads longer than one tile of 256 positions, hits in every tile; an index without entries"""
    rng = np.random.default_rng(10)
    ref = C.random_bases(rng, 1500)
    reads = [C.mutate(rng, ref[200:1100], 0.05), R.revcomp(C.mutate(rng, ref[600:1400], 0.05)), ref[:257], ref[1000:1256]]
    _assert_seeds(ref, reads, 7, 3, 8, 2048)
    # thousands of anchors per read (short k-mers, every one a minimizer): the in-kernel sort over several exchanges per thread, of a
    # count that is no power of two, and of a truncated prefix
    dense = [C.random_bases(rng, 700), R.revcomp(ref[:650])]
    got, want = _assert_seeds(ref[:600], dense, 4, 1, 8, 4096)
    assert all(1024 < n < 4096 and n & (n - 1) for n, _, _ in want)
    got, want = _assert_seeds(ref[:600], dense, 4, 1, 8, 1000)
    assert [(n, t) for n, _, t in want] == [(1000, 1), (1000, 1)]
    _assert_seeds([1, 4] * 10, [[1, 4, 1, 4, 1, 4]], 4, 2, 8, 4)                      # palindromes only: nothing to index
    W.check_device_flags()


# ---- chain --------------------------------------------------------------------------------------------------------------------

def _assert_chain(reads, lengths, k, want_pred=True, **kw):
    """reads: per read a list of (s, r, q') in any order"""
    cap = max(1, max(len(r) for r in reads))
    rows = np.zeros((len(reads), cap, 3), dtype=np.int64)
    for b, r in enumerate(reads):
        rows[b, :len(r)] = np.array(r, dtype=np.int64).reshape(-1, 3)
    anchors = W.Anchors.from_table(rows, [len(r) for r in reads], lengths, k, device=DEV)
    got = W.chain_anchors(anchors, want_pred=want_pred, **kw)
    want = [R.chain_ref(sorted(r), n, k, **kw) for r, n in zip(reads, lengths)]
    table = torch.stack(list(got[:8]), dim=1).cpu().numpy()
    assert all(t.dtype == torch.int32 for t in got[:8]) and np.array_equal(table, C.result_rows(want)), (table, C.result_rows(want))
    if want_pred:
        for b, r in enumerate(want):
            n = len(r["f"])
            assert got.f[b, :n].tolist() == r["f"] and got.pred[b, :n].tolist() == r["pred"], b
            assert got.f[b, n:].eq(INT_MIN).all() and got.pred[b, n:].eq(-1).all()
    else:
        assert got.f is None and got.pred is None
    return got, want


def test_chain_worked_by_hand():
    rows = [(0, 10, 2), (0, 14, 6), (0, 19, 10), (0, 40, 3)]
    got, _ = _assert_chain([rows, [(1, r, q) for _, r, q in rows], [], [(0, 30, 7)], [(0, 30, 7), (1, 3, 1)]], [50] * 5, 4,
                           h=64, max_dist=100, bandwidth=10, gap_base=2, gap_log=8)
    table = torch.stack(list(got[:8]), dim=1).tolist()
    assert table[0] == [190, 0, 10, 23, 2, 14, 3, 64] and table[1] == [190, 1, 10, 23, 36, 48, 3, 64]
    assert table[2] == [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN]                      # no anchors
    assert table[3] == [64, 0, 30, 34, 7, 11, 1, INT_MIN]                             # one anchor: no runner-up
    assert table[4] == [64, 0, 30, 34, 7, 11, 1, 64]                                  # equal best on both strands: forward
    assert got.f[0, :4].tolist() == [64, 128, 190, 64] and got.pred[0, :4].tolist() == [-1, 0, 1, -1]
    W.check_device_flags()


def _reach(d):
    """d + 1 anchors: the last chains to the first and to nothing else, and the first is d positions before it"""
    return [(0, 0, 0)] + [(0, 1 + t, 10000 - t) for t in range(d - 1)] + [(0, d + 10, 20)]


@pytest.mark.parametrize("h", [1, 64, 130])
def test_chain_window_of_predecessors(h):
    """the predecessor i - h is reachable, i - h - 1 is not: 63, 64 and 65 predecessors at h = 64 (one round of lanes and the first
    of the next), 129, 130, 131 at h = 130 (the third round); and dense colinear anchors where every window is full"""
    ds = [1, 2, 63, 64, 65, 129, 130, 131]
    got, want = _assert_chain([_reach(d) for d in ds], [20000] * len(ds), 15, h=h, gap_base=0, gap_log=0)
    assert [w["pred"][-1] for w in want] == [0 if d <= h else -1 for d in ds]
    rng = np.random.default_rng(20 + h)
    dense = [sorted(set((int(s), int(r), int(q)) for s, r, q in zip(rng.integers(0, 2, 300), rng.integers(0, 400, 300), rng.integers(0, 400, 300))))
             for _ in range(3)]
    _assert_chain(dense, [500] * 3, 5, h=h, max_dist=60, bandwidth=25, gap_base=1, gap_log=3)
    W.check_device_flags()


def test_chain_limits_of_a_pair():
    """dr = 0 and dq <= 0 are excluded; max_dist and bandwidth on both sides; dd over the integer log"""
    kw = dict(h=64, max_dist=1000, bandwidth=300, gap_base=0, gap_log=0)
    pairs = {"dr0": [(0, 50, 5), (0, 50, 9)], "dq0": [(0, 50, 5), (0, 60, 5)], "dq<0": [(0, 50, 5), (0, 60, 4)],
             "dr=max": [(0, 0, 0), (0, 1000, 700)], "dr>max": [(0, 0, 0), (0, 1001, 701)],
             "dq=max": [(0, 0, 0), (0, 700, 1000)], "dq>max": [(0, 0, 0), (0, 701, 1001)],
             "dd=bw": [(0, 0, 0), (0, 400, 100)], "dd>bw": [(0, 0, 0), (0, 401, 100)], "dd=bw'": [(0, 0, 0), (0, 100, 400)], "dd>bw'": [(0, 0, 0), (0, 100, 401)]}
    names = list(pairs)
    got, want = _assert_chain([pairs[n] for n in names], [2000] * len(names), 15, **kw)
    assert [n for n, w in zip(names, want) if w["pred"][1] != 0] == ["dr0", "dq0", "dq<0", "dr>max", "dq>max", "dd>bw", "dd>bw'"]
    # the integer log: three anchors, the first two 480 together, the third dd off the diagonal on either side: 720 - (dd + 5 floor(log2 dd))
    dds = (0, 1, 2, 3, 4, 7, 8, 15, 16, 127, 128, 255, 256)
    reads = [[(1, 0, 0), (1, 100, 100), (1, 400 + dd, 400)] for dd in dds] + [[(0, 0, 0), (0, 100, 100), (0, 400, 400 + dd)] for dd in dds]
    got, want = _assert_chain(reads, [2000] * len(reads), 15, **dict(kw, gap_base=1, gap_log=5))
    assert [w["f"][2] for w in want[:5]] == [720, 719, 713, 712, 706] and [w["f"][2] for w in want[11:13]] == [720 - 255 - 35, 720 - 256 - 40]
    assert [w["f"][2] for w in want[13:]] == [w["f"][2] for w in want[:13]] and all(w["pred"] == [-1, 0, 1] for w in want)
    # the limits of the limits: 2^26 apart, the dearest gap; a candidate far below zero loses to the fresh start
    far = [[(0, 0, 0), (0, 2 ** 26 - 1, 1)], [(0, 0, 0), (0, 2 ** 26 - 1, 65535)], [(0, 5, 0), (0, 2 ** 25, 9), (0, 2 ** 25 + 9, 18)]]
    _assert_chain(far, [65535] * 3, 16, h=1024, max_dist=2 ** 26, bandwidth=2 ** 26, gap_base=1024, gap_log=1024)
    _assert_chain(far, [65535] * 3, 16, h=1024, max_dist=2 ** 26, bandwidth=2 ** 26, gap_base=0, gap_log=0)
    W.check_device_flags()


def test_chain_ties():
    free = dict(h=64, max_dist=100, bandwidth=10, gap_base=0, gap_log=0)
    # fresh = extension (gap_base = 16, dd = 1, min(dr, dq) = 1): the fresh start wins
    got, want = _assert_chain([[(0, 5, 5), (0, 7, 6)]], [50], 4, h=64, max_dist=100, bandwidth=10, gap_base=16, gap_log=0)
    assert want[0]["f"] == [64, 64] and want[0]["pred"] == [-1, -1] and got.ref_start.tolist() == [5] and got.runner_up.tolist() == [64]
    # two equal extensions: the larger j wins -- in one round of lanes, and across rounds (66 equal predecessors: the nearest is lane 0
    # of the first round; then with the nearest two worth less, min(dr, dq, k) = 2 and 3, so that the winner sits in lane 2)
    fan = [(0, t, 200 - t) for t in range(66)]
    got, want = _assert_chain([[(0, 1, 5), (0, 2, 4), (0, 9, 9)], fan + [(0, 100, 250)], fan + [(0, 67, 250)]], [300] * 3, 4,
                              **dict(free, h=128, max_dist=300, bandwidth=300))
    assert want[0]["pred"] == [-1, -1, 1] and want[1]["pred"][-1] == 65 and want[2]["pred"][-1] == 63 and got.n_anchors.tolist() == [2, 2, 2]
    # equal best within a strand: the smallest i; its runner-up equals the score.  On the reverse strand alone too
    got, want = _assert_chain([[(0, 30, 7), (0, 10, 9), (0, 20, 8)], [(1, 30, 7), (1, 10, 9)], [(0, 9, 9), (1, 3, 3), (1, 7, 7)]], [50] * 3, 4, **free)
    assert torch.stack(list(got[:8]), dim=1).tolist() == [[64, 0, 10, 14, 9, 13, 1, 64], [64, 1, 10, 14, 50 - 4 - 9, 50 - 9, 1, 64],
                                                         [128, 1, 3, 11, 50 - 4 - 7, 50 - 3, 2, 64]]
    W.check_device_flags()


def test_chain_runner_up():
    """the runner-up is the best anchor of another chain, wherever it sits: before, between and after the best chain's anchors, on the
    other strand; anchors of the best chain itself never count"""
    kw = dict(h=64, max_dist=100, bandwidth=10, gap_base=2, gap_log=8)
    a = [(0, 10, 10), (0, 15, 15), (0, 20, 20), (0, 25, 25)]                          # one chain: 64, 128, 192, 256
    b = [(0, 12, 40), (0, 17, 45), (0, 22, 50)]                                       # another between its anchors: 64, 128, 192
    c = [(1, 5, 5), (1, 9, 9)]
    got, want = _assert_chain([a, a + b, b + a[:2], a + c, c, a[:3] + b + [(0, 27, 55)]], [100] * 6, 4, **kw)
    assert got.score.tolist() == [256, 256, 192, 256, 128, 256] and got.runner_up.tolist() == [INT_MIN, 192, 128, 128, INT_MIN, 192]
    assert got.ref_start.tolist() == [10, 10, 12, 10, 5, 12] and got.n_anchors.tolist() == [4, 4, 3, 4, 2, 4]
    W.check_device_flags()


def test_chain_largest_row():
    """anchors_per_read = 32768 colinear anchors at k = 16 in one read, two bases apart: f = 16 * 16 + 32767 * 32, and the same row with
    want_pred off; a poisoned length and a poisoned count leave their reads unmapped and are counted"""
    n = 32768
    rows = np.zeros((3, n, 3), dtype=np.int64)
    rows[:, :, 1] = rows[:, :, 2] = 2 * np.arange(n)[None, :]
    anchors = W.Anchors.from_table(rows, [n, n, 5], [65535, 65535, 65535], 16, device=DEV)
    want = R.chain_ref([(0, 2 * i, 2 * i) for i in range(n)], 65535, 16, h=3)
    assert want["score"] == 256 + 32767 * 32 and want["n_anchors"] == n
    got = W.chain_anchors(anchors, h=3, want_pred=True)
    assert torch.stack(list(got[:8]), dim=1)[0].tolist() == [want[f] for f in C.FIELDS] == [256 + 32767 * 32, 0, 0, 65534 + 16, 0, 65534 + 16, n, INT_MIN]
    assert got.f[0].tolist() == want["f"] and got.pred[0].tolist() == want["pred"] and got.score[2].item() == 256 + 4 * 32
    again = W.chain_anchors(anchors, h=1024)
    assert all(torch.equal(u, v) for u, v in zip(again[:8], got[:8])) and again.f is None
    W.check_device_flags()
    anchors.lengths = _dev(np.array([65535, -1, 65536], dtype=np.int32))
    anchors.n_anchors = _dev(np.array([n + 1, n, 5], dtype=np.int32))
    bad = W.chain_anchors(anchors, h=2)
    assert torch.stack(list(bad[:8]), dim=1).tolist() == [[INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN]] * 3
    with pytest.raises(RuntimeError, match="3 read\\(s\\) with a length outside \\[0, 65535\\] or an anchor count outside \\[0, 32768\\]"):
        W.check_device_flags()
    W.check_device_flags()


# ---- whole --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted_index():
    return W.read_index(C.planted_reference_bases(), device=DEV)


def _assert_planted(m):
    want = C.planted_results()
    assert np.array_equal(torch.stack(list(m[:8]), dim=1).cpu().numpy(), C.result_rows(want))
    a = m.anchors
    assert a.n_anchors.tolist() == [r["n_kept"] for r in want] and a.n_minimizers.tolist() == [r["n_minimizers"] for r in want]
    assert a.truncated.tolist() == [0] * len(want)
    keys = a.keys.cpu().numpy()
    for b, r in enumerate(want):
        n = r["n_kept"]
        assert keys[b, :n].tolist() == r["keys"] and (keys[b, n:] == PAD).all()
        assert m.f[b, :n].tolist() == r["f"] and m.pred[b, :n].tolist() == r["pred"]


def test_the_planted_run(planted_index):
    """64 reads with 8 % errors on both strands against 20 000 bases with a planted repeat: every field equals the reference's, which
    tests/test_readmap_ref.py holds to the truth; the repeat read reports the lower copy and an equal runner-up"""
    _assert_index(planted_index, C.planted_reference_bases(), 15, 10)
    p = C.planted()
    labels, lengths = _dev(p["labels"]), _dev(p["lengths"])
    m = W.map_reads(labels, lengths, planted_index, want_pred=True)
    _assert_planted(m)
    again = W.map_reads(labels, lengths, planted_index, want_pred=True, chunk=64)
    assert all(torch.equal(u, v) for u, v in zip(again, m)) and torch.equal(again.anchors.keys, m.anchors.keys)      # bitwise repeatable
    assert m.mapped.all() and torch.equal(m.ref_span(), torch.stack([m.ref_start, m.ref_end], 1).long())
    read, (strand, a, b) = C.repeat_read()
    want = R.map_read_ref(read, C.planted_index())
    rl, rn = C.rows([read])
    got = W.map_reads(_dev(rl), _dev(rn), planted_index)
    assert torch.stack(list(got[:8]), dim=1).tolist() == [[want[f] for f in C.FIELDS]]
    assert got.runner_up.item() == got.score.item() and a - 20 <= got.ref_start.item() < got.ref_end.item() <= b + 20 and got.mapq().item() == 0.0
    W.check_device_flags()


def test_mapped_stretches_align_to_their_reads(planted_index):
    """decode -> map -> pairwise_align: the mapped stretch of the reference, in read orientation, against the mapped span of the read
    has an identity of at least 0.85 for every planted read (reads with 8 % errors; the CPU pairwise reference gives 0.903 as the
    least identity of the reference chain's stretches); and the PAF lines of the run"""
    p = C.planted()
    want = C.planted_results()
    labels, lengths = _dev(p["labels"]), _dev(p["lengths"])
    m = W.map_reads(labels, lengths, planted_index)
    ref, ref_lengths = m.labels()
    for b in (0, 1, 2, 3):
        st = p["ref"][want[b]["ref_start"]:want[b]["ref_end"]]
        assert ref[b, :ref_lengths[b]].tolist() == (R.revcomp(st) if want[b]["strand"] else st) and ref[b, ref_lengths[b]:].eq(0).all()
    wide, wide_lengths = m.labels(flank=25000)
    assert wide_lengths.eq(C.PLANT_REF).all() and wide[0].tolist() == p["ref"] and wide[1].tolist() == R.revcomp(p["ref"])
    query, query_lengths = W.trim_reads(labels, lengths, torch.stack([m.query_start, m.query_end], dim=1))
    aln = W.pairwise_align(ref, ref_lengths, query, query_lengths)
    identity = aln.identity.cpu().tolist()
    print("least identity %.4f" % min(identity))
    assert min(identity) >= 0.85
    names = ["read%d" % b for b in range(len(identity))]
    lines = W.paf_records(names, lengths, m, "planted", alignment=aln)
    assert len(lines) == 64
    r, mq = want[1], m.mapq().cpu().tolist()
    assert lines[1] == "read1\t%d\t%d\t%d\t-\tplanted\t20000\t%d\t%d\t%d\t%d\t%d\n" % (
        int(p["lengths"][1]), r["query_start"], r["query_end"], r["ref_start"], r["ref_end"], int(aln.matches[1]), int(aln.length[1]), int(mq[1] + 0.5))
    assert all(q == 60.0 for q in mq)                                             # margins of 1712 and more: unambiguous, as planted
    W.check_device_flags()


def test_a_poisoned_read_length_in_the_whole_call(planted_index):
    p = C.planted()
    lengths = p["lengths"][:4].copy()
    lengths[1], lengths[2] = -5, p["labels"].shape[1] + 1
    W.check_device_flags()
    m = W.map_reads(_dev(p["labels"][:4]), _dev(lengths), planted_index)
    want = C.result_rows(C.planted_results()[:4])
    want[1] = want[2] = [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN]
    assert np.array_equal(torch.stack(list(m[:8]), dim=1).cpu().numpy(), want) and m.anchors.n_anchors[1:3].tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.map_reads: 2 read\\(s\\)"):
        W.check_device_flags()
    W.check_device_flags()


def test_captured_into_a_graph(planted_index):
    p = C.planted()
    labels, lengths = _dev(p["labels"]), _dev(p["lengths"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        eager = W.map_reads(labels, lengths, planted_index, want_pred=True)    # warms the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.map_reads(labels, lengths, planted_index, want_pred=True)
    graph.replay()
    torch.cuda.synchronize()
    _assert_planted(captured)
    assert all(torch.equal(u, v) for u, v in zip(captured, eager)) and torch.equal(captured.anchors.keys, eager.anchors.keys)
    W.check_device_flags()
