"""CPU: the reference of the read mapping (tests/readmap_ref.py) held to definitions that do not share its code: (a) a brute-force
minimizer set that enumerates every window, over all short sequences; (b) a brute-force chain score that enumerates every
subsequence of a few anchors as a whole chain, and the forest property of the predecessor links; (c) cases worked by hand; (d) the
planted run of the issue, which the GPU file then compares field by field."""
import itertools
import random


from tests import readmap_cases as C
from tests import readmap_ref as R

INT_MIN = -2 ** 31


def test_fmix32_is_murmur3s_finaliser():
    assert R.fmix32(0) == 0 and R.fmix32(1) == 0x514E28B7 and R.fmix32(0xFFFFFFFF) == 0x81F16F39
    assert len({R.fmix32(x) for x in range(4 ** 6)}) == 4 ** 6          # a bijection: no two codes share a hash


def test_kmer_codes():
    # " AGCT": A 1, G 2, C 3, T 4.  AGC: f = 0*16 + 1*4 + 2 = 6; its reverse complement GCT: r = 1*16 + 2*4 + 3 = 27
    assert R.kmer([1, 2, 3], 0, 3) == (6, 0) and R.kmer([2, 3, 4], 0, 3) == (6, 1)
    assert R.kmer([1, 4], 0, 2) is None and R.kmer([2, 3], 0, 2) is None            # AT, GC: palindromes
    assert R.kmer([1, 0, 2], 0, 3) is None and R.kmer([1, 5, 2], 0, 3) is None      # breaks
    assert R.kmer([4] * 16, 0, 16) == (0, 1) and R.kmer([1] * 16, 0, 16) == (0, 0)  # poly-T is poly-A's reverse complement
    assert R.kmer([2] * 16, 0, 16) == (0x55555555, 0) and R.kmer([3] * 15 + [4], 0, 16) == (R.kmer([1] + [2] * 15, 0, 16)[0], 1)


def _brute_minimizers(keys, w):
    """every window's least valid key, collected: the definition read window by window"""
    n_k = len(keys)
    windows = [range(0, n_k)] if n_k < w else [range(s, s + w) for s in range(n_k - w + 1)]
    out = set()
    for win in windows:
        valid = [keys[t] for t in win if keys[t] is not None]
        if valid:
            out.add(min(valid)[1])
    return sorted(out)


def test_minimizers_against_every_window_of_every_short_sequence():
    """(a) all sequences of at most 8 labels over {1, 2, 4, 0} at k in {1, 2, 3} and w in {1, 2, 3, 5}"""
    checked = 0
    for n in range(0, 9):
        for seq in itertools.product((1, 2, 4, 0), repeat=n):
            for k in (1, 2, 3):
                n_k = n - k + 1
                if n_k < 1:
                    assert R.minimizers_ref(seq, k, 1) == []
                    continue
                codes = [R.kmer(seq, p, k) for p in range(n_k)]
                keys = [None if c is None else (R.fmix32(c[0]), p) for p, c in enumerate(codes)]
                for w in (1, 2, 3, 5):
                    got = R.minimizers_ref(seq, k, w)
                    assert [p for p, _, _ in got] == _brute_minimizers(keys, w), (seq, k, w)
                    assert all((c, s) == codes[p] for p, c, s in got)
                    checked += 1
    assert checked > 900000


def test_minimizers_worked_by_hand():
    """(c) A G C T A at k = 1, w = 2.  Codes (canon, strand): A (0, 0), G (1, 0), C (1, 1), T (0, 1); fmix32(0) = 0 < fmix32(1).
    Keys: (0, 0) (h, 1) (h, 2) (0, 3) (0, 4).  Windows [0,2) [1,3) [2,4) [3,5) have the minima 0, 1 (equal hashes: the smaller
    position), 3 and 3.  Position 4 holds the least hash there is and still is no minimizer: position 3 ties and comes first."""
    assert R.minimizers_ref([1, 2, 3, 4, 1], 1, 2) == [(0, 0, 0), (1, 1, 0), (3, 0, 1)]
    # n_k < w: the single window [0, n_k); a break invalidates exactly k k-mers
    assert R.minimizers_ref([2, 1, 3], 1, 5) == [(1, 0, 0)]
    assert [p for p, _, _ in R.minimizers_ref([1, 1, 2, 0, 2, 1, 1], 2, 1)] == [0, 1, 4, 5]
    assert R.minimizers_ref([1, 2], 3, 2) == [] and R.minimizers_ref([], 1, 1) == []
    # a homopolymer: all hashes equal, every window's minimum is its first position
    assert [p for p, _, _ in R.minimizers_ref([1] * 9, 3, 4)] == [0, 1, 2, 3]


def _brute_best_chain(part, k, h, max_dist, bandwidth, gap_base, gap_log):
    """the best score over every subsequence of the anchors taken as a whole chain (None: not a chain)"""
    best = None
    for m in range(1, len(part) + 1):
        for idx in itertools.combinations(range(len(part)), m):
            score = 16 * k
            for j, i in zip(idx, idx[1:]):
                dr, dq = part[i][0] - part[j][0], part[i][1] - part[j][1]
                if i - j > h or not (0 < dr <= max_dist and 0 < dq <= max_dist) or abs(dr - dq) > bandwidth:
                    score = None
                    break
                score += 16 * min(dr, dq, k) - R.gap_cost(abs(dr - dq), gap_base, gap_log)
            if score is not None and (best is None or score > best):
                best = score
    return best


def test_chain_against_every_subsequence_and_the_forest():
    """(b) at most 7 anchors of one strand: max f equals the best whole chain, and the predecessor links form a forest"""
    rnd = random.Random(5)
    for trial in range(400):
        m = rnd.randint(1, 7)
        part = sorted(set((rnd.randint(0, 30), rnd.randint(0, 30)) for _ in range(m)))
        args = (rnd.randint(1, 5), rnd.choice([1, 2, 3, 64]), rnd.randint(3, 30), rnd.randint(1, 12), rnd.randint(0, 6), rnd.randint(0, 12))
        f, pred, root, count = R.chain_strand_ref(part, *args)
        assert max(f) == _brute_best_chain(part, *args), (part, args)
        members = {}
        for i in range(len(part)):
            path, j = [], i
            while j >= 0:
                path.append(j)
                j = pred[j]
            assert path[-1] == root[i] and len(path) == count[i] and all(a > b for a, b in zip(path, path[1:]))
            members.setdefault(root[i], set()).update(path)
        roots = sorted(members)
        assert sum(len(s) for s in members.values()) == len(part)       # different roots: disjoint anchor sets, together all anchors
        assert all(root[j] == r for r in roots for j in members[r])


def test_chain_worked_by_hand():
    """(c) k = 4, h = 64, max_dist = 100, bandwidth = 10, gap_base = 2, gap_log = 8; forward anchors (r, q') = (10, 2) (14, 6) (19, 10)
    (40, 3).  f0 = 64 (fresh).  f1: from 0, dr = dq = 4, dd = 0: 64 + 16 * 4 = 128.  f2: from 1, dr = 5, dq = 4, dd = 1, gap = 2 * 1 +
    8 * 0 = 2: 128 + 64 - 2 = 190; from 0, dr = 9, dq = 8: 64 + 64 - 2 = 126.  f3: from 0, dq = 1 but dd = 29 > 10; from 1 and 2, dq < 0:
    fresh, 64.  The chain 0 -> 1 -> 2 covers the reference [10, 19 + 4) and the query [2, 10 + 4); the best score on another chain: 64."""
    rows = [(0, 10, 2), (0, 14, 6), (0, 19, 10), (0, 40, 3)]
    got = R.chain_ref(rows, 50, 4, 64, 100, 10, 2, 8)
    assert got["f"] == [64, 128, 190, 64] and got["pred"] == [-1, 0, 1, -1]
    assert [got[n] for n in C.FIELDS] == [190, 0, 10, 23, 2, 14, 3, 64]
    # the same anchors on the reverse strand of a read of 50: the query span turns round: [50 - 4 - 10, 50 - 2)
    got = R.chain_ref([(1, r, q) for _, r, q in rows], 50, 4, 64, 100, 10, 2, 8)
    assert [got[n] for n in C.FIELDS] == [190, 1, 10, 23, 36, 48, 3, 64] and got["pred"] == [-1, 0, 1, -1]
    # integer log: gap(1) = 2, gap(2) = 4 + 8, gap(3) = 6 + 8, gap(4) = 8 + 16, gap(7) = 14 + 16, gap(8) = 16 + 24
    assert [R.gap_cost(d, 2, 8) for d in (0, 1, 2, 3, 4, 7, 8)] == [0, 2, 12, 14, 24, 30, 40]
    # a fresh start beats an extension of equal score: gap_base = 16, dd = 1, min(dr, dq) = 1: 16 k + 16 - 16 = 16 k
    got = R.chain_ref([(0, 5, 5), (0, 7, 6)], 50, 4, 64, 100, 10, 16, 0)
    assert got["f"] == [64, 64] and got["pred"] == [-1, -1] and got["runner_up"] == 64 and got["ref_start"] == 5
    # a nearer predecessor with the greater score wins on the score: from (1, 1) 64 + 64, from (2, 2) 80 + 64
    got = R.chain_ref([(0, 1, 1), (0, 2, 2), (0, 9, 9)], 50, 4, 64, 100, 10, 16, 0)
    assert got["f"] == [64, 80, 144] and got["pred"] == [-1, 0, 1]
    # two EQUAL extensions: (1, 5) and (2, 4) are both fresh (dq < 0 between them) and both reach (9, 9) at 64 + 16 * 4 with free
    # gaps: the nearer predecessor, j = 1, wins, and the other start is the runner-up
    got = R.chain_ref([(0, 1, 5), (0, 2, 4), (0, 9, 9)], 50, 4, 64, 100, 10, 0, 0)
    assert got["f"] == [64, 64, 128] and got["pred"] == [-1, -1, 1] and got["ref_start"] == 2 and got["runner_up"] == 64
    # no anchors; equal best on both strands goes to the forward strand
    assert [R.chain_ref([], 50, 4)[n] for n in C.FIELDS] == [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN]
    got = R.chain_ref([(0, 30, 7), (1, 3, 1)], 50, 4)
    assert [got[n] for n in C.FIELDS] == [64, 0, 30, 34, 7, 11, 1, 64]
    assert R.chain_ref([(0, 30, 7)], 50, 4)["runner_up"] == INT_MIN


def test_anchors_worked_by_hand():
    """k = 2, w = 1 (every valid k-mer is a minimizer).  Reference A A G A C: k-mers AA (0, 0) at 0, AG at 1, GA at 2, AC at 3.
    AG: f = 1, r = CT = 2*4 + 3 = 11: canon 1 forward.  GA: f = 4, r = TC = 3*4 + 2 = 14: canon 4 forward.  AC: f = 2, r = GT = 7:
    canon 2 forward.  The read G T (length 2) holds GT = reverse complement of AC: canon 2, strand 1, so one anchor on the reverse
    strand: r = 3, q' = n - k - q = 0."""
    index = R.index_ref([1, 1, 2, 1, 3], 2, 1)
    assert index == [(0, 0, 0), (1, 1, 0), (2, 3, 0), (4, 2, 0)]
    assert R.anchors_ref([2, 4], index, 2, 1, 8, 16) == ([(1, 3, 0)], 1, 0)
    # A A A G: AA at 0 and 1 hits the one AA of the reference, AG its AG; enumeration order is by q, the cap keeps a prefix
    assert R.anchors_ref([1, 1, 1, 2], index, 2, 1, 8, 16) == ([(0, 0, 0), (0, 0, 1), (0, 1, 2)], 3, 0)
    assert R.anchors_ref([1, 1, 1, 2], index, 2, 1, 8, 2) == ([(0, 0, 0), (0, 0, 1)], 3, 1)
    assert R.anchors_ref([1, 1, 1, 2], index, 2, 1, 8, 3)[2] == 0
    # max_occ: the reference A A A has AA twice; max_occ = 1 drops both, max_occ = 2 keeps both
    twice = R.index_ref([1, 1, 1], 2, 1)
    assert R.anchors_ref([1, 1], twice, 2, 1, 1, 16) == ([], 1, 0)
    assert R.anchors_ref([1, 1], twice, 2, 1, 2, 16) == ([(0, 0, 0), (0, 1, 0)], 1, 0)
    assert R.pack((1, 3, 0)) == (1 << 43) | (3 << 16) and R.pack((0, 2 ** 26 - 1, 65535)) == (2 ** 26 - 1) * 65536 + 65535


def test_the_planted_run_maps_where_it_was_drawn():
    """(d) every read on its true strand, its reference span inside the true span widened by 20 bases and covering at least half of
    it.  Measured with this reference at the fixed seed: 64 of 64 reads, least coverage 0.717, least margin over the runner-up 1712."""
    p, results = C.planted(), C.planted_results()
    assert len(results) == C.PLANT_READS and all(400 * 0.85 < len(r) < 1200 * 1.15 for r in p["reads"])
    cover, margin = [], []
    for got, (strand, a, b) in zip(results, p["truth"]):
        assert got["strand"] == strand and got["truncated"] == 0
        assert a - 20 <= got["ref_start"] < got["ref_end"] <= b + 20
        assert 2 * (got["ref_end"] - got["ref_start"]) >= b - a
        assert 0 <= got["query_start"] < got["query_end"] <= len(p["reads"][len(cover)])
        cover.append((got["ref_end"] - got["ref_start"]) / (b - a))
        margin.append(got["score"] - max(got["runner_up"], 0))
    print("planted run: least coverage %.3f, least margin %d" % (min(cover), min(margin)))
    assert {s for s, _, _ in p["truth"]} == {0, 1}


def test_a_read_inside_the_repeat_has_an_equal_runner_up():
    """a read drawn wholly inside [3000, 3600) has the same anchors, shifted by 12 000, at [15000, 15600): two chains of equal
    score.  The lower copy comes first in (r, q') order, so it is the mapping, and runner_up == score says that it is ambiguous."""
    read, (strand, a, b) = C.repeat_read()
    got = R.map_read_ref(read, C.planted_index())
    assert got["strand"] == strand and got["runner_up"] == got["score"] > 16 * 15
    assert a - 20 <= got["ref_start"] < got["ref_end"] <= b + 20 and got["n_anchors"] >= 3
    shift = C.PLANT_REPEAT[2] - C.PLANT_REPEAT[0]
    keys = set(got["keys"])
    assert all(k + (shift << 16) in keys for k in got["keys"] if C.PLANT_REPEAT[0] <= (k >> 16) & (2 ** 27 - 1) < C.PLANT_REPEAT[1])
