"""CPU: what the cases of tests/tool_limits_cases.py reach, from the references alone (tests/event_align_ref.py,
tests/event_detect_ref.py, tests/readmap_ref.py, tests/demux_ref.py) -- so that tests/test_gpu_tool_limits.py, which runs them on
the device, holds the kernels where their header comments say they are tight.  No test here touches the library."""
import numpy as np
import pytest

from tests import demux_ref as DR
from tests import event_align_cases as EA
from tests import event_align_ref as EAR
from tests import event_detect_cases as ED
from tests import readmap_ref as RR
from tests import tool_limits_cases as C


# ================================================================================================================ event alignment
def _windows(case, ref):
    """[(read, e0, nf, g0, lowest byte, highest byte, s_end & 3)] over the aligned reads of a case"""
    out = []
    for b, sc in enumerate(ref["score"]):
        if sc not in (EAR.NO_ALIGNMENT, EAR.BAD_READ):
            out += [(b,) + w for w in C.event_trace_windows(ref["states"][b, :int(case.n_events[b])])]
    return out


def _steep_windows(band):
    names = [n for n in C.EVENT_ALIGN if n.endswith("_w%d" % band)]
    return [w for n in names for w in _windows(C.event_align_case(n), C.event_align_reference(n))]


def test_the_model_of_the_trace_loop_by_hand():
    """E = 129, one leading move of 2: the state of event e >= 1 is 3 e - 1, the full chunk [64, 128) ends in state 380 = 0 (mod 4)
    and its window, from byte 47 of the row, is read from byte 0 (state 191) to byte 48 (state 380)"""
    states = [0] + [3 * e - 1 for e in range(1, 129)]
    assert C.event_trace_windows(states) == [(128, 1, 48, 47, 47, 3), (64, 64, 47, 0, 48, 0), (0, 64, 0, 0, 47, 0)]
    plain = [3 * e for e in range(129)]                              # all double skips: a full chunk ends at 1 (mod 4): bytes 1 to 48
    assert C.event_trace_windows(plain)[1] == (64, 64, 47, 1, 48, 1)


@pytest.mark.parametrize("name", [n for n in C.EVENT_ALIGN if not n.startswith("largest")])
def test_steep_reads_follow_the_planted_moves(name):
    case, ref = C.event_align_case(name), C.event_align_reference(name)
    assert ref["bad"] == 0
    for b, want in enumerate(C.planted_moves(name)):
        assert ref["score"][b] not in (EAR.NO_ALIGNMENT, EAR.BAD_READ)
        if want is not None:
            assert ref["moves"][b].tolist() == want and 1 + sum(want) == case.n_events[b], (name, b)
    for w in _windows(case, ref):
        assert 0 <= w[4] <= w[5] < C.WIN_BYTES, (name, w)           # the model stays inside the window: so does the kernel


@pytest.mark.parametrize("band", C.STEEP_BANDS)
def test_the_trace_window_is_read_at_both_corners(band):
    """among windows that do not start at byte 0 of the row: a chunk reads byte 0 and byte 48 together; all four values of s_end & 3
    occur; byte 0 is reached at s_end = 0 and at s_end = 3 (mod 4); a read of several chunks ends in a partial one"""
    inner = [w for w in _steep_windows(band) if w[3] > 0]
    assert any(w[4] == 0 and w[5] == C.WIN_BYTES - 1 for w in inner)
    assert {w[6] for w in inner} == {0, 1, 2, 3}
    assert {w[6] for w in inner if w[4] == 0} == {0, 3}
    assert {w[5] for w in inner if w[4] == 0} == {C.WIN_BYTES - 2, C.WIN_BYTES - 1}      # s_end = 3 (mod 4): bytes 0 to 47
    assert any(0 < w[2] < C.TRACE and w[1] > 0 for w in _steep_windows(band))
    partial = [w for w in _steep_windows(band) if w[2] < C.TRACE]
    assert {w[2] for w in partial} >= {1, 2, 3, 4}                   # E = 65..68 and 129, 193: a last chunk of 1 to 4 events


def test_the_earlier_cases_never_read_byte_0_of_an_inner_window():
    """tests/event_align_cases.py, recomputed: the lowest byte of a window with g0 > 0 is 1 (and 2) in `three_rearm` and 12 in
    every other case: no window is read at byte 0"""
    inner = []
    for name, case in EA.CASES.items():
        inner += [(name,) + w for w in _windows(case, EA.reference(name)) if w[3] > 0]
    assert inner and not any(w[5] == 0 for w in inner)
    assert min(w[5] for w in inner) == 1 and {w[0] for w in inner if w[5] < 12} == {"three_rearm"}
    assert min(w[5] for w in inner if w[0] != "three_rearm") == 12


@pytest.mark.parametrize("name", list(C.LARGEST_MOVES))
def test_the_largest_scores(name):
    """T_b = 2^24 exactly; the dearest read costs 2^24 (2^31 - 1 + 2^30 - 1) = 1.5 2^55 - 2^25 and its moves, below the 2^56 of the
    kernel's bound; the cheapest -2^24 (2^30 - 1) and its moves: about -2^54, a score and no sentinel; the read that ends at
    2^24 + 1 is bad and nothing else is"""
    case, ref = C.event_align_case(name), C.event_align_reference(name)
    n, E = C.LARGEST_N, C.LARGEST_E
    assert case.ev_starts[:3, E].tolist() == [1 << 24] * 3 and case.ev_starts[3, E + 1] == (1 << 24) + 1 == EAR.MAX_SIGNAL + 1
    assert case.n_events.tolist() == [E, E, E, E + 1] and ref["bad"] == 1
    score = [int(v) for v in ref["score"]]
    assert score[3] == EAR.BAD_READ and (ref["moves"][3] == -1).all() and (ref["states"][3] == -1).all()
    mc = C.LARGEST_MOVES[name]
    moves = [sum(int(c) * m for c, m in zip(ref["moves"][b], mc)) for b in range(3)]
    assert score[0] == E * n * ((1 << 31) - 1 + (1 << 30) - 1) + moves[0] and 3 << 54 > score[0] - moves[0] == (3 << 54) - (1 << 25)
    assert score[1] == -E * n * ((1 << 30) - 1) + moves[1] and -(1 << 54) <= score[1] - moves[1] < -(1 << 54) + (1 << 25)
    assert score[2] == E * n + moves[2]
    assert EAR.BAD_READ < score[1] < 0 and all(abs(s) < 1 << 56 for s in score[:3])
    if name == "largest_top_moves":
        assert moves == [(E - 1) * ((1 << 30) - 1)] * 3 and score[0] > 3 << 54          # 255 moves at the largest cost a move can have


# ================================================================================================================ event detection
def test_one_sample_at_the_reach_decides_a_boundary_at_every_seam():
    """for every pair: the plain read and the one altered 95 samples to the right (96 to the left) of position i differ in whether
    i is a boundary; altered one sample further out, nothing changes.  i is the last position before and the first after the seams
    256, 768 and 1536"""
    ref = C.reach_reference()
    assert ref["bad"] == 0
    seen = set()
    for p, (side, seam, i, at, beyond) in enumerate(C.reach_pairs()):
        assert at == (i + 95 if side == "right" else i - 96) and abs(beyond - i) == abs(at - i) + 1
        plain, altered, further = (ED.boundaries(ref, 3 * p + u) for u in range(3))
        assert ((i, ED.R.KIND_LONG) in altered) != ((i, ED.R.KIND_LONG) in plain), (side, i)
        assert ((i, ED.R.KIND_LONG) in plain) == (side == "left")
        assert further == plain and altered != plain
        assert not any(pos == i for pos, _ in (altered if side == "left" else plain))
        seen.add((side, seam, i - seam))
    assert seen == {(s, m, o) for s in ("left", "right") for m in C.REACH_SEAMS for o in (-1, 0)}
    case = C.reach_case()
    assert (case.signal_lengths == C.REACH_T).all() and case.kw["windows"] == (16, 16) and case.kw["radii"][0] == 64
    sub, raw, ss, want, rows = C.reach_int16()                        # the int16 form quantises to the same integers
    assert [ED.boundaries(want, u) for u in range(len(rows))] == [ED.boundaries(ref, b) for b in rows]
    assert np.array_equal(raw * 0.5 + 3.0, sub.signal) and raw.dtype == np.int16


@pytest.mark.parametrize("M", [32, 33])
def test_event_sums_on_both_sides_of_the_hand_over(M):
    """66 forced events of M samples and a last one of 1, 31, 32 (and 33) samples, all samples +-(2^23 - 1): closed forms"""
    (case, lasts), ref = C.sums_case(M), C.sums_reference(M)
    assert lasts == [1, 31, 32, 33][:3 + (M == 33)] and ref["bad"] == 0
    for b in range(len(case.signal_lengths)):
        sign, last = (1 if b < len(lasts) else -1), lasts[b % len(lasts)]
        n = C.SUMS_EVENTS + 1
        assert ref["n_events"][b] == n and ref["kind"][b, 1:n].tolist() == [ED.R.KIND_FORCED] * (n - 1)
        lens = [M] * C.SUMS_EVENTS + [last]
        assert [int(v) for v in ref["sum"][b, :n]] == [sign * m * C.QMAX for m in lens]
        assert [int(v) for v in ref["sumsq"][b, :n]] == [m * C.QMAX * C.QMAX for m in lens]


# =================================================================================================================== read mapping
@pytest.mark.parametrize("w", C.K16_W)
def test_k16_codes_with_bit_31(w):
    """index entries and anchors whose canonical code is 2^31 or more exist; the reads look up the smallest and the largest code of
    the index (the largest has bit 31 set), which puts the lower-bound probes at entry 0 and at n_entries"""
    index, results = C.k16_index(w), C.k16_results(w)
    ref, reads = C.k16()
    high = {p for c, p, _ in index if c >= 1 << 31}
    assert len(index) > 100 and len(index) // 8 < len(high) < len(index) // 2
    hit = set()
    for r in results:
        assert r["truncated"] == 0 and r["n_kept"] > 0 and r["score"] > 0
        hit |= {(key >> 16) & ((1 << 27) - 1) for key in r["keys"]}
    assert hit & high
    assert index[-1][0] >= 1 << 31 and index[-1][1] in hit and index[0][1] in hit
    assert {r["strand"] for r in results} == {0, 1}
    for b, read in enumerate(reads):                                 # the anchors with bit 31 set carry a read's own lookups
        mins = RR.minimizers_ref(read, 16, w)
        assert any(c >= 1 << 31 for _, c, _ in mins) and len(read) > 250


def test_fast_anchors_equal_the_plain_reference_on_a_cut():
    """the whole-array form of anchors_ref at k = w = 1 against the plain loops, on cuts of the reads with the cap on both sides of
    the total"""
    ref, reads = C.occ()
    index = C.occ_index()
    for name, lo, hi in (("dense", 0, 40), ("sparse", 0, 700), ("sparse", 64900, 65535), ("shorter", 280, 330), ("two_tiles", 0, 257)):
        cut = reads[name][lo:hi]
        for cap in (1, 100, 1000, 32768):
            for max_occ in (63, 64, 65):
                got = C.fast_anchors_k1(cut, index, max_occ, cap)
                want = RR.anchors_ref(cut, index, 1, 1, max_occ, cap)
                assert got[:3] == want, (name, cap, max_occ)


def test_fast_chains_equal_the_plain_reference_on_a_cut():
    """the whole-array form of chain_strand_ref against the plain loops: on kept prefixes of the reads below, with h below and above
    the anchors that share a reference position, and on the 1400 anchors of the window case at h = 1024"""
    reads = C.occ()[1]
    for name, cap, h in (("dense", 1000, 64), ("dense", 3000, 300), ("sparse", 1000, 64), ("two_tiles", 2000, 1024)):
        rows = sorted(C.fast_anchors_k1(reads[name], C.occ_index(), 64, cap)[0])
        assert C.fast_chain_ref(rows, len(reads[name]), 1, h=h) == RR.chain_ref(rows, len(reads[name]), 1, h=h), name
    assert C.fast_chain_ref(C.window_anchors(), 20000, C.WINDOW_K, h=1024, **C.WINDOW_KW) == C.window_reference(1024)
    assert RR.chain_strand_ref.__module__ == RR.__name__             # the plain function is back in its place


def test_the_longest_read_at_the_largest_max_occ():
    """the code 0 has exactly 64 entries and the code 1 has 65; the dense read has 65535 * 64 anchors, the most a read can have
    (2^22 - 64: the 2^22 of the packed field is out of reach by one position), and full tiles of 256 positions with 64 hits each;
    among the kept reverse-strand anchors of the sparse read q' reaches 65534 and 0"""
    index = C.occ_index()
    assert [sum(1 for c, _, _ in index if c == v) for v in (0, 1)] == [C.OCC_REF_KEPT, C.OCC_REF_DROPPED] == [64, 65]
    ref, reads = C.occ()
    assert [len(reads[n]) for n in C.OCC_READS] == [65535, 65535, 65534, 257]
    big, small = C.occ_results(32768), C.occ_results(1000)
    assert big[0]["total"] == 65535 * 64 == (1 << 22) - 64 and big[2]["total"] == 65234 * 64 > 1 << 21
    assert np.isin(reads["dense"][:256], (1, 4)).all() and np.isin(reads["shorter"][512:768], (1, 4)).all()       # whole tiles of hits
    assert [r["n_minimizers"] for r in big] == [65535, 65535, 65534, 257]
    assert [(r["n_anchors"], r["truncated"]) for r in big] == [(32768, 1), (300 * 64, 0), (32768, 1), (257 * 64, 0)]
    assert [(r["n_anchors"], r["truncated"]) for r in small] == [(1000, 1)] * 4
    rev = [(r, q) for s, r, q in big[1]["rows"] if s == 1]
    assert max(q for _, q in rev) == 65534 and min(q for _, q in rev) == 0
    assert {s for s, _, _ in big[0]["rows"]} == {0, 1}
    for r in big + small:
        assert r["keys"] == sorted(r["keys"]) and len(set(r["keys"])) == len(r["keys"]) and r["chain"]["score"] > 16
    back = [i - p for i, p in enumerate(big[0]["chain"]["pred"]) if p >= 0]      # h = 1024 on 32768 anchors: the ring wraps 32 times
    assert C.OCC_H[32768] == 1024 and max(back) == 1024 and sum(1 for d in back if d > 512) > 1000 and big[0]["chain"]["n_anchors"] == 64


def test_the_full_window_of_predecessors():
    """1400 anchors of one strand: the ring of 1024 wraps; predecessors lie more than 512, more than 960 (the last round of lanes)
    and more than 1000 anchors back, so h = 1000 and h = 1024 differ; the companion rows reach exactly h back"""
    rows = C.window_anchors()
    assert len(rows) == C.WINDOW_ANCHORS >= 1300 and {s for s, _, _ in rows} == {0}
    full, less = C.window_reference(1024), C.window_reference(1000)
    back = [i - p for i, p in enumerate(full["pred"]) if p >= 0]
    assert max(back) > 1000 and sum(1 for d in back if d > 512) >= 10 and sum(1 for d in back if d > 960) >= 2
    assert max(i - p for i, p in enumerate(less["pred"]) if p >= 0) <= 1000 and less["f"] != full["f"]
    assert {(d - 1) // 64 for d in back} >= set(range(10)) | {15}
    for h in C.WINDOW_H:
        for d in C.WINDOW_REACH:
            r = RR.chain_ref(C.reach_anchors(d), 20000, 15, h=h, **C.WINDOW_REACH_KW)
            assert r["pred"][-1] == (0 if d <= h else -1), (h, d)


# ================================================================================================================= demultiplexing
def test_1024_patterns_and_picks_past_lane_63():
    case, ref = C.demux_case(), C.demux_reference()
    assert (case.n_front, len(case.group) - case.n_front, len(case.group)) == (513, 511, DR.MAX_PATTERNS)
    assert set(case.pattern_lengths.tolist()) == set(range(1, 13)) and ref["bad"] == 0
    pick = C.demux_pick_reference(0, 1, 0.0)
    for b, (lo, hi) in enumerate(C.DX_PLANTS):
        assert ref["score"][b, lo] == ref["score"][b, hi] == 12 * case.costs[0] == ref["score"][b, :case.n_front].max()
        assert pick["hits"][b, 0].tolist() == [lo, 72, 0, 12]
    assert C.DX_PLANTS[0][0] >= 64 and C.DX_PLANTS[0][0] % 64 == C.DX_PLANTS[0][1] % 64      # one lane, two rounds of the strided loop
    assert pick["runner_up"][0, 0] == 72 and case.group[70] != case.group[134]                # ties with another group's
    assert pick["runner_up"][1, 0] < 72 and case.group[75] == case.group[139]                 # ties with its own group's only
    assert pick["runner_up"][2, 0] == 72 and C.DX_PLANTS[2][0] < 64 <= C.DX_PLANTS[2][1]
    assert (pick["hits"][:, 1, 0] >= case.n_front).all()
    strict = C.demux_pick_reference(1, 1, 0.0)
    assert strict["barcode"].tolist() != pick["barcode"].tolist() or (strict["trim"] != pick["trim"]).any()
