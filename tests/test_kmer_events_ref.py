"""CPU: the plain-loop reference of wn_kmer_events (tests/kmer_events_ref.py) on a case worked by hand, the invariants that tie
its tables to its event rows, and the cases the GPU tests use (tests/kmer_events_cases.py) holding what they are meant to hold."""
import numpy as np

from tests import kmer_events_cases as EC
from tests import kmer_events_ref as R


def _hand_case():
    # read 0: samples 1 2 | 3 | 4 5 6 | 7, bases 1 2 3 4;  read 1: samples -1 -1.5 | (empty) | 2.5 0.5 | 10, cut after 5 samples
    signal = np.array([[1, 2, 3, 4, 5, 6, 7, 0], [-1, -1.5, 2.5, 0.5, 10, 10, 0, 0]], dtype=np.float32)
    begin = np.array([[0, 2, 3, 6], [0, 2, 2, 4]], dtype=np.int32)
    end = np.array([[2, 3, 6, 7], [2, 2, 4, 6]], dtype=np.int32)
    labels = np.array([[1, 2, 3, 4], [4, 4, 1, 2]], dtype=np.int32)
    return signal, np.array([7, 5], dtype=np.int32), labels, np.array([4, 4], dtype=np.int32), begin, end, np.array([4, 4], dtype=np.int32)


def test_the_hand_worked_case():
    out = R.kmer_events_ref(*_hand_case(), k=2, first=0, frac_bits=1, max_dwell=2)
    # k = 2, first = 0: event j takes labels j, j + 1; event 3 runs off the labels.  q = 2 x (frac_bits 1)
    assert out["kmer"].tolist() == [[0 * 4 + 1, 1 * 4 + 2, 2 * 4 + 3, -1], [3 * 4 + 3, -2, 0 * 4 + 1, -3]]
    assert out["start"].tolist() == [[0, 2, 3, 6], [0, 2, 2, 4]]
    assert out["length"].tolist() == [[2, 1, 3, 1], [2, 0, 2, 1]]
    assert out["sum"].tolist() == [[2 + 4, 6, 8 + 10 + 12, 0], [-2 - 3, 0, 5 + 1, 0]]
    assert out["sumsq"].tolist() == [[4 + 16, 36, 64 + 100 + 144, 0], [4 + 9, 0, 25 + 1, 0]]
    assert out["read_counts"].tolist() == [[3, 1, 0, 6], [2, 0, 2, 4]]
    assert out["bad"] == 0
    stats = out["kmer_stats"]
    assert stats[1].tolist() == [2, 4, 6 + 6, 20 + 26, 0]            # k-mer 1 (bases 1 2): event 0 of read 0, event 2 of read 1
    assert stats[6].tolist() == [1, 1, 6, 36, 0] and stats[11].tolist() == [1, 3, 30, 308, 0] and stats[15].tolist() == [1, 2, -5, 13, 0]
    assert int(stats[:, 0].sum()) == 5
    hist = out["dwell_hist"]
    assert hist.shape == (16, 3) and hist[1].tolist() == [0, 0, 2] and hist[6].tolist() == [0, 1, 0] and hist[11].tolist() == [0, 0, 1]


def test_rounding_ties_and_limits():
    assert [R.quantise(x, None, 0) for x in (0.5, 1.5, 2.5, -0.5, -1.5)] == [0, 2, 2, 0, -2]
    assert R.quantise(np.float32(8388607.0), None, 0) == 8388607 and R.quantise(np.float32(8388608.0), None, 0) is None
    assert R.quantise(np.float32(-2048.0), None, 12) is None and R.quantise(np.float32(2047.9998), None, 12) == 8388607
    assert R.quantise(float("nan"), None, 3) is None and R.quantise(float("inf"), None, 3) is None
    assert R.quantise(np.float32(1e30), (np.float32(1e30), np.float32(0)), 20) is None
    assert R.quantise(np.int16(-7), (np.float32(0.5), np.float32(0.25)), 2) == -13        # (-3.5 + 0.25) * 4


def test_a_bad_read_leaves_no_trace():
    args = list(_hand_case())
    args[4] = args[4].copy()
    args[4][1, 2] = 1                                                # event 2 of read 1 begins inside event 0
    out = R.kmer_events_ref(*args, k=2, first=0, frac_bits=1, max_dwell=2)
    assert out["bad"] == 1 and out["kmer"][1].tolist() == [-4] * 4 and out["read_counts"][1].tolist() == [-1] * 4
    assert not out["length"][1].any() and not out["sum"][1].any()
    assert int(out["kmer_stats"][:, 0].sum()) == 3                   # read 0 alone


def _check_invariants(out, max_dwell):
    used = out["kmer"] >= 0
    stats, hist = out["kmer_stats"], out["dwell_hist"]
    for code in range(stats.shape[0]):
        m = out["kmer"] == code
        squares = [int(v) for v in out["sumsq"][m]]
        assert stats[code].tolist() == [int(m.sum()), int(out["length"][m].sum()), int(out["sum"][m].sum()),
                                        sum(v & 0xffffffff for v in squares), sum(v >> 32 for v in squares)]
        assert hist[code].tolist() == np.bincount(np.minimum(out["length"][m], max_dwell), minlength=max_dwell + 1).tolist()
    good = out["read_counts"][:, 0] >= 0
    assert np.array_equal(out["read_counts"][good, 0], used[good].sum(1))
    assert np.array_equal(out["read_counts"][good, 3], (out["length"] * used)[good].sum(1))
    assert not out["sum"][~used].any() and not out["sumsq"][~used].any()


def test_table_columns_are_the_sums_over_used_events():
    for name in ("wave_edges_65_129", "gaps", "max_dwell_1", "cut_by_signal_length", "labels_shorter_than_k"):
        for layout in EC.LAYOUTS:
            _check_invariants(EC.reference(name, layout, "i16", 12), EC.CASES[name].kw.get("max_dwell", 255))
    for layout in EC.LAYOUTS:
        _check_invariants(EC.bad_reference(layout), 255)


def test_the_cases_hold_what_they_are_for():
    ref = EC.reference("long_events", "spans", "f32", 12)
    lengths = ref["length"][ref["kmer"] >= 0]
    assert {64, 65, 65536} <= set(lengths.tolist()) and 65537 not in lengths
    assert 65537 in ref["length"][ref["kmer"] == -3]
    assert EC.CASES["long_events"].signal.shape[1] < 70000
    assert (EC.reference("labels_shorter_than_k", "spans", "f32", 0)["kmer"] < 0).all()
    cut = EC.reference("cut_by_signal_length", "starts", "f32", 12)
    assert cut["kmer"][0].tolist().count(-3) == 1 and cut["kmer"][0].tolist().count(-2) == 3 and (cut["kmer"][1] == -2).all()
    assert (EC.spans_of(EC.CASES["gaps"])[:, 1:, 0] > EC.spans_of(EC.CASES["gaps"])[:, :-1, 1]).any()
    assert EC.reference("k6", "spans", "f32", 12)["kmer"].max() > 1023
    assert EC.reference("max_dwell_1", "starts", "i16", 0)["dwell_hist"][:, 0].sum() == 0
    for layout in EC.LAYOUTS:
        bad = EC.bad_reference(layout)
        assert (bad["read_counts"][:, 0] < 0).tolist() == EC.bad_expected(layout), layout
        assert bad["bad"] == sum(EC.bad_expected(layout))
    for name in EC.CASES:                                            # no case holds a bad read by accident
        for layout in EC.LAYOUTS:
            assert EC.reference(name, layout, "i16", 0)["bad"] == 0 and (EC.reference(name, layout, "f32", 12)["kmer"] >= 0).any() == (
                name != "labels_shorter_than_k"), (name, layout)
    # fp32 and int16 forms differ, frac_bits 0 and 12 differ: four references per layout, not one
    a, b = EC.reference("gaps", "spans", "f32", 12), EC.reference("gaps", "spans", "i16", 12)
    assert np.array_equal(a["kmer"], b["kmer"]) and not np.array_equal(a["sum"], b["sum"])
