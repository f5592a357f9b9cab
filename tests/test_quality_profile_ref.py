"""CPU: the loop reference of the quality profile (tests/quality_profile_ref.py) held to a hand-checked example, to its
invariants on random consistent op strings, to the bad-read rules; the calibration fit held to planted tables; and the inputs
of the GPU test (tests/quality_profile_cases.py) held to what that test says they contain."""
import numpy as np
import pytest

from tests import quality_profile_cases as PC
from tests import quality_profile_ref as PR

A, G, C, T = 1, 2, 3, 4                                              # the decoder's alphabet " AGCT"; 5 stands for the gap
GAP = 5


def _one(ops, ref, query, count_ends, qual=None, dwell=None, classes=5):
    return PR.profile([ops], [len(ops)], [ref], [len(ref)], [query], [len(query)], None if qual is None else [qual],
                      None if dwell is None else [dwell], classes, count_ends)


def _entries(table):
    return {(int(r), int(c)): int(table[r, c]) for r, c in zip(*np.nonzero(table))}


def test_the_worked_example():
    """ref ACGTT against query GACTTA:      -ACGTT-
                                            GAC-TTA      ops 4 1 1 3 1 1 4
    columns 0 and 6 lie outside [lo, hi] = [1, 5]: end columns unless count_ends"""
    ops, ref, query = [4, 1, 1, 3, 1, 1, 4], [A, C, G, T, T], [G, A, C, T, T, A]
    qual, dwell = [10, 20, 30, 40, 50, 93], [1, 2, 3, 40, 5, 6]
    r = _one(ops, ref, query, False, qual, dwell)
    assert r["bad"] == 0
    assert r["outcome"].tolist() == [[4, 1, 1, 1, 1, 4]]
    assert r["ref_index"].tolist() == [[-1, 0, 1, 3, 4, -1]]
    assert r["read_counts"].tolist() == [[4, 0, 0, 1, 2]]            # matches, mismatches, insertions, deletions, end columns
    assert _entries(r["confusion"]) == {(A, A): 1, (C, C): 1, (T, T): 2, (G, GAP): 1}
    assert _entries(r["q_counts"]) == {(20, 0): 1, (30, 0): 1, (40, 0): 1, (50, 0): 1}
    assert _entries(r["dwell_counts"]) == {(2, 0): 1, (3, 0): 1, (32, 0): 1, (5, 0): 1}       # dwell 40 goes to row 32
    r = _one(ops, ref, query, True, qual, dwell)
    assert r["outcome"].tolist() == [[3, 1, 1, 1, 1, 3]]
    assert r["ref_index"].tolist() == [[-1, 0, 1, 3, 4, -1]]
    assert r["read_counts"].tolist() == [[4, 0, 2, 1, 0]]
    assert _entries(r["confusion"]) == {(A, A): 1, (C, C): 1, (T, T): 2, (G, GAP): 1, (GAP, G): 1, (GAP, A): 1}
    assert _entries(r["q_counts"]) == {(20, 0): 1, (30, 0): 1, (40, 0): 1, (50, 0): 1, (10, 2): 1, (93, 2): 1}
    assert _entries(r["dwell_counts"]) == {(2, 0): 1, (3, 0): 1, (32, 0): 1, (5, 0): 1, (1, 2): 1, (6, 2): 1}


def test_a_mismatch_an_inner_insertion_and_no_aligned_column():
    r = _one([1, 2, 4, 1], [A, C, T], [A, G, G, T], False, qual=[7, 8, 9, 10])       # AC-T / AGGT
    assert r["outcome"].tolist() == [[1, 2, 3, 1]] and r["ref_index"].tolist() == [[0, 1, -1, 2]]
    assert r["read_counts"].tolist() == [[2, 1, 1, 0, 0]]
    assert _entries(r["confusion"]) == {(A, A): 1, (C, G): 1, (GAP, G): 1, (T, T): 1}
    assert _entries(r["q_counts"]) == {(7, 0): 1, (8, 1): 1, (9, 2): 1, (10, 0): 1}
    assert r["dwell_counts"] is None
    for count_ends, counts, outcome in ((False, [0, 0, 0, 0, 3], [4, 4]), (True, [0, 0, 2, 1, 0], [3, 3])):
        r = _one([3, 4, 4], [A], [C, C], count_ends, qual=[1, 2])
        assert r["read_counts"].tolist() == [counts] and r["outcome"].tolist() == [outcome]
        assert int(r["confusion"].sum()) == (3 if count_ends else 0) and int(r["q_counts"].sum()) == (2 if count_ends else 0)
    r = _one([], [], [], False)                                      # empty against empty is a valid read
    assert r["bad"] == 0 and r["read_counts"].tolist() == [[0, 0, 0, 0, 0]] and r["outcome"].shape == (1, 0)


@pytest.mark.parametrize("seed", range(6))
def test_invariants_on_random_walks(seed):
    rng = np.random.default_rng(seed)
    batch = PC.Batch(seed, [PC.random_ops(rng, int(n)) for n in rng.integers(0, 400, size=5)], 5)
    for count_ends in (False, True):
        r = batch.reference(count_ends)
        assert r["bad"] == 0
        counts = r["read_counts"].astype(np.int64)
        assert np.array_equal(counts.sum(1), batch.ops_len)          # the five counts sum to ops_len
        total = counts.sum(0)
        assert int(r["q_counts"].sum()) == int(r["dwell_counts"].sum()) == int(total[:3].sum())       # no deletion carries a quality
        assert np.array_equal(r["q_counts"].sum(0), total[:3]) and np.array_equal(r["dwell_counts"].sum(0), total[:3])
        assert int(r["confusion"].sum()) == int(total[:4].sum())
        assert int(r["confusion"][5, :].sum()) == total[2] and int(r["confusion"][:, 5].sum()) == total[3]
        assert int(np.trace(r["confusion"][:5, :5])) == total[0]
        for b in range(5):
            ops = batch.ops[b, :batch.ops_len[b]]
            if count_ends:                                           # then the counts are the op counts
                assert counts[b].tolist() == [int((ops == k).sum()) for k in (1, 2, 4, 3)] + [0]
            n = batch.query_len[b]
            assert (r["outcome"][b, :n] > 0).all() and not r["outcome"][b, n:].any() and (r["ref_index"][b, n:] == -1).all()
            aligned = r["outcome"][b, :n] <= 2
            assert (np.diff(r["ref_index"][b, :n][aligned]) > 0).all() and (r["ref_index"][b, :n][~aligned] == -1).all()


def test_bad_reads():
    good, mixed, bad_rows = PC.bad_batches()
    assert len(bad_rows) == len(PC.BAD_KINDS) == 8
    for count_ends in (False, True):
        want, got = good.reference(count_ends), mixed.reference(count_ends)
        assert want["bad"] == 0 and got["bad"] == 8
        for name in ("q_counts", "dwell_counts", "confusion"):       # a bad read adds nothing
            assert np.array_equal(want[name], got[name])
        assert (got["read_counts"][bad_rows] == -1).all() and not got["outcome"][bad_rows].any()
        assert (got["ref_index"][bad_rows] == -1).all()
        keep = [b for b in range(len(mixed.ops)) if b not in bad_rows]
        for name in ("read_counts", "outcome", "ref_index"):         # the neighbours are the good reads, in order
            assert np.array_equal(got[name][keep], want[name])
    # each kind alone makes a bad read, and the read it was copied from is good
    for b in bad_rows:
        assert mixed.take([b]).reference(False)["bad"] == 1
    # further rules: an op 2 over equal labels, a negative dwell, a negative label, ops that stop short of the labels
    assert _one([2], [A], [A], False)["bad"] == 1
    assert _one([1], [A], [A], False, dwell=[-1])["bad"] == 1
    assert _one([1], [-1], [-1], False)["bad"] == 1
    assert _one([1], [A, C], [A], False)["bad"] == 1 and _one([1], [A], [A, C], False)["bad"] == 1
    assert _one([1], [A], [A], False, qual=[93], dwell=[0])["bad"] == 0


def test_into_accumulates():
    a, b = PC.case("edges_c5_b4"), PC.case("special_c5")
    ra, rb = PC.reference("edges_c5_b4", False), PC.reference("special_c5", False)
    both = b.reference(False, into=tuple(a.reference(False)[k] for k in ("q_counts", "dwell_counts", "confusion")))
    for name in ("q_counts", "dwell_counts", "confusion"):
        assert np.array_equal(both[name], ra[name] + rb[name])


def test_the_gpu_cases_hold_what_they_promise():
    seen = set()
    for name in ("edges_c5", "edges_c64", "edges_c5_b4"):
        c = PC.case(name)
        assert 4 <= len(c.ops) <= 12
        seen.update(int(n) for n in c.ops_len)
        assert PC.reference(name, False)["bad"] == 0 and PC.reference(name, True)["bad"] == 0
    assert seen >= set(PC.OPS_LENGTHS)
    assert int(PC.case("edges_c64").ref.max()) > 32 and PC.case("edges_c64").classes == 64
    assert int(PC.case("edges_c5").dwell.max()) > 32
    s = PC.reference("special_c5", False)
    assert s["bad"] == 0
    assert s["read_counts"][0].tolist() == [0, 0, 0, 0, 70]          # no aligned column: all end columns
    assert s["read_counts"][1][4] == 70 + 90 + 5 + 7                 # the head of op 3s and op 4s, and the tail
    assert s["read_counts"][2].tolist() == [0, 0, 0, 0, 0]
    assert PC.reference("special_c5", True)["read_counts"][1][4] == 0


PLANTED = ((0.8, 3.0), (1.0, 0.0), (0.55, 6.5))


@pytest.mark.parametrize("a,b", PLANTED)
def test_fit_recovers_a_planted_line(a, b):
    table = PR.planted_table(a, b)
    assert int(table[60].sum()) == 99                                # the bin that must be ignored
    slope, bias, bins, bases, q_emp = PR.fit(table, min_count=100)
    print("planted (%g, %g): slope off by %.4f, intercept off by %.4f" % (a, b, abs(slope - a), abs(bias - b)))
    assert bins == 36 and bases == 36 * 200000
    assert abs(slope - a) <= 0.005 and abs(bias - b) <= 0.05
    assert np.isnan(q_emp[60]) and np.isnan(q_emp[4]) and np.isfinite(q_emp[5:41]).all()
    with_it = PR.fit(table, min_count=99)                            # and the bin is not ignored by accident
    assert with_it[2] == 37 and abs(with_it[0] - a) > 1e-6


def test_fit_definitions_by_hand():
    table = np.zeros((94, 3), dtype=np.int64)
    table[10] = (899, 60, 40)                                        # p = 100.5 / 1000
    table[20] = (1989, 5, 5)                                         # p = 10.5 / 2000
    slope, bias, bins, bases, q_emp = PR.fit(table, min_count=100)
    qe10, qe20 = -10 * np.log10(100.5 / 1000), -10 * np.log10(10.5 / 2000)
    assert abs(q_emp[10] - qe10) < 1e-12 and abs(q_emp[20] - qe20) < 1e-12
    assert abs(slope - (qe20 - qe10) / 10) < 1e-12 and abs(bias - (qe10 - slope * 10)) < 1e-12      # two points: the line through them
    assert (bins, bases) == (2, 2998)
    table[20] = 0
    assert PR.fit(table)[:3] == (None, None, 1)


@pytest.mark.parametrize("a,b", PLANTED)
def test_the_package_fit_on_the_same_tables(a, b):
    """wavenet_speech_amd.fit_quality_calibration is plain torch float64, so it runs wherever its table lies: the same bounds"""
    import torch
    import wavenet_speech_amd as W
    table = PR.planted_table(a, b)
    cal = W.fit_quality_calibration(torch.from_numpy(table), min_count=100)
    assert isinstance(cal, W.QualityCalibration) and isinstance(cal.qscale, float) and isinstance(cal.qbias, float)
    assert abs(cal.qscale - a) <= 0.005 and abs(cal.qbias - b) <= 0.05
    want = PR.fit(table)
    assert abs(cal.qscale - want[0]) <= 1e-9 * abs(want[0]) and abs(cal.qbias - want[1]) <= 1e-9 * max(abs(want[1]), 1.0)
    assert (cal.bins_used, cal.bases_used) == want[2:4] == (36, 7200000)
    assert np.array_equal(np.isnan(cal.q_empirical.numpy()), np.isnan(want[4]))
    assert np.allclose(cal.q_empirical.numpy()[5:41], want[4][5:41], rtol=1e-12, atol=0)


def test_the_package_fit_refuses_what_is_no_calibration():
    import torch
    import wavenet_speech_amd as W
    table = torch.zeros(94, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="a line needs two"):
        W.fit_quality_calibration(table)
    table[10] = torch.tensor([899, 60, 40])
    with pytest.raises(ValueError, match="a line needs two"):
        W.fit_quality_calibration(table)
    table[20] = torch.tensor([500, 300, 200])                        # more errors at the higher quality: a falling line
    with pytest.raises(ValueError, match="no calibration"):
        W.fit_quality_calibration(table)
    table[20] = torch.tensor([899, 60, 40])                          # a flat line
    with pytest.raises(ValueError, match="no calibration"):
        W.fit_quality_calibration(table)
    for wrong in (table[:93], table.double(), table.tolist()):
        with pytest.raises(ValueError):
            W.fit_quality_calibration(wrong)
    with pytest.raises(ValueError):
        W.fit_quality_calibration(table, min_count=0)
