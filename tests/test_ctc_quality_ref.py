"""CPU: the float64 reference of the per-base qualities (tests/ctc_quality_ref.py) against the worked example of DESIGN.md
section 7h, closed forms, its own invariants and the bad-input rules; and the precondition of tests/test_gpu_quality.py on the
very inputs that test uses: few bases sit on a rounding boundary of Q."""
import math

import numpy as np
import pytest

from tests import ctc_decode_ref as DR
from tests import ctc_quality_cases as QC
from tests import ctc_quality_ref as QR

EXAMPLE = np.array([[.9, .05, .05], [.1, .8, .1], [.2, .6, .2], [.7, .2, .1], [.25, .25, .5], [.4, .4, .2]]).T     # [C = 3, T = 6]


def test_the_worked_example():
    labels, frames = DR.greedy_decode(EXAMPLE)
    assert (labels, frames) == ([1, 2], [1, 4])                      # frame 5 is a tie and goes to class 0
    e, q, k, d, re, bad = QR.read_qualities(EXAMPLE, labels, frames, kind="probs", stat="mean")
    assert bad == 0 and d == [2, 1] and k == [5, 3]
    assert abs(e[0] - .3) < 1e-12 and abs(e[1] - .5) < 1e-12 and abs(re - .4) < 1e-12
    assert abs(q[0] - 5.228787452803376) < 1e-12 and abs(q[1] - 3.010299956639812) < 1e-12
    e, q, k, d, re, bad = QR.read_qualities(EXAMPLE, labels, frames, kind="probs", stat="best")
    assert d == [2, 1] and k == [7, 3]
    assert abs(e[0] - .2) < 1e-12 and abs(q[0] - 6.989700043360188) < 1e-12 and abs(re - .35) < 1e-12
    # the same frames as log-probabilities: the weights are p / max p, the ratio is the same
    e2, _, k2, d2, _, _ = QR.read_qualities(np.log(EXAMPLE), labels, frames, kind="log_probs")
    assert d2 == [2, 1] and k2 == [5, 3] and abs(e2[0] - .3) < 1e-12 and abs(e2[1] - .5) < 1e-12


def test_uniform_logits_give_four_fifths():
    x = np.full((1, 5, 9), 0.37)
    labels, frames, lengths = np.array([[3, 1] + [0] * 7]), np.array([[2, 5] + [0] * 7]), np.array([2])
    for stat in QR.STATS:
        r = QR.batch_qualities(x, labels, frames, lengths, stat=stat)
        assert np.abs(r["error"][0, :2] - 0.8).max() < 1e-15 and r["qual"][0, :2].tolist() == [1, 1]
        assert r["dwell"][0, :2].tolist() == [1, 1]                  # every frame's argmax is class 0: no run goes on
        assert abs(r["read_error"][0] - 0.8) < 1e-15 and r["bad"] == 0
        assert np.isnan(r["error"][0, 2:]).all() and not r["qual"][0, 2:].any() and not r["dwell"][0, 2:].any()


def test_quality_rounding_and_limits():
    assert QR.phred(0.0) == (float("inf"), 93)
    assert QR.phred(float("nan"))[1] == 0 and math.isnan(QR.phred(float("nan"))[0])
    assert QR.phred(1.0) == (0.0, 0) and QR.phred(1e-12)[1] == 93 and QR.phred(2.0)[1] == 0
    assert QR.phred(10 ** -0.95)[1] == 10 and QR.phred(10 ** -0.949)[1] == 9          # Q = 9.5 rounds up, 9.49 down
    q, k = QR.phred(0.3, qscale=0.7, qbias=2.5)
    assert abs(q - (0.7 * 5.228787452803376 + 2.5)) < 1e-12 and k == 6


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_dwell_sums_to_the_non_blank_argmax_frames(name):
    """on a greedy path every non-blank argmax frame before T_b belongs to exactly one run"""
    c = QC.case(name)
    for b in range(QC.B):
        tb = int(c.input_lengths[b])
        want = sum(1 for t in range(tb) if QR.frame_argmax(c.x[b, :, t]) != 0)
        assert int(c.ref["dwell"][b].sum()) == want
    assert c.ref["bad"] == 0
    v = c.valid()
    assert (c.ref["dwell"][v] >= 1).all() and (c.ref["error"][v] > 0).all() and (c.ref["error"][v] < 1).all()
    assert np.isnan(c.ref["read_error"][c.lengths == 0]).all() and np.isfinite(c.ref["read_error"][c.lengths > 0]).all()


def test_the_cases_hold_what_the_gpu_test_needs():
    c = QC.case("peaked_T1000")
    assert int(c.ref["dwell"][1].max()) >= QC.LONG_RUN               # one run across any 256-frame tile
    assert c.lengths[3] == 0 and math.isnan(c.ref["read_error"][3])  # the empty read
    tb, n = int(c.input_lengths[2]), int(c.lengths[2])
    assert tb < c.T and int(c.frames[2, n - 1] + c.ref["dwell"][2, n - 1]) == tb          # the last run ends exactly at T_b
    assert QR.frame_argmax(c.x[2, :, tb]) == c.labels[2, n - 1]      # and only T_b ends it: the next frame would go on
    assert (QC.case("peaked_T257").ref["dwell"] > 1).any() and (QC.case("random_T257").lengths > 64).any()
    for name in QC.CASES:
        assert QC.case(name).D < 40.0, name                          # expf(-D) stays far above the subnormal range


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_few_bases_sit_on_a_rounding_boundary(name):
    """the precondition of the GPU test's exact comparison of qual: at most 1 % of the bases of each of its inputs have a
    reference Q within 1e-3 of k + 0.5 (about 0.2 % is expected of a continuous distribution)"""
    c = QC.case(name)
    near, bases = int(c.near_boundary().sum()), int(c.valid().sum())
    print("%s: %d of %d bases within %.0e of a rounding boundary" % (name, near, bases, QC.NEAR))
    assert near <= 0.01 * bases


def test_bad_input_rules():
    c = QC.case("peaked_T37")
    x = c.x
    b = int(np.argmax(c.lengths))
    n, tb = int(c.lengths[b]), int(c.input_lengths[b])
    assert n >= 4
    good = QR.read_qualities(x[b], c.labels[b, :n], c.frames[b, :n], tb)

    def run(labels=None, frames=None, tb=tb):
        return QR.read_qualities(x[b], c.labels[b, :n] if labels is None else labels, c.frames[b, :n] if frames is None else frames, tb)

    def only(j, got, also_changed=()):
        e, q, k, d, re, bad = got
        assert math.isnan(e[j]) and k[j] == 0 and d[j] == 0 and math.isnan(re)
        for i in range(n):
            if i != j and i not in also_changed:
                assert (e[i], k[i], d[i]) == (good[0][i], good[2][i], good[3][i])
        return bad

    for value in (0, 99, -1, QC.C):                                  # the blank, and labels outside [0, C)
        labels = c.labels[b, :n].copy()
        labels[1] = value
        assert only(1, run(labels=labels)) == 1
    for value in (tb, -1, 2 ** 31 - 1):                              # a frame outside [0, T_b): the last base, so no successor suffers
        frames = c.frames[b, :n].copy()
        frames[n - 1] = value
        assert only(n - 1, run(frames=frames), also_changed=(n - 2,) if value < 0 else ()) == 1
    frames = c.frames[b, :n].copy()
    frames[2] = frames[1]                                            # two equal frames: the second base is bad, the first keeps {f} at least
    got = run(frames=frames)
    assert only(2, got, also_changed=(1,)) == 1 and got[3][1] == 1
    # a whole read: a length outside [0, Lmax], an input length outside [0, T]
    lengths, in_len = c.lengths.copy(), c.input_lengths.copy()
    lengths[b] = c.labels.shape[1] + 1
    r = QR.batch_qualities(x, c.labels, c.frames, lengths, in_len)
    assert r["bad"] == 1 and np.isnan(r["error"][b]).all() and not r["qual"][b].any() and not r["dwell"][b].any()
    assert math.isnan(r["read_error"][b])
    other = [i for i in range(QC.B) if i != b]
    assert np.array_equal(r["dwell"][other], c.ref["dwell"][other])
    lengths[b], in_len[b] = n, c.T + 1
    assert QR.batch_qualities(x, c.labels, c.frames, lengths, in_len)["bad"] == 1
    in_len[b] = -1
    assert QR.batch_qualities(x, c.labels, c.frames, lengths, in_len)["bad"] == 1


def test_fastq_records_on_the_host():
    import torch
    from wavenet_speech_amd.decoding import fastq_records, labels_to_strings
    labels = torch.tensor([[0, 0, 0], [1, 4, 0], [2, 3, 3]], dtype=torch.int32)
    qual = torch.tensor([[0, 0, 0], [0, 93, 7], [5, 40, 12]], dtype=torch.uint8)
    lengths = torch.tensor([0, 2, 3])
    records = fastq_records(["e", "f", "g h"], labels, lengths, qual)
    assert records == ["@e\n\n+\n\n", "@f\nAT\n+\n!~\n", "@g h\nGCC\n+\n&I-\n"]      # an empty read: empty SEQ and QUAL lines
    for rec, seq, q, n in zip(records, labels_to_strings(labels, lengths), qual.tolist(), lengths.tolist()):
        assert rec.split("\n")[1] == seq and [ord(ch) - 33 for ch in rec.split("\n")[3]] == q[:n]
    with pytest.raises(ValueError):
        fastq_records(["e"], labels, lengths, qual)
    with pytest.raises(ValueError):
        fastq_records(["e", "f", "g"], labels, lengths, torch.full((3, 3), 94, dtype=torch.uint8))
