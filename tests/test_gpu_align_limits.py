"""GPU: ctc_forced_align (csrc/wn_align.hip), pairwise_align (csrc/wn_pairalign.hip) and quality_profile (csrc/wn_profile.hip) at
the window, cost and length limits their header comments state, against tests/ctc_align_ref.py, tests/pairwise_align_ref.py and
tests/quality_profile_ref.py.  Every comparison is exact equality: the forced aligner's inputs lie on a quarter grid where every
sum is exact and ties are real, the other two kernels are integer.  No tolerance and no excluded frame.  The inputs and their
references are built once in tests/align_limits_cases.py; tests/test_align_limits_ref.py asserts on the CPU that they reach what
each test below names (the corners of both trace windows among them)."""
import time

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import align_limits_cases as C
from tests import ctc_align_ref as A
from tests import pairwise_align_ref as R
from tests.gpu_labels import assert_profile as _equal, forced_align as _run, pair_align as _align
from tests.gpu_util import DEV, dev as _dev, no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu


# ========================================================================================================= the forced aligner
def _check_exact(labels, blank, Tb, want, states, frame_labels, spans, score, tag):
    """one utterance, as tests/gpu_labels.py::check_utterance(exact=True) has it, against a cached reference"""
    want_states, want_score, want_spans = want
    L = len(labels)
    assert (states[Tb:] == -1).all() and (frame_labels[Tb:] == -1).all() and (spans[L:] == -1).all(), tag
    if not want_score > -np.inf or Tb == 0:
        assert score == np.float32(want_score), (tag, score, want_score)
        assert (states == -1).all() and (frame_labels == -1).all() and (spans == -1).all(), tag
        return
    st = states[:Tb]
    assert np.array_equal(frame_labels[:Tb], A.frame_labels_of(st, labels, blank)), tag
    assert np.array_equal(spans[:L], A.spans_of(st, L)), tag
    assert np.array_equal(st, want_states), (tag, np.nonzero(st != want_states)[0][:10])
    assert np.array_equal(spans[:L], want_spans), tag
    assert score == np.float32(want_score), (tag, score, want_score)


@pytest.mark.parametrize("name", list(C.FORCED))
def test_forced_alignment_equals_the_reference(name):
    """steep_* / lead_* / near_*: a trace chunk walks its whole 9-word window; ties_*: the tie rule where `left` crosses waves;
    time_*: the 64-frame chunk edges; two_classes_* / classes64_*: the class limits; neg_inf: -inf log-probabilities"""
    case = C.forced(name)
    T = case.x.shape[2]
    in_len = None if case.input_lengths is None else torch.tensor(case.input_lengths)
    states, frame_labels, spans, score = _run(torch.from_numpy(case.x), case.labels, in_len, input="log_probs", blank=case.blank)
    W.check_device_flags()                                           # an utterance without an alignment is not a bad one
    for b, (labels, want) in enumerate(zip(case.labels, C.forced_reference(name))):
        Tb = T if case.input_lengths is None else case.input_lengths[b]
        _check_exact(labels, case.blank, Tb, want, states[b], frame_labels[b], spans[b], score[b], "%s[%d]" % (name, b))
    if name == "neg_inf":
        assert np.isneginf(score[1]) and np.isfinite(score[[0, 2]]).all()


# ======================================================================================================= the pairwise aligner
def _check_pair(a, b, costs, free, want, score, stats, ops, ops_len, tag):
    """one pair, as tests/gpu_labels.py::check_pair has it, against a cached reference or a closed form"""
    assert score == want.score, (tag, score, want.score)
    assert tuple(stats) == (want.matches, want.mismatches, want.gaps, want.length), (tag, tuple(stats), want[1:5])
    assert ops_len == want.length, (tag, ops_len, want.length)
    got = ops[:ops_len]
    assert np.array_equal(got, want.ops), (tag, np.nonzero(got != want.ops)[0][:10])
    assert (ops[ops_len:] == 0).all(), tag
    _check_consistent(a, b, costs, free, score, stats, got, tag)


def _check_consistent(a, b, costs, free, score, stats, got, tag):
    """without any reference: both rows come out exactly once, the ops rescore to the score, the counts are the op counts"""
    assert R.replay(a, b, got) == (list(a), list(b)), tag
    assert R.rescore(got, *costs, free) == score, tag
    assert (int((got == 1).sum()), int((got == 2).sum()), int((got >= 3).sum()), len(got)) == tuple(stats), tag


def _check_case(name, free, rows=None, one_by_one=False):
    """the pairs of a case in one launch, or each in a launch of its own (so that a short query runs in the one-wave kernel)"""
    case = C.pairs(name)
    rows = range(len(case.refs)) if rows is None else rows
    for group in ([[n] for n in rows] if one_by_one else [list(rows)]):
        refs, queries = [case.refs[n] for n in group], [case.queries[n] for n in group]
        score, stats, ops, ops_len = _align(refs, queries, case.costs, free)
        for k, n in enumerate(group):
            _check_pair(refs[k], queries[k], case.costs, free, C.pair_reference(name, n, free), int(score[k]), stats[k], ops[k],
                        int(ops_len[k]), "%s[%d] free=%s" % (name, n, free))
    W.check_device_flags()


def _score_only(a, b, costs, free):
    from wavenet_speech_amd import decoding as D
    score, stats, ops, ops_len = D._pair_align("test", _dev(np.array([a], dtype=np.int32)), _dev(np.array([len(a)], dtype=np.int32)),
                                               _dev(np.array([b], dtype=np.int32)), _dev(np.array([len(b)], dtype=np.int32)), costs, free,
                                               False, False)
    assert stats is None and ops is None and ops_len is None
    return int(score.cpu()[0])


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", ["emboss", "largest"])
@pytest.mark.parametrize("group", sorted(C.SELF_GROUPS))
def test_a_row_against_itself(group, costs, free):
    """64 diagonal lookups per trace chunk: the 72-step x 9-thread window from corner to corner, at every column phase"""
    _check_case("self_%s/%s" % (group, costs), free)


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("name", ["variants_200/emboss", "variants_200/largest", "variants_600/emboss"])
def test_a_row_against_itself_with_one_mismatch_or_shifted(name, free):
    _check_case(name, free)


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", ["emboss", "largest"])
def test_the_widest_row_against_itself_by_closed_form(costs, free):
    """N = M = 8192: all 1024 threads, 128 full trace chunks on the diagonal.  Beyond the reference's reach: the closed form"""
    a, b = C.identical_rows(C.SELF_CLOSED)
    score, stats, ops, ops_len = _align([a], [b], C.COSTS[costs], free)
    _check_pair(a, b, C.COSTS[costs], free, C.identical_result(C.SELF_CLOSED, C.COSTS[costs]), int(score[0]), stats[0], ops[0],
                int(ops_len[0]), "identical 8192")
    assert _score_only(a, b, C.COSTS[costs], free) == int(score[0])
    W.check_device_flags()


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", C.COST_LIMIT_SETS)
@pytest.mark.parametrize("size", [300, 1100])
def test_cost_limits(size, costs, free):
    """match / mismatch of +-1024, gap_open 1024, gap_extend 0 and equal to gap_open, all zero, all positive: the full form, and
    the stats-only and score-only forms equal to it"""
    name = "costs_%d/%s" % (size, costs)
    _check_case(name, free)
    case = C.pairs(name)
    score, stats, ops, ops_len = _align(case.refs, case.queries, case.costs, free, return_ops=False)
    for n in range(len(case.refs)):
        want = C.pair_reference(name, n, free)
        assert int(score[n]) == want.score and tuple(stats[n]) == tuple(want[1:5]), (name, n)
        assert _score_only(case.refs[n], case.queries[n], case.costs, free) == want.score, (name, n)
    W.check_device_flags()


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("N", C.RING_N)
def test_ring_reloads(N, free):
    """the reference ring reloads every 1024 steps: N around the reloads against M = 8 (one wave), 520 and 1100 (several)"""
    _check_case("ring_N%d" % N, free, one_by_one=True)


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("name", ["threads_1100x8192", "waves_2100x4104"])
def test_all_threads_and_nine_waves_across_a_reload(name, free):
    _check_case(name, free)


@pytest.mark.parametrize("free", [True, False])
def test_the_longest_stream_score_only(free):
    """N = 65535 = kPaMaxRef against M = 8192 = kPaMaxQuery, by closed form"""
    N, M = C.LONGEST
    assert _score_only(*C.unequal_rows(N, M), C.UNEQUAL_COSTS, free) == C.unequal_score(N, M, free)
    assert _score_only(*C.equal_rows(N, M), C.EQUAL_COSTS, free) == C.equal_score(N, M, free)
    W.check_device_flags()


def _longest_full_form(free):
    a, b = C.unequal_rows(*C.LONGEST)
    torch.cuda.synchronize()
    t0 = time.time()
    score, stats, ops, ops_len = _align([a], [b], C.UNEQUAL_COSTS, free)
    print("full form %d x %d free=%s: %.3f s with the copies" % (C.LONGEST + (free, time.time() - t0)))
    return a, b, int(score[0]), stats[0], ops[0], int(ops_len[0])


@pytest.mark.parametrize("free", [True, False])
def test_the_longest_stream_full_form(free):
    """the same pair with its path: 66558 steps of 1024 threads, a workspace of 272 MB.  There is NO reference path at this size
    (ties everywhere: which reference labels face a gap is the tie rule's choice), so the ops are held to what needs none: they
    spell both rows, rescore to the closed-form score, and the counts are the op counts.  With free end gaps the path is empty and
    the ops are the closed form: the whole reference, then the whole query"""
    N, M = C.LONGEST
    a, b, score, stats, ops, ops_len = _longest_full_form(free)
    assert score == C.unequal_score(N, M, free) and (ops[ops_len:] == 0).all()
    _check_consistent(a, b, C.UNEQUAL_COSTS, free, score, stats, ops[:ops_len], "longest")
    if free:
        assert np.array_equal(ops[:ops_len], C.unequal_free_ops(N, M))
    else:
        assert ops_len == N and tuple(stats) == (0, M, N - M, N)
    W.check_device_flags()


# ========================================================================================================= the quality profile
def _profile(ops, ref, query, qual, dwell, count_ends):
    ops = np.asarray(ops, dtype=np.uint8)[None]
    alignment = W.PairwiseAlignment(None, None, None, None, None, _dev(ops), _dev(np.array([ops.shape[1]], dtype=np.int32)))
    return W.quality_profile(alignment, _dev(np.array([ref], dtype=np.int32)), _dev(np.array([len(ref)], dtype=np.int32)),
                             _dev(np.array([query], dtype=np.int32)), _dev(np.array([len(query)], dtype=np.int32)), qual=_dev(qual),
                             dwell=_dev(dwell), classes=C.PROFILE_CLASSES, count_ends=count_ends)


@pytest.mark.parametrize("count_ends", [False, True])
def test_profile_of_the_longest_alignments(count_ends):
    """the aligner's own ops at kPaMaxQuery (8192 matches) and at kPaMaxRef (65535 columns), through quality_profile"""
    a, b = C.identical_rows(C.SELF_CLOSED)
    _, _, ops, ops_len = _align([a], [b], R.EMBOSS, True)
    qual, dwell = C.profile_inputs(661, len(b))
    got = _profile(ops[0, :ops_len[0]], a, b, qual, dwell, count_ends)
    _equal(got, C.profile_reference(C.identical_result(C.SELF_CLOSED, R.EMBOSS).ops, a, b, qual, dwell, count_ends), "identical 8192")
    a, b, _, _, ops, ops_len = _longest_full_form(False)
    qual, dwell = C.profile_inputs(662, len(b))
    got = _profile(ops[:ops_len], a, b, qual, dwell, count_ends)
    want = C.profile_reference(ops[:ops_len], a, b, qual, dwell, count_ends)     # of the device's ops: there is no reference path
    assert want["bad"] == 0 and want["read_counts"][0].sum() == ops_len
    _equal(got, want, "longest")
    W.check_device_flags()


@pytest.mark.parametrize("count_ends", [False, True])
@pytest.mark.parametrize("kind", ["longest", "mixed"])
def test_profile_of_synthetic_op_strings_at_both_length_limits(kind, count_ends):
    """65535 reference and 8192 query labels: 73727 columns (no room for a match), and 65727 columns with 8000 aligned ones"""
    ops, ref, query = C.synthetic_ops(kind)
    qual, dwell = C.profile_inputs(663, len(query))
    got = _profile(ops, ref, query, qual, dwell, count_ends)
    _equal(got, C.profile_reference(ops, ref, query, qual, dwell, count_ends), kind)
    W.check_device_flags()
