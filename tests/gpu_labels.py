"""The drivers of the label tools on the device (ctc_forced_align, pairwise_align, demux, read mapping, the read generator's plan,
the quality profile): label lists through the tool, and each result held to the host reference of tests/*_ref.py.
Used by the tools' own files, tests/test_gpu_align_limits.py, test_gpu_tool_limits.py and test_gpu_wave_steps.py.  Nothing here is
rewritten by pytest, so every assert carries its message."""
import numpy as np
import torch

from tests import ctc_align_ref as A
from tests import pairwise_align_ref as R
from tests import readmap_cases as RC
from tests import readmap_ref as RR
from tests.gpu_util import DEV, assert_equal_arrays, dev

INT_MIN = -2 ** 31
PAD = 2 ** 63 - 1
MARGIN = 1e-6               # the margin rule of tests/test_gpu_align.py
MAX_EXCLUDED = 1e-3


def package():
    """the package, imported when a test first asks: collecting a file does not load the library"""
    import wavenet_speech_amd as W
    return W


def decoding():
    from wavenet_speech_amd import decoding
    return decoding


# ---- ctc_forced_align ---------------------------------------------------------------------------------------------------------------

def pad_targets(label_lists, width=None):
    width = max([len(l) for l in label_lists] + [1]) if width is None else width
    out = np.zeros((len(label_lists), width), dtype=np.int64)
    for b, l in enumerate(label_lists):
        out[b, :len(l)] = l
    return torch.tensor(out), torch.tensor([len(l) for l in label_lists])


def forced_align(x, label_lists, input_lengths=None, width=None, **kw):
    """the device result of a batch of label lists as numpy arrays: states, frame_labels, spans, score"""
    targets, tlens = pad_targets(label_lists, width)
    out = package().ctc_forced_align(x.to(DEV), targets, tlens, input_lengths=input_lengths, **kw)
    torch.cuda.synchronize()
    assert out.states.dtype == torch.int32 and out.frame_labels.dtype == torch.int32 and out.spans.dtype == torch.int32, \
        "states %s, frame_labels %s, spans %s" % (out.states.dtype, out.frame_labels.dtype, out.spans.dtype)
    assert out.score.dtype == torch.float32 and out.states.is_cuda and out.spans.shape == (x.shape[0], targets.shape[1], 2), \
        "score %s, states on %s, spans %s" % (out.score.dtype, out.states.device, tuple(out.spans.shape))
    return [v.cpu().numpy() for v in out]


def check_utterance(lp, labels, states, frame_labels, spans, score, exact=False, tag=""):
    """one utterance of a device result against the reference on the fp64 log-probabilities lp [C][Tb]; returns the margins"""
    Tb, L = lp.shape[1], len(labels)
    want_states, want_score, want_spans = A.viterbi_align(lp, labels)
    assert (states[Tb:] == -1).all() and (frame_labels[Tb:] == -1).all() and (spans[L:] == -1).all(), "%s: not -1 past the lengths" % tag
    if not want_score > -np.inf or Tb == 0:
        assert score == np.float32(want_score), (tag, score, want_score)
        assert (states == -1).all() and (frame_labels == -1).all() and (spans == -1).all(), "%s: not -1 where nothing aligns" % tag
        return None
    st = states[:Tb]
    # the outputs agree with each other whatever the path is
    assert_equal_arrays(frame_labels[:Tb], A.frame_labels_of(st, labels), "%s frame_labels of the states" % tag)
    assert_equal_arrays(spans[:L], A.spans_of(st, L), "%s spans of the states" % tag)
    margins = A.frame_margins(lp, labels, want_states)
    if exact:
        assert_equal_arrays(st, want_states, "%s states" % tag)
        assert_equal_arrays(spans[:L], want_spans, "%s spans" % tag)
        assert score == np.float32(want_score), (tag, score, want_score)
        return margins
    clear = margins > MARGIN
    excluded = int((~clear).sum())
    print("%s frames %d labels %d: min margin %.3g, excluded %d, score %.6f (device %.6f)"
          % (tag, Tb, L, margins.min(), excluded, want_score, score))
    assert excluded <= MAX_EXCLUDED * Tb, (tag, excluded, Tb)
    assert_equal_arrays(st[clear], want_states[clear], "%s states at the clear frames" % tag)
    rescored = A.path_score(lp, labels, st)                          # asserts that the path is a legal alignment too
    assert abs(rescored - want_score) <= 1e-9 * abs(want_score), (tag, rescored, want_score)
    assert abs(float(score) - want_score) <= 1e-6 * abs(want_score), (tag, score, want_score)
    return margins


def check_forced_batch(x, label_lists, input_lengths, got, kind="logits", exact=False, tag=""):
    states, frame_labels, spans, score = got
    xs = x.double().numpy()
    out = []
    for b, labels in enumerate(label_lists):
        Tb = x.shape[2] if input_lengths is None else int(input_lengths[b])
        lp = A.to_log_probs(xs[b][:, :Tb], kind)
        out.append(check_utterance(lp, labels, states[b], frame_labels[b], spans[b], score[b], exact, "%s[%d]" % (tag, b)))
    return out


# ---- pairwise_align -----------------------------------------------------------------------------------------------------------------

def pad_rows(rows, width=None, fill=0, dtype=torch.int32):
    width = max([len(r) for r in rows] + [1]) if width is None else width
    out = np.full((len(rows), width), fill, dtype=np.int64)
    for n, r in enumerate(rows):
        out[n, :len(r)] = r
    return torch.tensor(out, dtype=dtype), torch.tensor([len(r) for r in rows], dtype=torch.int32)


def pair_align(refs, queries, costs, free, ref_width=None, query_width=None, fill=0, dtype=torch.int32, return_ops=True):
    """the device result of a batch of label lists as numpy arrays: score in half units (int), stats [B][4], ops, ops_len"""
    a, an = pad_rows(refs, ref_width, fill, dtype)
    b, bn = pad_rows(queries, query_width, fill, dtype)
    out = package().pairwise_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV), match=costs[0] / 2, mismatch=costs[1] / 2,
                                   gap_open=costs[2] / 2, gap_extend=costs[3] / 2, end_gaps_free=free, return_ops=return_ops)
    torch.cuda.synchronize()
    assert out.score.dtype == torch.float32 and out.score.is_cuda and out.matches.dtype == torch.int32, \
        "score %s on %s, matches %s" % (out.score.dtype, out.score.device, out.matches.dtype)
    score2 = (out.score.double() * 2).cpu().numpy()
    assert (score2 == np.round(score2)).all(), "a score that is no half unit: %s" % score2[score2 != np.round(score2)][:4]
    stats = torch.stack([out.matches, out.mismatches, out.gaps, out.length], dim=1).cpu().numpy()
    if not return_ops:
        assert out.ops is None and out.ops_len is None, "ops were returned"
        return score2.astype(np.int64), stats, None, None
    assert out.ops.dtype == torch.uint8 and out.ops.shape == (len(refs), a.shape[1] + b.shape[1]) and out.ops_len.dtype == torch.int32, \
        "ops %s %s, ops_len %s" % (out.ops.dtype, tuple(out.ops.shape), out.ops_len.dtype)
    return score2.astype(np.int64), stats, out.ops.cpu().numpy(), out.ops_len.cpu().numpy()


def check_pair(a, b, costs, free, score, stats, ops, ops_len, tag=""):
    """one pair of a device result: equal to the reference in every number, and consistent in itself"""
    want = R.align(a, b, *costs, free)
    assert score == want.score, (tag, score, want.score)
    assert tuple(stats) == (want.matches, want.mismatches, want.gaps, want.length), (tag, tuple(stats), want[1:5])
    if ops is None:
        return want
    assert ops_len == want.length, (tag, ops_len, want.length)
    got = ops[:ops_len]
    assert_equal_arrays(got, want.ops, "%s ops" % tag)
    assert (ops[ops_len:] == 0).all(), "%s: ops past ops_len" % tag
    # without the reference: both rows come out exactly once, the ops rescore to the score, the counts are the op counts
    assert R.replay(a, b, got) == (list(a), list(b)), "%s: the ops do not spell the two rows" % tag
    assert R.rescore(got, *costs, free) == score, (tag, R.rescore(got, *costs, free), score)
    assert (int((got == 1).sum()), int((got == 2).sum()), int((got >= 3).sum()), len(got)) == tuple(stats), (tag, tuple(stats))
    return want


def check_pair_batch(refs, queries, costs, free, got, tag=""):
    score, stats, ops, ops_len = got
    return [check_pair(a, b, costs, free, int(score[n]), stats[n], None if ops is None else ops[n],
                       None if ops is None else int(ops_len[n]), "%s[%d]" % (tag, n)) for n, (a, b) in enumerate(zip(refs, queries))]


# ---- demux ----------------------------------------------------------------------------------------------------------------------------

def kit(case):
    ends = [0] * case.n_front + [1] * (len(case.group) - case.n_front)
    return package().BarcodeSet.from_table(case.patterns, case.pattern_lengths, ends, case.group)


def kw(case):
    return dict(zip(("match", "mismatch", "gap_open", "gap_extend"), (c / 2.0 for c in case.costs)), window=case.window)


def assert_scores(got, ref):
    assert got.score.dtype == torch.float32 and got.start.dtype == torch.int32 and got.end.dtype == torch.int32, \
        "score %s, start %s, end %s" % (got.score.dtype, got.start.dtype, got.end.dtype)
    assert_equal_arrays(got.score.cpu().numpy().astype(np.float64) * 2.0, ref["score"].astype(np.float64), "score")
    assert_equal_arrays(got.start.cpu().numpy(), ref["start"], "start")
    assert_equal_arrays(got.end.cpu().numpy(), ref["end"], "end")


def assert_pick(got, want):
    for name in ("barcode", "trim", "hits", "runner_up"):
        t = getattr(got, name)
        assert t.dtype == torch.int32, "%s is %s" % (name, t.dtype)
        assert_equal_arrays(t.cpu().numpy(), want[name], name)


# ---- read mapping and the read generator ------------------------------------------------------------------------------------------------

def assert_index(index, ref, k, w):
    want = [(c << 28) | (p << 1) | s for c, p, s in RR.index_ref(ref, k, w)]
    assert index.n_entries == len(want), "%d index entries, expected %d" % (index.n_entries, len(want))
    assert_equal_arrays(index.entries[:index.n_entries].cpu().numpy(), np.array(want, dtype=np.int64), "index entries")
    assert (index.R, index.k, index.w) == (len(ref), k, w) and index.bases.tolist() == list(ref), "R, k, w or the bases of the index"


def assert_seeds(ref, reads, k, w, max_occ, cap, width=None):
    """seed_anchors of the reads against the index of `ref`: the sorted kept keys and the three counts -> (Anchors, [(kept,
    minimizers, truncated)])"""
    index = package().read_index(ref, k=k, w=w, device=DEV)
    assert_index(index, ref, k, w)
    labels, lengths = RC.rows(reads, width)
    got = package().seed_anchors(dev(labels), dev(lengths), index, max_occ=max_occ, anchors_per_read=cap)
    host = RR.index_ref(ref, k, w)
    keys = np.full((len(reads), cap), PAD, dtype=np.int64)
    want = []
    for b, read in enumerate(reads):
        anchors, n_min, trunc = RR.anchors_ref(read, host, k, w, max_occ, cap)
        keys[b, :len(anchors)] = sorted(RR.pack(a) for a in anchors)
        want.append((len(anchors), n_min, trunc))
    assert got.keys.dtype == torch.int64, "keys are %s" % got.keys.dtype
    assert_equal_arrays(got.keys.cpu().numpy(), keys, "keys")
    counts = [got.n_anchors.tolist(), got.n_minimizers.tolist(), got.truncated.tolist()]
    assert counts == [list(c) for c in zip(*want)], "n_anchors, n_minimizers, truncated: %s, expected %s" % (counts, [list(c) for c in zip(*want)])
    assert all(t.dtype == torch.int32 for t in (got.n_anchors, got.n_minimizers, got.truncated)), "a count that is not int32"
    return got, want


def plan_given(bases, base_lengths, dwell, window, max_dwell=1 << 14, dwell_model=("fixed", 1)):
    """wn_reads_plan on given bases / lengths / dwell (CPU tensors, [B, n] / [B] / [B, K]); any of them may be None"""
    from wavenet_speech_amd import synthetic as S

    def rows(x, width):
        out = torch.zeros(x.shape[0], width, dtype=torch.int32, device=DEV)
        out[:, :x.shape[1]] = x.to(DEV)
        return out

    B = (bases if bases is not None else dwell if dwell is not None else base_lengths).shape[0]
    nmax = bases.shape[1] if bases is not None else int(base_lengths.max())
    mb = nmax + 1
    return S.hip_reads_plan(B, 5 + 2 * window, mb, window, dwell_model, max_dwell, 17, DEV,
                            None if bases is None else rows(bases, mb),
                            None if base_lengths is None else base_lengths.to(device=DEV, dtype=torch.int32),
                            None if dwell is None else rows(dwell, mb))


# ---- quality_profile ------------------------------------------------------------------------------------------------------------------

PROFILE_TABLES = ("q_counts", "dwell_counts", "confusion")
PROFILE_FIELDS = PROFILE_TABLES + ("read_counts", "outcome", "ref_index")


def assert_profile(got, want, what):
    """a QualityProfile against the reference's dict, field by field; a field the reference leaves None must be None"""
    assert isinstance(got, package().QualityProfile), "%s: %s" % (what, type(got))
    for name, dtype in zip(PROFILE_FIELDS, (torch.int64,) * 3 + (torch.int32, torch.uint8, torch.int32)):
        t = getattr(got, name)
        if want[name] is None:
            assert t is None, (what, name)
            continue
        assert t.is_cuda and t.dtype == dtype, (what, name, t.device, t.dtype)
        assert_equal_arrays(t.cpu().numpy(), want[name], "%s %s" % (what, name))
