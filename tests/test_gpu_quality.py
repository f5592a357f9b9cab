"""GPU: per-base qualities (csrc/wn_quality.hip through wavenet_speech_amd.decoding.ctc_base_qualities) against the float64
reference of tests/ctc_quality_ref.py on the greedy decoder's own output, on a beam path, on bad input, and end to end from
Basecaller to FASTQ text.  The inputs and their references are built once in tests/ctc_quality_cases.py.

Bounds (none of them measured from the kernel): dwell is an integer and must be equal.  error and read_error are within the
relative (2 D + 2 C + 16) 2^-24 of tests/ctc_quality_cases.error_bound, D computed from each input.  qual must be equal
wherever the reference Q is further than 1e-3 from a rounding boundary: an error within that relative bound moves Q by at most
10 / ln 10 * bound < 2e-5.  tests/test_ctc_quality_ref.py holds the share of excluded bases below 1 % for every input."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import ctc_decode_ref as DR
from tests import ctc_quality_cases as QC
from tests import ctc_quality_ref as QR
from tests.gpu_util import DEV, basecall_model as _model, bits as _bits, same_bits as _same

pytestmark = pytest.mark.gpu


def _check(got, ref, valid, near, bound, what):
    """got: BaseQualities; ref: the dict of batch_qualities; prints every figure before it asserts"""
    error, qual, dwell = got.error.cpu().numpy(), got.qual.cpu().numpy(), got.dwell.cpu().numpy()
    read_error = got.read_error.cpu().numpy()
    assert error.dtype == np.float32 and qual.dtype == np.uint8 and dwell.dtype == np.int32 and read_error.dtype == np.float32
    assert np.array_equal(dwell, ref["dwell"])
    ok = valid & ~np.isnan(ref["error"])
    assert np.array_equal(np.isnan(error), ~ok)                      # NaN exactly at bad bases and past the lengths
    rel = np.abs(error[ok].astype(np.float64) - ref["error"][ok]) / ref["error"][ok] if ok.any() else np.zeros(1)
    live = ~np.isnan(ref["read_error"])
    assert np.array_equal(np.isnan(read_error), ~live)
    rrel = np.abs(read_error[live].astype(np.float64) - ref["read_error"][live]) / ref["read_error"][live] if live.any() else np.zeros(1)
    sure = valid & ~near
    print("%s: error rel %.3e, read_error rel %.3e (allowed %.3e); qual compared on %d of %d bases, %d differ"
          % (what, rel.max(), rrel.max(), bound, int(sure.sum()), int(valid.sum()), int((qual != ref["qual"])[sure].sum())))
    assert rel.max() <= bound and rrel.max() <= bound
    assert int(near.sum()) <= 0.01 * int(valid.sum())
    assert np.array_equal(qual[sure], ref["qual"][sure])
    assert not qual[~valid].any()


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_against_the_reference_on_the_greedy_path(name):
    c = QC.case(name)
    x = torch.from_numpy(c.x).to(DEV)
    if c.layout == "BTC":
        x = x.transpose(1, 2).contiguous()
    in_len = torch.from_numpy(c.input_lengths)
    labels, lengths, frames = W.ctc_greedy_decode(x, input_lengths=in_len, layout=c.layout)
    assert labels.shape == (QC.B, c.T)                               # Lmax = T
    assert np.array_equal(labels.cpu().numpy(), c.labels) and np.array_equal(frames.cpu().numpy(), c.frames)
    assert np.array_equal(lengths.cpu().numpy(), c.lengths)
    kw = dict(input_lengths=in_len, input=c.kind, layout=c.layout, stat=c.stat, qscale=c.qscale, qbias=c.qbias)
    got = W.ctc_base_qualities(x, labels, lengths, frames, **kw)
    assert all(t.is_cuda for t in got)
    _check(got, c.ref, c.valid(), c.near_boundary(), QC.error_bound(c.D), name)
    want_q = c.qscale * (-10.0 * np.log10(c.ref["read_error"])) + c.qbias
    live = ~np.isnan(want_q)
    mean_q = got.mean_qscore.cpu().numpy()
    assert np.array_equal(np.isnan(mean_q), ~live)
    assert np.abs(mean_q[live] - want_q[live]).max(initial=0.0) <= 1e-4 * (1.0 + np.abs(want_q[live]).max(initial=0.0))
    again = W.ctc_base_qualities(x, labels, lengths, frames, **kw)   # two runs are bitwise identical in all outputs
    assert _same(got, again)
    W.check_device_flags()


def test_both_stats_agree_where_a_run_is_one_frame():
    c, best = QC.case("peaked_T1000"), QC.case("peaked_T1000_best")
    x = torch.from_numpy(c.x).to(DEV)
    args = [torch.from_numpy(a).to(DEV) for a in (c.labels.astype(np.int32), c.lengths, c.frames.astype(np.int32))]
    mean = W.ctc_base_qualities(x, *args, input_lengths=torch.from_numpy(c.input_lengths), stat="mean")
    least = W.ctc_base_qualities(x, *args, input_lengths=torch.from_numpy(best.input_lengths), stat="best")
    one = mean.dwell == 1
    assert bool(one.any()) and torch.equal(mean.error[one], least.error[one]) and torch.equal(mean.dwell, least.dwell)
    longer = mean.dwell > 1
    assert bool((least.error[longer] <= mean.error[longer]).all()) and bool((least.error[longer] < mean.error[longer]).any())
    W.check_device_flags()


def test_a_beam_path_through_strided_views():
    """the best beam of a beam search, passed as the views labels[:, 0], frames[:, 0]: its emission frames need not be argmax
    frames, and the run still holds them"""
    T = 200
    x_h, in_len = QC.random_logits(77, T)
    x = torch.from_numpy(x_h).to(DEV)
    labels, lengths, _scores, frames = W.ctc_beam_decode(x, beam_width=4, input_lengths=torch.from_numpy(in_len))
    lab, frm, n = labels[:, 0], frames[:, 0], lengths[:, 0]
    assert lab.stride(0) == 4 * T and not lab.is_contiguous()
    got = W.ctc_base_qualities(x, lab, n, frm, input_lengths=torch.from_numpy(in_len))
    lab_h, frm_h, n_h = lab.cpu().numpy(), frm.cpu().numpy(), n.cpu().numpy()
    off_argmax = sum(1 for b in range(QC.B) for j in range(int(n_h[b])) if QR.frame_argmax(x_h[b, :, frm_h[b, j]]) != lab_h[b, j])
    assert off_argmax > 0                                            # the case this test exists for
    ref = QR.batch_qualities(x_h, lab_h, frm_h, n_h, in_len)
    assert ref["bad"] == 0
    valid = np.arange(T)[None, :] < n_h[:, None]
    with np.errstate(invalid="ignore"):
        near = valid & (np.abs(ref["Q"] - np.floor(ref["Q"]) - 0.5) <= QC.NEAR)
    D = float((x_h.astype(np.float64).max(axis=1) - x_h.astype(np.float64).min(axis=1)).max())
    _check(got, ref, valid, near, QC.error_bound(D), "beam path (%d emission frames off the argmax)" % off_argmax)
    same = W.ctc_base_qualities(x, lab.contiguous(), n.contiguous(), frm.contiguous(), input_lengths=torch.from_numpy(in_len))
    assert _same(got, same)
    W.check_device_flags()


def test_bad_rows_are_poisoned_and_counted_and_their_neighbours_are_right():
    T = 257
    x_h, in_len = QC.peaked_logits(58, T, batch=7)
    in_len[:] = [T, T, T - 20, T, T, T, T]
    labels, frames, lengths = DR.greedy_decode_batch(x_h, input_lengths=in_len)
    labels, frames, lengths = labels.astype(np.int32), frames.astype(np.int32), lengths.astype(np.int32)
    assert min(int(lengths[b]) for b in (0, 1, 2, 4, 5, 6)) >= 6
    labels[0, 3] = 0                                                 # a label equal to the blank
    labels[1, 0] = 99                                                # a label outside [0, C)
    frames[2, lengths[2] - 1] = in_len[2]                            # a frame at T_b < T, inside the tensor
    frames[4, 5] = frames[4, 4]                                      # two equal frames
    lengths[5] = T + 1                                               # a length of Lmax + 1
    ref = QR.batch_qualities(x_h, labels, frames, lengths, in_len)
    assert ref["bad"] == 5                                           # four bases and one read; rows 3 (empty) and 6 are intact
    assert np.isnan(ref["read_error"][[0, 1, 2, 3, 4, 5]]).all() and np.isfinite(ref["read_error"][6])
    x = torch.from_numpy(x_h).to(DEV)
    got = W.ctc_base_qualities(x, torch.from_numpy(labels).to(DEV), torch.from_numpy(lengths).to(DEV), torch.from_numpy(frames).to(DEV),
                               input_lengths=torch.from_numpy(in_len))
    with pytest.raises(RuntimeError, match=r"ctc_base_qualities: 5 base"):
        W.check_device_flags()
    valid = (np.arange(T)[None, :] < lengths[:, None]) & (lengths[:, None] <= T)
    with np.errstate(invalid="ignore"):
        near = valid & (np.abs(ref["Q"] - np.floor(ref["Q"]) - 0.5) <= QC.NEAR)
    D = float((x_h.astype(np.float64).max(axis=1) - x_h.astype(np.float64).min(axis=1)).max())
    _check(got, ref, valid, near, QC.error_bound(D), "bad rows")
    for b, j in ((0, 3), (1, 0), (2, int(lengths[2]) - 1), (4, 5)):
        assert np.isnan(got.error[b, j].item()) and got.qual[b, j].item() == 0 and got.dwell[b, j].item() == 0
        assert bool((got.dwell[b, :int(lengths[b])] > 0).sum() == int(lengths[b]) - 1)       # every other base of the row is served
    assert bool(torch.isnan(got.error[5]).all()) and not bool(got.qual[5].any()) and not bool(got.dwell[5].any())
    W.check_device_flags()                                           # the flag was consumed: nothing is left over


@pytest.mark.parametrize("softmax", [False, True])
def test_basecaller_qualities_equal_the_direct_call_and_fastq_round_trips(softmax):
    g = torch.Generator().manual_seed(23)
    signal = torch.randn(2, 150, generator=g).to(DEV)
    n = torch.tensor([150, 97])
    bc = W.Basecaller(_model(softmax), chunk=32, batch=4)
    out = bc(signal, n, decode="greedy")
    q = bc.qualities(out)
    direct = W.ctc_base_qualities(out.logits, out.labels, out.label_lengths, out.frames, input_lengths=out.frame_lengths,
                                  input="probs" if softmax else "logits")
    assert isinstance(q, W.BaseQualities) and _same(q, direct)
    assert int(out.label_lengths.sum()) > 0 and bool((q.dwell.sum(1) > 0).any())
    if softmax:                                                      # read as logits the probabilities give another answer
        other = W.ctc_base_qualities(out.logits, out.labels, out.label_lengths, out.frames, input_lengths=out.frame_lengths)
        assert not torch.equal(_bits(other.error), _bits(q.error))
    assert _same(bc.qualities(out, stat="best", qscale=0.7, qbias=2.5),
                 W.ctc_base_qualities(out.logits, out.labels, out.label_lengths, out.frames, input_lengths=out.frame_lengths,
                                      input="probs" if softmax else "logits", stat="best", qscale=0.7, qbias=2.5))
    beam = bc(signal, n, decode="beam", beam_width=4)
    assert _same(bc.qualities(beam), W.ctc_base_qualities(beam.logits, beam.labels[:, 0], beam.label_lengths[:, 0], beam.frames[:, 0],
                                                          input_lengths=beam.frame_lengths, input="probs" if softmax else "logits"))
    with pytest.raises(ValueError, match="no logits"):
        bc.qualities(bc(signal, n, decode="greedy", want_logits=False))
    with pytest.raises(ValueError, match="no labels"):
        bc.qualities(bc(signal, n))
    # FASTQ: SEQ is labels_to_strings' text, QUAL - 33 is qual
    records = W.fastq_records(["read_a", "read_b"], out.labels, out.label_lengths, q.qual)
    seqs = W.labels_to_strings(out.labels, out.label_lengths)
    for b, (rec, name) in enumerate(zip(records, ("read_a", "read_b"))):
        head, seq, plus, quals, tail = rec.split("\n")
        assert (head, seq, plus, tail) == ("@" + name, seqs[b], "+", "")
        assert [ord(ch) - 33 for ch in quals] == q.qual[b, :int(out.label_lengths[b])].tolist()
    W.check_device_flags()


def test_an_empty_read_prints_empty_lines():
    labels = torch.tensor([[0, 0, 0], [1, 4, 0]], dtype=torch.int32, device=DEV)
    qual = torch.tensor([[0, 0, 0], [0, 93, 7]], dtype=torch.uint8, device=DEV)
    assert W.fastq_records(["e", "f"], labels, torch.tensor([0, 2]), qual) == ["@e\n\n+\n\n", "@f\nAT\n+\n!~\n"]


def test_what_cannot_be_scored_raises():
    x = torch.zeros(2, 5, 8)
    labels, frames, lengths = torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.ctc_base_qualities(x, labels.to(DEV), lengths.to(DEV), frames.to(DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.ctc_base_qualities(x.to(DEV), labels, lengths.to(DEV), frames.to(DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.ctc_base_qualities(x.to(DEV), labels.to(DEV), lengths.to(DEV), frames)
    xd, ld, fd, nd = x.to(DEV), labels.to(DEV), frames.to(DEV), lengths.to(DEV)
    for kw in (dict(stat="median"), dict(input="odds"), dict(layout="TBC"), dict(qscale=0.0), dict(qscale=float("nan")),
               dict(qbias=float("inf")), dict(blank=5), dict(blank=-1)):
        with pytest.raises(ValueError):
            W.ctc_base_qualities(xd, ld, nd, fd, **kw)
    with pytest.raises(ValueError):
        W.ctc_base_qualities(xd, torch.zeros(2, 9, dtype=torch.int32, device=DEV), nd, torch.zeros(2, 9, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        W.ctc_base_qualities(xd, ld, nd, fd[:, :7])
    with pytest.raises(ValueError):
        W.ctc_base_qualities(xd, ld.float(), nd, fd)
    got = W.ctc_base_qualities(xd, ld, nd, fd)                        # and the call itself is fine: two empty reads
    assert bool(torch.isnan(got.read_error).all()) and bool(torch.isnan(got.mean_qscore).all()) and not bool(got.dwell.any())
    W.check_device_flags()
