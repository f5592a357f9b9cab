"""GPU: the quality profile (csrc/wn_profile.hip through wavenet_speech_amd.quality_profile), the calibration fit and
Basecaller.calibrate against the loop reference of tests/quality_profile_ref.py.  Every output of the kernel is an integer, so
EVERYTHING is compared for exact equality; only the fit has a tolerance (1e-9 relative: float64 on both sides over at most 94
bins, rounding alone is about 1e-13, the rest is slack for the two log10 implementations).  The inputs and their references are
built once in tests/quality_profile_cases.py; the op strings there are random walks, not the aligner's output."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import quality_profile_cases as PC
from tests import quality_profile_ref as PR
from tests.gpu_labels import PROFILE_TABLES as TABLES, assert_profile as _equal
from tests.gpu_util import DEV, basecall_model as _model, dev as _dev, same as _same

pytestmark = pytest.mark.gpu


def _alignment(batch):
    """a PairwiseAlignment that carries the batch's ops; the other fields are not looked at by quality_profile"""
    ops, ops_len = _dev(batch.ops), _dev(batch.ops_len)
    return W.PairwiseAlignment(None, None, None, None, ops_len, ops, ops_len)


def _run(batch, count_ends, qual=True, dwell=True, into=None, views=None):
    """views: tensors that go in instead of the batch's own ref / query / qual / dwell"""
    args = dict(ref=_dev(batch.ref), query=_dev(batch.query), qual=_dev(batch.qual) if qual else None,
                dwell=_dev(batch.dwell) if dwell else None)
    args.update(views or {})
    return W.quality_profile(_alignment(batch), args["ref"], _dev(batch.ref_len), args["query"], _dev(batch.query_len),
                             qual=args["qual"], dwell=args["dwell"], classes=batch.classes, count_ends=count_ends, into=into)


@pytest.mark.parametrize("count_ends", [False, True])
@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_against_the_reference(name, count_ends):
    batch = PC.case(name)
    got = _run(batch, count_ends)
    _equal(got, PC.reference(name, count_ends), name)
    counts = got.read_counts.long()
    assert torch.equal(counts.sum(1), _dev(batch.ops_len).long())    # the five counts sum to ops_len
    assert int(got.q_counts.sum()) == int(got.dwell_counts.sum()) == int(counts[:, :3].sum())
    assert int(got.confusion.sum()) == int(counts[:, :4].sum())
    assert _same(got, _run(batch, count_ends))                       # two runs are bitwise equal
    W.check_device_flags()


@pytest.mark.parametrize("qual,dwell", [(True, False), (False, True), (False, False)])
def test_optional_inputs(qual, dwell):
    for name in ("edges_c5", "special_c64"):
        got = _run(PC.case(name), False, qual=qual, dwell=dwell)
        _equal(got, PC.reference(name, False, qual, dwell), name)
        assert (got.q_counts is None) == (not qual) and (got.dwell_counts is None) == (not dwell)
    W.check_device_flags()


def test_row_strided_and_int64_views():
    batch = PC.case("edges_c5")
    want = PC.reference("edges_c5", True)

    def wide(a, fill):
        t = torch.full((a.shape[0], a.shape[1] + 7), fill, dtype=torch.from_numpy(a).dtype, device=DEV)
        t[:, :a.shape[1]] = _dev(a)
        return t[:, :a.shape[1]]
    views = dict(ref=wide(batch.ref, 99), query=wide(batch.query, 99), qual=wide(batch.qual, 200), dwell=wide(batch.dwell, -9))
    assert all(v.stride(0) == v.shape[1] + 7 and not v.is_contiguous() for v in views.values())
    _equal(_run(batch, True, views=views), want, "row-strided")
    _equal(_run(batch, True, views=dict(ref=_dev(batch.ref).long(), query=wide(batch.query.astype(np.int64), 99))), want, "int64")
    ops = torch.zeros(len(batch.ops), batch.ops.shape[1] + 5, dtype=torch.uint8, device=DEV)       # and a row-strided ops view
    ops[:, :batch.ops.shape[1]] = _dev(batch.ops)
    alignment = W.PairwiseAlignment(None, None, None, None, None, ops[:, :batch.ops.shape[1]], _dev(batch.ops_len))
    got = W.quality_profile(alignment, _dev(batch.ref), _dev(batch.ref_len), _dev(batch.query), _dev(batch.query_len),
                            qual=_dev(batch.qual), dwell=_dev(batch.dwell), count_ends=True)
    _equal(got, want, "ops view")
    W.check_device_flags()


def test_into_accumulates_and_adds_in_64_bits():
    a, b = PC.case("edges_c5_b4"), PC.case("special_c5")
    ra, rb = PC.reference("edges_c5_b4", False), PC.reference("special_c5", False)
    first = _run(a, False)
    kept = [getattr(first, name) for name in TABLES]
    both = _run(b, False, into=first)
    for name, t in zip(TABLES, kept):
        assert getattr(both, name) is t                              # accumulated in place
        assert np.array_equal(t.cpu().numpy(), ra[name] + rb[name])
    assert np.array_equal(both.read_counts.cpu().numpy(), rb["read_counts"])       # the per-read fields are replaced
    assert np.array_equal(both.outcome.cpu().numpy(), rb["outcome"])
    # an entry preset to 2^32 - 1 comes back right: a 32-bit add would wrap
    preset = W.QualityProfile(*[torch.full_like(t, 2 ** 32 - 1) for t in kept], None, None, None)
    got = _run(a, False, into=preset)
    for name in TABLES:
        assert int(ra[name].max()) > 0
        assert np.array_equal(getattr(got, name).cpu().numpy(), ra[name] + (2 ** 32 - 1)), name
    with pytest.raises(ValueError, match="into"):                    # a table without its input, a table of another shape
        _run(a, False, qual=False, into=first)
    with pytest.raises(ValueError, match="into"):
        _run(PC.case("edges_c64"), False, into=first)
    W.check_device_flags()


@pytest.mark.parametrize("count_ends", [False, True])
def test_bad_reads_are_cleared_and_counted_and_their_neighbours_are_right(count_ends):
    good, mixed, bad_rows = PC.bad_batches()
    want_good, want = good.reference(count_ends), mixed.reference(count_ends)
    assert want["bad"] == len(bad_rows) == 8
    got = _run(mixed, count_ends)
    with pytest.raises(RuntimeError, match=r"quality_profile: 8 pair"):
        W.check_device_flags()
    _equal(got, want, "mixed")                                       # every neighbour is right
    for name in TABLES:                                              # the tables are those of the batch without the bad reads
        assert np.array_equal(getattr(got, name).cpu().numpy(), want_good[name]), name
    rows = torch.tensor(bad_rows, device=DEV)
    assert bool((got.read_counts[rows] == -1).all()) and not bool(got.outcome[rows].any()) and bool((got.ref_index[rows] == -1).all())
    _equal(_run(good, count_ends), want_good, "good")
    W.check_device_flags()                                           # the flag was consumed: nothing is left over


def _pairs():
    (truth, truth_len), (calls, calls_len) = PC.mutated_pairs()
    return _dev(truth), _dev(truth_len), _dev(calls), _dev(calls_len)


@pytest.mark.parametrize("end_gaps_free", [True, False])
def test_end_to_end_through_the_aligner(end_gaps_free):
    truth, truth_len, calls, calls_len = _pairs()
    al = W.pairwise_align(truth, truth_len, calls, calls_len, end_gaps_free=end_gaps_free)
    p = W.quality_profile(al, truth, truth_len, calls, calls_len, count_ends=True)
    assert p.q_counts is None and p.dwell_counts is None
    assert torch.equal(p.read_counts[:, 0], al.matches) and torch.equal(p.read_counts[:, 1], al.mismatches)
    assert torch.equal(p.read_counts[:, 2] + p.read_counts[:, 3], al.gaps) and not bool(p.read_counts[:, 4].any())
    assert int(al.mismatches.sum()) > 0 and int(al.gaps.sum()) > 0
    want = PR.profile(al.ops.cpu().numpy(), al.ops_len.cpu().numpy(), truth.cpu().numpy(), truth_len.cpu().numpy(),
                      calls.cpu().numpy(), calls_len.cpu().numpy(), classes=5, count_ends=True)
    _equal(p, want, "aligned, count_ends")
    q = W.quality_profile(al, truth, truth_len, calls, calls_len)    # the default: heads and tails are left out
    want = PR.profile(al.ops.cpu().numpy(), al.ops_len.cpu().numpy(), truth.cpu().numpy(), truth_len.cpu().numpy(),
                      calls.cpu().numpy(), calls_len.cpu().numpy(), classes=5, count_ends=False)
    _equal(q, want, "aligned")
    assert torch.equal(q.read_counts[:, :2], p.read_counts[:, :2]) and int(q.read_counts[:, 4].sum()) > 0
    assert torch.equal(q.read_counts.sum(1).int(), al.length)
    rates = q.rates.cpu().numpy()
    c = want["read_counts"].astype(np.float64)
    assert np.allclose(rates, np.stack([c[:, 1], c[:, 2], c[:, 3], c[:, 0]], 1) / c[:, :4].sum(1, keepdims=True), rtol=1e-15)
    sub = q.substitution_rates.cpu().numpy()[1:]                     # label 0 never occurs in these reads
    assert np.allclose(sub.sum(1), 1.0) and (sub.argmax(1) == np.arange(1, 5)).all()      # most bases are called as themselves
    W.check_device_flags()


def test_a_poisoned_pair_of_the_aligner_is_a_bad_read():
    truth, truth_len, calls, calls_len = _pairs()
    truth_len = truth_len.clone()
    truth_len[2] = truth.shape[1] + 1
    al = W.pairwise_align(truth, truth_len, calls, calls_len)
    with pytest.raises(RuntimeError, match="pairwise_align"):
        W.check_device_flags()
    p = W.quality_profile(al, truth, truth_len, calls, calls_len)
    with pytest.raises(RuntimeError, match=r"quality_profile: 1 pair"):
        W.check_device_flags()
    assert p.read_counts[2].tolist() == [-1] * 5 and not bool(p.outcome[2].any())
    keep = [0, 1, 3, 4, 5]
    ok = W.quality_profile(W.pairwise_align(truth[keep], truth_len[keep], calls[keep], calls_len[keep]), truth[keep], truth_len[keep],
                           calls[keep], calls_len[keep])
    assert torch.equal(p.confusion, ok.confusion) and torch.equal(p.read_counts[keep], ok.read_counts)
    W.check_device_flags()


@pytest.mark.parametrize("decode", ["greedy", "beam"])
def test_basecaller_calibrate_equals_the_direct_calls(decode):
    g = torch.Generator().manual_seed(23)
    signal = torch.randn(2, 150, generator=g).to(DEV)
    n = torch.tensor([150, 97])
    bc = W.Basecaller(_model(), chunk=32, batch=4)
    out = bc(signal, n, decode=decode, **(dict(beam_width=4) if decode == "beam" else {}))
    truth = torch.randint(1, 5, (2, 60), generator=g).to(DEV)
    truth_len = torch.tensor([60, 41], dtype=torch.int32, device=DEV)
    prof = bc.calibrate(out, truth, truth_len)
    labels, lengths = (out.labels[:, 0], out.label_lengths[:, 0]) if decode == "beam" else (out.labels, out.label_lengths)
    assert int(lengths.sum()) > 0
    q = bc.qualities(out)
    al = W.pairwise_align(truth, truth_len, labels, lengths)
    direct = W.quality_profile(al, truth, truth_len, labels, lengths, qual=q.qual, dwell=q.dwell, classes=5)
    assert isinstance(prof, W.QualityProfile) and _same(prof, direct)
    assert int(prof.q_counts.sum()) == int(prof.read_counts[:, :3].sum()) > 0
    again = bc.calibrate(out, truth, truth_len, into=prof, gap_open=5, end_gaps_free=False)      # align_kw pass through
    other = W.quality_profile(W.pairwise_align(truth, truth_len, labels, lengths, gap_open=5, end_gaps_free=False), truth, truth_len,
                              labels, lengths, qual=q.qual, dwell=q.dwell, classes=5)
    assert again.q_counts is prof.q_counts and torch.equal(again.confusion, direct.confusion + other.confusion)
    assert torch.equal(again.read_counts, other.read_counts)
    with pytest.raises(ValueError, match="return_ops"):              # the profile walks the ops
        bc.calibrate(out, truth, truth_len, return_ops=False)
    W.check_device_flags()


def test_fit_on_the_device_against_numpy():
    tables = [PR.planted_table(a, b) for a, b in ((0.8, 3.0), (1.0, 0.0), (0.55, 6.5))]
    rng = np.random.default_rng(41)                                  # and a noisy table with uneven bins, some below min_count
    noisy = np.zeros((94, 3), dtype=np.int64)
    for q in range(2, 60):
        n = int(rng.integers(50, 100000))
        err = rng.binomial(n, min(0.9, 10.0 ** (-(0.7 * q + 2.0) / 10.0)))
        ins = rng.binomial(err, 0.3)
        noisy[q] = (n - err, err - ins, ins)
    for table in tables + [noisy]:
        want = PR.fit(table, min_count=100)
        cal = W.fit_quality_calibration(_dev(table), min_count=100)
        rel = (abs(cal.qscale - want[0]) / abs(want[0]), abs(cal.qbias - want[1]) / abs(want[1]) if want[1] else abs(cal.qbias))
        print("fit: slope %.12g (numpy %.12g), intercept %.12g (numpy %.12g), relative %.2e / %.2e" % (cal.qscale, want[0], cal.qbias, want[1], *rel))
        assert max(rel) <= 1e-9
        assert (cal.bins_used, cal.bases_used) == want[2:4]
        assert cal.q_empirical.is_cuda and cal.q_empirical.dtype == torch.float64
        emp = cal.q_empirical.cpu().numpy()
        used = ~np.isnan(want[4])
        assert np.array_equal(np.isnan(emp), ~used) and np.abs(emp[used] / want[4][used] - 1.0).max() <= 1e-9
    # the loop a user writes: the fitted line goes into the qualities
    cal = W.fit_quality_calibration(_dev(tables[0]))
    x = torch.randn(2, 5, 40, generator=torch.Generator().manual_seed(5)).to(DEV)
    labels, lengths, frames = W.ctc_greedy_decode(x)
    raw = W.ctc_base_qualities(x, labels, lengths, frames)
    fitted = W.ctc_base_qualities(x, labels, lengths, frames, qscale=cal.qscale, qbias=cal.qbias)
    assert torch.equal(raw.error.view(torch.int32), fitted.error.view(torch.int32)) and not torch.equal(raw.qual, fitted.qual)
    W.check_device_flags()


def test_what_cannot_be_profiled_raises():
    batch = PC.case("edges_c5_b4")
    al = _alignment(batch)
    ref, ref_len, query, query_len = _dev(batch.ref), _dev(batch.ref_len), _dev(batch.query), _dev(batch.query_len)
    qual, dwell = _dev(batch.qual), _dev(batch.dwell)
    for kw in (dict(ref=ref.cpu()), dict(query=query.cpu()), dict(qual=qual.cpu()), dict(dwell=dwell.cpu())):
        args = dict(ref=ref, query=query, qual=qual, dwell=dwell)
        args.update(kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            W.quality_profile(al, args["ref"], ref_len, args["query"], query_len, qual=args["qual"], dwell=args["dwell"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.quality_profile(W.PairwiseAlignment(None, None, None, None, None, al.ops.cpu(), al.ops_len.cpu()), ref, ref_len, query, query_len)
    no_ops = W.PairwiseAlignment(None, None, None, None, None, None, None)
    for wrong in (no_ops, (al.ops, al.ops_len), None):
        with pytest.raises(ValueError, match="PairwiseAlignment"):
            W.quality_profile(wrong, ref, ref_len, query, query_len)
    for kw in (dict(classes=0), dict(classes=65), dict(qual=qual.int()), dict(dwell=dwell.long()), dict(qual=qual[:, :-1]),
               dict(dwell=dwell[:2]), dict(into="tables")):
        with pytest.raises(ValueError):
            W.quality_profile(al, ref, ref_len, query, query_len, **kw)
    with pytest.raises(ValueError):
        W.quality_profile(al, ref[:3], ref_len[:3], query, query_len)
    with pytest.raises(ValueError):
        W.quality_profile(al, ref.float(), ref_len, query, query_len)
    with pytest.raises(ValueError):
        W.quality_profile(W.PairwiseAlignment(None, None, None, None, None, al.ops.int(), al.ops_len), ref, ref_len, query, query_len)
    _equal(W.quality_profile(al, ref, ref_len, query, query_len, qual=qual, dwell=dwell), PC.reference("edges_c5_b4", False), "after all")
    W.check_device_flags()
