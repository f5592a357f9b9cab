"""GPU: read normalisation (wavenet_speech_amd/normalise.py, csrc/wn_select.hip).  The selection kernels are held to np.sort
for exact equality on ragged batches whose padding is extreme garbage, on value patterns that exercise every digit, in deviation
mode and on refused input; med / MAD, quantiles and (scale, shift) to the numpy restatement tests/read_stats_ref.py; two calls to
bitwise equality, a captured graph to the eager results, and Basecaller(normalise=...) to the explicit scale / shift call."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import read_stats_cases as C
from tests import read_stats_ref as R
from tests.gpu_util import DEV, dev as _dev
from wavenet_speech_amd import normalise as N
from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet

pytestmark = pytest.mark.gpu
T = N.TILE
LINEAR_BOUND = 2.0 ** -22          # "linear" quantiles and 1 / (1.4826 mad): see tests/test_read_stats_ref.py and the docstrings below


def _select(x, lengths, ranks, centers=None, bad=None):
    out = N.read_order_statistics(_dev(x), _dev(np.asarray(lengths, dtype=np.int32)), _dev(np.asarray(ranks, dtype=np.int32)),
                                  center=None if centers is None else _dev(centers), bad=bad)
    return out.cpu().numpy()


def _same(got, want):
    np.testing.assert_array_equal(np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32))     # NaN equals NaN


_SORTED = {}


def _sorted(name, x, lengths, centers=None):
    if name not in _SORTED:
        _SORTED[name] = C.sorted_reads(x, lengths, centers)
    return _SORTED[name]


# ---- order statistics against np.sort ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("K", [1, 8])
def test_order_statistics_of_a_ragged_batch(dtype, K):
    """reads of 1 .. 2 T + 5 samples around every vector, wave and tile edge; +-extreme garbage past each length; odd row length"""
    x, lengths = C.ragged(dtype)
    assert x.shape[1] % 2 == 1 and sorted(lengths) == sorted(C.SIZES)
    ranks = C.edge_ranks(lengths, K, 21)
    _same(_select(x, lengths, ranks), C.pick(_sorted(dtype, x, lengths), ranks))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_every_rank_of_the_short_reads(dtype):
    x, lengths = C.ragged(dtype)
    want = _sorted(dtype, x, lengths)
    for call in range(9):                                            # 9 x 8 ranks: every rank of the reads of up to 65 samples
        ranks = C.sweep_ranks(lengths, 8, call, 22)
        _same(_select(x, lengths, ranks), C.pick(want, ranks))


def test_int16_value_patterns():
    names, x, lengths = C.int16_patterns()
    assert names == ("all_equal", "two_values", "extremes", "low_byte_only", "high_byte_only", "concentrated", "uniform")
    want = _sorted("int16_patterns", x, lengths)
    for K, seed in ((8, 23), (1, 24)):
        ranks = C.edge_ranks(lengths, K, seed)
        _same(_select(x, lengths, ranks), C.pick(want, ranks))


def test_fp32_value_patterns():
    names, x, lengths = C.fp32_patterns()
    assert names == ("mixed_signs", "signed_zeros", "infinities", "denormals", "duplicates", "low_mantissa_byte", "exponent_only", "one_nan")
    want = _sorted("fp32_patterns", x, lengths)
    n = int(lengths[-1])
    for K, seed in ((8, 25), (1, 26)):
        ranks = C.edge_ranks(lengths, K, seed)
        got = _select(x, lengths, ranks)
        _same(got, C.pick(want, ranks))
        # the read with a positive NaN, against torch.sort on the CPU at the same ranks: the NaN is the largest element
        by_torch = torch.sort(torch.from_numpy(x[-1, :n].copy()))[0].numpy()
        _same(got[-1], by_torch[ranks[-1]])
    assert np.isnan(_select(x, lengths, np.full((len(lengths), 1), n - 1))[-1, 0])


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_deviation_mode(dtype):
    """out = np.sort(|float32(x) - c|)[rank] in float32; centres integer, half-integer and arbitrary in turn"""
    x, lengths = C.ragged(dtype)
    centers = C.deviation_centers(x.dtype.type, len(lengths))
    want = _sorted(dtype + "_dev", x, lengths, centers)
    for K, seed in ((8, 27), (1, 28)):
        ranks = C.edge_ranks(lengths, K, seed)
        _same(_select(x, lengths, ranks, centers), C.pick(want, ranks))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("with_center", [False, True])
def test_refusals(dtype, with_center):
    """ranks -1 and n, a length of 0, of ld + 1 and below 0: 0.0 for exactly those entries, counted once each; the rest is right"""
    x, lengths = C.ragged(dtype)
    ld = x.shape[1]
    lengths = lengths.copy()
    centers = C.deviation_centers(x.dtype.type, len(lengths)) if with_center else None
    ranks = C.edge_ranks(lengths, 8, 29)
    refused = np.zeros(ranks.shape, dtype=bool)
    ranks[3, 1], ranks[3, 6] = -1, lengths[3]                        # one read with two bad ranks among good ones
    ranks[12, 0] = lengths[12]                                       # the read fed by three workgroups
    refused[3, 1] = refused[3, 6] = refused[12, 0] = True
    for b, n in ((5, 0), (7, ld + 1), (9, -4)):                      # whole reads: every rank of theirs
        lengths[b] = n
        refused[b] = True
    ranks[5] = 0
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _select(x, lengths, ranks, centers, bad=bad)
    want = np.zeros(ranks.shape, dtype=np.float32)
    rows = C.sorted_reads(x, np.where(refused.all(1), 0, lengths), centers)
    for b in range(len(lengths)):
        for k in range(8):
            if not refused[b, k]:
                want[b, k] = rows[b][ranks[b, k]]
    _same(got, want)
    assert np.all(got[refused] == 0.0)
    assert int(bad.item()) == int(refused.sum()) == 3 + 3 * 8
    # without a counter of the caller's the refusals raise
    with pytest.raises(RuntimeError, match="refused"):
        N.read_order_statistics(_dev(x), _dev(lengths), _dev(ranks))


# ---- med / MAD, quantiles, (scale, shift) ------------------------------------------------------------------------------------

def _med_mad_batches(exotic=True):
    for dtype in ("int16", "float32"):
        yield C.ragged(dtype)                                        # n = 1 (mad 0), even and odd n
    yield C.int16_patterns()[1:]                                     # all_equal: mad 0 with n > 1
    if exotic:                                                       # infinities, denormals, signed zeros; without the NaN read
        names, x, lengths = C.fp32_patterns()
        yield x[:-1], lengths[:-1]


def test_read_med_mad_equals_the_reference():
    for x, lengths in _med_mad_batches():
        med, mad = N.read_med_mad(_dev(x), _dev(lengths))
        want = np.array([R.med_mad(x[b], int(n)) for b, n in enumerate(lengths)], dtype=np.float32)
        _same(med.cpu().numpy(), want[:, 0])
        _same(mad.cpu().numpy(), want[:, 1])
        if x.dtype == np.int16:                                      # and float64 numpy, exactly
            r = [x[b, :n].astype(np.float64) for b, n in enumerate(lengths)]
            _same(med.cpu().numpy(), [np.median(v) for v in r])
            _same(mad.cpu().numpy(), [np.median(np.abs(v - np.median(v))) for v in r])


def test_read_med_mad_of_one_sample():
    x, lengths = C.ragged("int16")
    med, mad = N.read_med_mad(_dev(x), _dev(lengths))
    assert lengths[0] == 1 and float(med[0]) == float(x[0, 0]) and float(mad[0]) == 0.0
    sig3 = _dev(x)[:, None, :]                                       # [B, 1, Lpad] is accepted too
    med3, mad3 = N.read_med_mad(sig3, _dev(lengths))
    assert torch.equal(med3, med) and torch.equal(mad3, mad)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_read_quantiles(dtype):
    """lower / higher / midpoint are exact selections; linear is one fp32 rounding of the fp64 lerp and numpy orders its lerp
    differently: 2^-22 relative to the largest magnitude of the read"""
    x, lengths = C.ragged(dtype)
    q = (0.0, 0.2, 0.9, 0.3333)
    xd, ld = _dev(x), _dev(lengths)
    for method in ("lower", "higher", "midpoint"):
        got = N.read_quantiles(xd, ld, q, interpolation=method).cpu().numpy()
        want = np.array([[R.quantile(x[b], int(n), v, method) for v in q] for b, n in enumerate(lengths)], dtype=np.float32)
        _same(got, want)
        by_numpy = np.array([[np.quantile(x[b, :n].astype(np.float64), v, method=method) for v in q] for b, n in enumerate(lengths)])
        _same(got, by_numpy.astype(np.float32))
    got = N.read_quantiles(xd, ld, q).cpu().numpy().astype(np.float64)
    for b, n in enumerate(lengths):
        r = x[b, :n].astype(np.float64)
        err = np.abs(got[b] - np.quantile(r, q)).max()
        print("linear quantiles, n = %d: error %.3e, bound %.3e" % (n, err, LINEAR_BOUND * np.abs(r).max()))
        assert err <= LINEAR_BOUND * np.abs(r).max()
    with pytest.raises(ValueError):
        N.read_quantiles(xd, ld, (0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError):
        N.read_quantiles(xd, ld, (0.5,), interpolation="nearest")


def test_read_normalisation_medmad():
    """shift = -med exactly; scale against float32 numpy within 2^-22 relative (the device's fp32 division is not assumed to be
    correctly rounded: up to a few ulp of 2^-24 each); 1 where mad == 0"""
    for x, lengths in _med_mad_batches(exotic=False):
        scale, shift = N.read_normalisation(_dev(x), _dev(lengths))
        med, mad = N.read_med_mad(_dev(x), _dev(lengths))
        assert torch.equal(shift, -med)
        want = np.array([R.medmad_normalisation(x[b], int(n)) for b, n in enumerate(lengths)], dtype=np.float32)
        _same(shift.cpu().numpy(), want[:, 1])
        s, mad = scale.cpu().numpy(), mad.cpu().numpy()
        assert (mad == 0).any() and np.all(s[mad == 0] == 1.0)
        rel = np.abs(s.astype(np.float64) - want[:, 0]) / want[:, 0]
        print("medmad scale: worst relative error %.3e" % rel.max())
        assert rel.max() <= LINEAR_BOUND


def test_read_normalisation_quantile():
    x, lengths = C.ragged("int16")
    scale, shift = N.read_normalisation(_dev(x), _dev(lengths), method="quantile", q=(0.2, 0.9), factor=1.5, min_spread=2.0)
    v = N.read_quantiles(_dev(x), _dev(lengths), (0.2, 0.9))
    assert torch.equal(shift, -((v[:, 0] + v[:, 1]) * 0.5))
    spread = torch.clamp((v[:, 1] - v[:, 0]) * 1.5, min=2.0)
    assert torch.equal(scale, 1.0 / spread) and float(scale[0]) == 0.5           # one sample: the floor
    with pytest.raises(ValueError):
        N.read_normalisation(_dev(x), _dev(lengths), method="mean")


def test_cpu_tensors_raise():
    x, lengths = C.ragged("int16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.read_med_mad(torch.from_numpy(x), _dev(lengths))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.read_med_mad(_dev(x), torch.from_numpy(lengths))


# ---- reproducibility and graph capture ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_two_calls_are_bitwise_equal(dtype):
    x, lengths = C.ragged(dtype)
    xd, ld = _dev(x), _dev(lengths)
    one = (xd[12:13].contiguous(), ld[12:13].contiguous())           # B = 1, 2 T + 5 samples: three workgroups feed one read
    assert int(one[1][0]) == 2 * T + 5
    for sig, n in (one, (xd, ld)):                                   # and B = 13
        ranks = _dev(C.edge_ranks(n.cpu().numpy(), 8, 30))
        a = (N.read_order_statistics(sig, n, ranks), *N.read_med_mad(sig, n))
        b = (N.read_order_statistics(sig, n, ranks), *N.read_med_mad(sig, n))
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_graph_capture(dtype):
    """read_med_mad captured once, workspaces allocated before the capture, replayed on two inputs written into the static buffers"""
    x, lengths = C.ragged(dtype)
    second = np.ascontiguousarray(x[::-1]), np.ascontiguousarray(lengths[::-1])
    if dtype == "int16":
        second = ((second[0].astype(np.int32) // 2 - 77).astype(np.int16), second[1])
    sig, n = _dev(x).clone(), _dev(lengths).clone()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = (N.select_workspace(len(lengths), 2, sig.dtype, False, DEV), N.select_workspace(len(lengths), 2, sig.dtype, True, DEV))
    eager = [N.read_med_mad(_dev(a), _dev(b)) for a, b in ((x, lengths), second)]
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        N.read_med_mad(sig, n, bad=bad, workspaces=ws)               # warm-up on the capture stream
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            med, mad = N.read_med_mad(sig, n, bad=bad, workspaces=ws)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    for (a, b), (want_med, want_mad) in list(zip(((x, lengths), second), eager))[::-1]:
        sig.copy_(_dev(a))
        n.copy_(_dev(b))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(med, want_med) and torch.equal(mad, want_mad)
    assert int(bad.item()) == 0


# ---- Basecaller ------------------------------------------------------------------------------------------------------------

def test_basecaller_normalise():
    torch.manual_seed(31)
    net = RawCTCNet(16, 3, 5, [(16, 16, 2, d) for d in (1, 2, 4, 3)], 16, softmax=False, causal=False).to(DEV)
    bc = W.Basecaller(net, chunk=32, batch=4)
    g = torch.Generator().manual_seed(32)
    lengths = torch.tensor([1, 29, 150, 333])
    raw = torch.randint(380, 620, (4, 333), generator=g).to(torch.int16).to(DEV)
    len_d = lengths.to(DEV)
    s, t = N.read_normalisation(raw, len_d.to(torch.int32))
    want = bc(raw, lengths, scale=s, shift=t).logits
    assert torch.equal(bc(raw, lengths, normalise="medmad").logits, want)
    assert torch.equal(bc(raw, len_d, normalise="medmad").logits, want)
    seen = []

    def mine(signal, n):
        seen.append((tuple(signal.shape), n.dtype, n.is_cuda))
        return N.read_normalisation(signal, n, method="medmad")

    assert torch.equal(bc(raw[:, None, :], lengths, normalise=mine).logits, want)
    assert seen == [((4, 333), torch.int32, True)]
    sq, tq = N.read_normalisation(raw, len_d, method="quantile")
    assert torch.equal(bc(raw, lengths, normalise="quantile").logits, bc(raw, lengths, scale=sq, shift=tq).logits)
    for kw in (dict(scale=s), dict(shift=t), dict(scale=s, shift=t)):
        with pytest.raises(ValueError, match="normalise"):
            bc(raw, lengths, normalise="medmad", **kw)
    with pytest.raises(ValueError, match="normalise"):
        bc(raw, lengths, normalise="zscore")
    fsig = raw.float()
    assert torch.equal(bc(fsig, lengths, normalise=None).logits, bc(fsig, lengths).logits)
    assert torch.equal(bc(raw, lengths, scale=s, shift=t, normalise=None).logits, want)
