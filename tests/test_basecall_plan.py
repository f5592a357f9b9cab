"""CPU: the host side of chunked whole-read basecalling (wavenet_speech_amd/basecalling.py) against the fp64 oracle.
receptive_field() must equal the reach measured by perturbing single samples; chunk_plan(), driven through the oracle (zero-
filled chunks of exactly `chunk` samples, `count` frames kept from `u_lo`), must reproduce the forward of the zero-padded read
to summation order -- a seam error (an off-by-one at the deepest tap) is many orders larger than the 1e-12 bound."""
import pytest
import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as O
from wavenet_speech_amd.basecalling import _plan, chunk_plan, receptive_field
from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet

# name -> (feature_kwidth, block kernel width, dilations, causal, expected (left, right))
MODELS = {
    "k2_noncausal": (3, 2, (1, 2, 4, 3), False, (9, 4)),
    "k3_noncausal": (1, 3, (1, 2, 5), False, (9, 8)),
    "k2_causal": (2, 2, (1, 2, 4), True, (9, 0)),
}


def _model(name):
    fk, k, dil, causal, _ = MODELS[name]
    torch.manual_seed(11)
    layers = [(8, 8, k, d) for d in dil]
    net = RawCTCNet(8, fk, 5, layers, 8, softmax=False, causal=causal)
    sd = {key: v.detach().double() for key, v in net.state_dict().items()}
    return net, sd, layers, fk, causal


def _forward(x, sd, layers, fk, causal):
    return O.raw_ctcnet(x, sd, layers, fk, softmax=False, causal=causal)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_receptive_field_equals_the_perturbed_reach(name):
    net, sd, layers, fk, causal = _model(name)
    left, right = receptive_field(net)
    assert (left, right) == MODELS[name][4]
    L, t = 64, 30
    x = torch.randn(1, 1, L, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    y = _forward(x, sd, layers, fk, causal)

    def moved(sample):
        xp = x.clone()
        xp[0, 0, sample] += 1.0
        return float((_forward(xp, sd, layers, fk, causal)[0, :, t] - y[0, :, t]).abs().max())

    assert moved(t - left) > 0.0                  # the edge of the reach changes frame t ...
    assert moved(t - left - 1) == 0.0             # ... one sample further out does not
    assert moved(t + right) > 0.0
    assert moved(t + right + 1) == 0.0


def test_receptive_field_refuses_what_a_chunk_cannot_reproduce():
    with pytest.raises(ValueError):
        receptive_field(RawCTCNet(8, 3, 5, [(8, 8, 2, 1)], 8, positions=True))
    with pytest.raises(TypeError):
        receptive_field(torch.nn.Linear(2, 2))


def _chunk_sizes(left, right):
    return [left + right + 1, left + right + 2, 32, 64]


def _lengths(chunk, right):
    return [1, 2, chunk - right - 1, chunk - right, chunk - right + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]


def _expected_chunks(T, chunk, left, right):
    first, step = chunk - right, chunk - left - right
    return 1 if T <= first else 1 + -(-(T - first) // step)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_plan_through_the_oracle_equals_the_padded_forward(name):
    net, sd, layers, fk, causal = _model(name)
    left, right = receptive_field(net)
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for chunk in _chunk_sizes(left, right):
        lengths = [n for n in _lengths(chunk, right) if n >= 1]
        # the arithmetic behind chunk_plan without its chunk % 4 rule: the smallest chunk sizes are no multiple of 4 (that is a
        # requirement of the gather kernel's stores, not of the plan, which is what this test holds to the oracle)
        plan = _plan(lengths, chunk, left, right, fk, None, 1)
        if chunk % 4 == 0:
            assert torch.equal(chunk_plan(lengths, chunk, left, right, fk).rows, plan.rows)
        assert plan.frame_lengths.tolist() == [n + fk - 1 for n in lengths]
        at = 0
        for b, n in enumerate(lengths):
            T = n + fk - 1
            read = torch.randn(1, 1, n, dtype=torch.float64, generator=g)
            want = _forward(F.pad(read, (0, right + 3)), sd, layers, fk, causal)[..., :T]
            k = int(plan.chunks_per_read[b])
            assert k == _expected_chunks(T, chunk, left, right), (chunk, n)
            rows = plan.rows[at:at + k].tolist()
            at += k
            xs = torch.zeros(k, 1, chunk, dtype=torch.float64)
            for i, (rd, s0, _u, _t0, _c) in enumerate(rows):
                assert rd == b and 0 <= s0 < n
                m = min(n - s0, chunk)
                xs[i, 0, :m] = read[0, 0, s0:s0 + m]                 # samples at or past n read as 0
            ys = _forward(xs, sd, layers, fk, causal)
            got = torch.full_like(want, float("nan"))
            for i, (_rd, _s0, u_lo, t0, count) in enumerate(rows):
                got[0, :, t0:t0 + count] = ys[i, :, u_lo:u_lo + count]
            err = float((got - want).abs().max())                    # NaN (a frame no chunk kept) fails the bound too
            worst = max(worst, err)
            assert err <= 1e-12, (name, chunk, n, err)
        assert at == plan.rows.shape[0]
    print("%s: worst |chunked - padded forward| = %.2e (fp64)" % (name, worst))


@pytest.mark.parametrize("left,right,fk", [(9, 4, 3), (9, 8, 1), (9, 0, 2), (0, 0, 1), (40, 37, 5)])
def test_plan_invariants(left, right, fk):
    for chunk in sorted({(left + right + 1 + 3) // 4 * 4, (left + right + 1 + 3) // 4 * 4 + 4, 32 if left + right < 32 else 96, 4096}):
        lengths = sorted({n for n in _lengths(chunk, right) + [5 * chunk, 17] if n >= 1})
        plan = chunk_plan(torch.tensor(lengths), chunk, left, right, fk)
        assert plan.rows.dtype == torch.int32 and plan.frame_lengths.dtype == torch.int32
        assert plan.rows.shape == (int(plan.chunks_per_read.sum()), 5)
        at = 0
        for b, n in enumerate(lengths):
            T = n + fk - 1
            k = int(plan.chunks_per_read[b])
            assert k == _expected_chunks(T, chunk, left, right)
            covered = 0
            for i, (rd, s0, u_lo, t0, count) in enumerate(plan.rows[at:at + k].tolist()):
                assert rd == b and count >= 1
                assert t0 == covered                                  # no gap, no overlap, in order
                assert t0 == s0 + u_lo                                # chunk-local frame u is read frame s0 + u
                assert (s0, u_lo) == (0, 0) if i == 0 else u_lo == left
                assert u_lo + count <= chunk - right and 0 <= s0 < n
                covered += count
            assert covered == T
            at += k


def test_plan_refuses_bad_arguments():
    for bad in ([0], [5, -1], [], [[3]], [2.5]):
        with pytest.raises(ValueError):
            chunk_plan(bad, 32, 9, 4, 3)
    with pytest.raises(ValueError):
        chunk_plan([10, 101], 32, 9, 4, 3, capacity=100)              # a read longer than the row it is stored in
    chunk_plan([10, 100], 32, 9, 4, 3, capacity=100)
    with pytest.raises(ValueError):
        chunk_plan([10], 12, 9, 4, 3)                                 # chunk < left + right + 1 = 14
    chunk_plan([10], 16, 9, 4, 3)
    with pytest.raises(ValueError):
        chunk_plan([10], 30, 9, 4, 3)                                 # not a multiple of 4
    with pytest.raises(ValueError):
        chunk_plan([10], 32, -1, 4, 3)
    with pytest.raises(ValueError):
        chunk_plan([10], 32, 9, 4, 0)
