"""GPU: chunked whole-read basecalling (wavenet_speech_amd/basecalling.py, csrc/wn_chunk.hip).  The gather and stitch kernels
are held bit-equal to indexing on the CPU; the Basecaller's logits are held to the fp64 oracle of the zero-padded read at the
project's parity bar (fp32) or at the error of the existing full-length forward in the same mode (bf16, f16x3), and the graphed
forward to bitwise equality with the eager one."""
import pytest
import torch
import torch.nn.functional as F

import wavenet_speech_amd as W
from oracle import wavenet_oracle as O
from wavenet_speech_amd.basecalling import Basecaller, chunk_gather, chunk_plan, chunk_stitch, receptive_field
from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = 32
LENGTHS = (1, 27, 28, 29, 32, 33, 150, 333)         # around chunk - right = 28 and chunk = 32, then several chunks
# name -> (feature_kwidth, block kernel width, dilations, causal, lengths)
VARIANTS = {
    "k2_noncausal": (3, 2, (1, 2, 4, 3), False, LENGTHS),
    "k3_noncausal": (1, 3, (1, 2, 5), False, (23, 140)),
    "k2_causal": (2, 2, (1, 2, 4), True, (31, 140)),
}


class Case(object):
    """one model on the CPU with its reads, and the fp64 oracle's logits of every zero-padded read (computed once)"""

    def __init__(self, name):
        fk, k, dil, causal, lengths = VARIANTS[name]
        torch.manual_seed(21)
        self.layers = [(16, 16, k, d) for d in dil]
        self.net = RawCTCNet(16, fk, 5, self.layers, 16, softmax=False, causal=causal)
        self.fk, self.causal, self.lengths = fk, causal, list(lengths)
        self.left, self.right = receptive_field(self.net)
        g = torch.Generator().manual_seed(22)
        self.signal = torch.zeros(len(lengths), max(lengths))
        for b, n in enumerate(lengths):
            self.signal[b, :n] = torch.randn(n, generator=g)
        # every row of the zero-padded batch IS its read followed by at least right + 3 zeros
        sd = {key: v.detach().double() for key, v in self.net.state_dict().items()}
        padded = F.pad(self.signal.double().unsqueeze(1), (0, self.right + 3))
        full = O.raw_ctcnet(padded, sd, self.layers, fk, softmax=False, causal=causal)
        self.want = [full[b, :, :n + fk - 1] for b, n in enumerate(lengths)]

    def model(self, precision="f32"):
        import copy
        net = copy.deepcopy(self.net).to(DEV)
        W.set_precision(net, precision)
        return net

    def errors(self, logits):
        """rel_err of every read's frames against the oracle"""
        logits = logits.detach().cpu().double()
        return [O.rel_err(logits[b, :, :w.shape[1]], w) for b, w in enumerate(self.want)]


_CASES = {}


def case(name="k2_noncausal"):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------------

def _gather_want(signal, lengths, rows, chunk, scale=None, shift=None):
    """torch indexing on the CPU: (x.float() + shift) * scale inside the read, 0 past it and in dead chunks"""
    x = signal.float()
    if shift is not None:
        x = x + shift[:, None]
    if scale is not None:
        x = x * scale[:, None]
    out = torch.zeros(len(rows), chunk)
    for i, (rd, s0, _u, _t0, count) in enumerate(rows):
        if count == 0:
            continue
        m = max(0, min(lengths[rd] - s0, chunk))
        out[i, :m] = x[rd, s0:s0 + m]
    return out


GATHER_ROWS = [(0, 0, 0, 0, 5), (0, 19, 9, 28, 3), (1, 0, 0, 0, 28), (1, 57, 9, 66, 19), (1, 101, 9, 110, 2), (0, 0, 0, 0, 0),
               (2, 7, 9, 16, 1), (2, 68, 9, 77, 1), (1, 3, 9, 12, 19)]
GATHER_LENGTHS = [40, 130, 71]                       # read 0 ends inside its second chunk, read 2 one sample into its last


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
@pytest.mark.parametrize("affine", ["none", "scale", "shift", "both"])
@pytest.mark.parametrize("chunk", [32, 1028])
def test_gather_is_bit_equal_to_indexing(dtype, affine, chunk):
    g = torch.Generator().manual_seed(3)
    ld = 136                                                          # rows longer than the longest read
    if dtype == torch.int16:
        signal = torch.randint(-32768, 32768, (3, ld), generator=g).to(torch.int16)
    else:
        signal = torch.randn(3, ld, generator=g) * 90 + 400
    scale = torch.tensor([0.1755, 1.0 / 3.0, 7.25]) if affine in ("scale", "both") else None
    shift = torch.tensor([-13.0, 0.3, 1e-3]) if affine in ("shift", "both") else None
    rows = torch.tensor(GATHER_ROWS, dtype=torch.int32)
    out = torch.full((len(GATHER_ROWS), chunk), float("nan"), device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    chunk_gather(signal.to(DEV), torch.tensor(GATHER_LENGTHS, dtype=torch.int32, device=DEV), rows.to(DEV), chunk, out,
                 None if scale is None else scale.to(DEV), None if shift is None else shift.to(DEV), bad)
    want = _gather_want(signal, GATHER_LENGTHS, GATHER_ROWS, chunk, scale, shift)
    assert int(bad.item()) == 0
    assert torch.equal(out.cpu(), want)                               # every element written, bit for bit
    assert float(out[5].abs().max()) == 0.0                           # the dead chunk


def test_gather_counts_bad_rows_and_writes_zeros():
    signal = torch.arange(1.0, 201.0).view(2, 100)
    lengths = torch.tensor([100, 101], dtype=torch.int32)             # read 1 claims more samples than a row holds
    rows = [(0, 10, 0, 10, 4), (2, 0, 0, 0, 4), (-1, 0, 0, 0, 4), (0, 100, 9, 109, 1), (0, -1, 0, 0, 4), (1, 0, 0, 0, 4), (0, 90, 0, 90, 4)]
    out = torch.full((len(rows), 32), float("nan"), device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    chunk_gather(signal.to(DEV), lengths.to(DEV), torch.tensor(rows, dtype=torch.int32, device=DEV), 32, out, None, None, bad)
    assert int(bad.item()) == 5                                       # read 2, read -1, s0 = ld, s0 = -1, the overlong read
    out = out.cpu()
    assert torch.equal(out[0], signal[0, 10:42])
    assert torch.equal(out[6], torch.cat([signal[0, 90:], torch.zeros(22)]))
    assert float(out[1:6].abs().max()) == 0.0


def test_stitch_is_bit_equal_to_indexing():
    g = torch.Generator().manual_seed(4)
    C, Ty = 5, 34
    rows = [(0, 0, 0, 0, 28), (0, 19, 9, 28, 19), (0, 38, 9, 47, 3), (1, 0, 0, 0, 7), (0, 0, 0, 0, 0), (2, 0, 0, 0, 28), (2, 19, 9, 28, 19)]
    frame_lengths = [50, 7, 47]
    # y through its strides: [N, C, Ty] is a transposed, strided view of a larger [N, Ty, 2 C] tensor
    base = torch.randn(len(rows), Ty, 2 * C, generator=g)
    y = base.to(DEV)[:, :, ::2].transpose(1, 2)
    assert y.shape == (len(rows), C, Ty) and y.stride() == (Ty * 2 * C, 2, 2 * C)
    out = torch.zeros(3, C, 60, device=DEV)[:, :, :52]                # rows of out need not be dense either
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    chunk_stitch(y, torch.tensor(rows, dtype=torch.int32, device=DEV), out, torch.tensor(frame_lengths, dtype=torch.int32, device=DEV), bad)
    want = torch.zeros(3, C, 52)
    yc = base[:, :, ::2].transpose(1, 2)
    for i, (rd, _s0, u_lo, t0, count) in enumerate(rows):
        want[rd, :, t0:t0 + count] = yc[i, :, u_lo:u_lo + count]
    assert int(bad.item()) == 0
    assert torch.equal(out.cpu(), want)


def test_stitch_skips_rows_that_overrun():
    C, Ty = 3, 34
    y = torch.randn(6, C, Ty, generator=torch.Generator().manual_seed(5))
    rows = [(0, 0, 0, 0, 10), (0, 10, 9, 19, 12), (1, 0, 0, 0, 9), (2, 0, 0, 0, 4), (1, 0, 30, 0, 5), (0, 0, 0, 10, 9)]
    frame_lengths = [30, 8]                    # row 1 ends at frame 31 > 30; row 2 keeps 9 > 8; row 3: read 2 of 2; row 4: u_lo + count > Ty
    out = torch.zeros(2, C, 30, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    chunk_stitch(y.to(DEV), torch.tensor(rows, dtype=torch.int32, device=DEV), out, torch.tensor(frame_lengths, dtype=torch.int32, device=DEV),
                 bad)
    assert int(bad.item()) == 4
    want = torch.zeros(2, C, 30)
    want[0, :, 0:10] = y[0, :, 0:10]
    want[0, :, 10:19] = y[5, :, 0:9]
    assert torch.equal(out.cpu(), want)


# ---- the Basecaller ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,batch", [("k2_noncausal", 4), ("k2_noncausal", 64), ("k3_noncausal", 4), ("k2_causal", 4)])
def test_f32_logits_against_the_oracle_and_the_full_length_forward(name, batch):
    c = case(name)
    net = c.model()
    sig, lengths = c.signal.to(DEV), torch.tensor(c.lengths)
    n_chunks = int(chunk_plan(lengths, CHUNK, c.left, c.right, c.fk).chunks_per_read.sum())
    assert (n_chunks % batch != 0) if batch == 4 else (n_chunks < batch)        # dead chunks in the last / only micro-batch
    out = Basecaller(net, chunk=CHUNK, batch=batch)(sig.unsqueeze(1), lengths)
    assert out.frame_lengths.dtype == torch.int32 and out.frame_lengths.tolist() == [n + c.fk - 1 for n in c.lengths]
    assert out.logits.shape == (len(c.lengths), 5, max(c.lengths) + c.fk - 1) and out.logits.dtype == torch.float32
    assert out.labels is None and out.label_lengths is None and out.frames is None and out.scores is None
    errs = c.errors(out.logits)
    own = []
    with torch.no_grad():
        for b, n in enumerate(c.lengths):
            T = n + c.fk - 1
            full = net(F.pad(sig[b:b + 1, None, :n], (0, c.right + 3)))[..., :T]
            own.append(O.rel_err(out.logits[b:b + 1, :, :T], full))
            assert float(out.logits[b, :, T:].abs().max() if T < out.logits.shape[2] else 0.0) == 0.0      # exactly 0 past T_b
    print("%s batch %d: vs fp64 oracle %.2e, vs the package's full-length forward %.2e" % (name, batch, max(errs), max(own)))
    assert max(errs) <= 1e-4, errs
    assert max(own) <= 2e-4, own


@pytest.mark.parametrize("precision", ["bf16", "f16x3"])
def test_half_modes_are_as_close_to_the_oracle_as_the_full_length_forward(precision):
    c = case()
    net = c.model(precision)
    sig, lengths = c.signal.to(DEV), torch.tensor(c.lengths)
    out = Basecaller(net, chunk=CHUNK, batch=4)(sig, lengths)
    with torch.no_grad():
        full = net(F.pad(sig.unsqueeze(1), (0, c.right + 3)))        # the existing forward: every row is its read, zero-padded
    chunked, whole = max(c.errors(out.logits)), max(c.errors(full))
    print("%s: chunked %.3e, full-length %.3e against the fp64 oracle" % (precision, chunked, whole))
    assert chunked <= 1.25 * whole + 1e-6, (chunked, whole)


def test_graphed_forward_is_bitwise_the_eager_one():
    c = case()
    net = c.model("bf16")
    eager, graphed = Basecaller(net, chunk=CHUNK, batch=4), Basecaller(net, chunk=CHUNK, batch=4, graph=True)
    lengths = torch.tensor(c.lengths)
    g = torch.Generator().manual_seed(9)
    for _ in range(2):                                                # new reads each call: the replay reads the refilled buffer
        sig = (c.signal != 0).float() * torch.randn(c.signal.shape, generator=g)
        a, b = eager(sig.to(DEV), lengths), graphed(sig.to(DEV), lengths)
        assert torch.equal(a.logits, b.logits)
        assert float(b.logits.abs().max()) > 0.0
    W.check_device_flags()


def test_graphed_fp16_overflow_raises():
    c = case()
    net = c.model("f16")
    bc = Basecaller(net, chunk=CHUNK, batch=4, graph=True)
    sig, lengths = c.signal.to(DEV), torch.tensor(c.lengths)
    bc(sig, lengths)                                                  # in range: no exception
    huge = torch.full((len(c.lengths),), 1e8, device=DEV)       # finite in fp32, far outside fp16
    with pytest.raises(RuntimeError):
        bc(sig, lengths, scale=huge)
    bc(sig, lengths)                                                  # and the next call is clean again
    W.check_device_flags()


def test_decoders_get_the_logits_and_frame_lengths():
    c = case()
    bc = Basecaller(c.model(), chunk=CHUNK, batch=4)
    sig, lengths = c.signal.to(DEV), torch.tensor(c.lengths)
    out = bc(sig, lengths, decode="greedy")
    labels, label_lengths, frames = W.ctc_greedy_decode(out.logits, input_lengths=out.frame_lengths)
    assert torch.equal(out.labels, labels) and torch.equal(out.label_lengths, label_lengths) and torch.equal(out.frames, frames)
    assert out.scores is None
    out = bc(sig, lengths, decode="beam", beam_width=4)
    labels, label_lengths, scores, frames = W.ctc_beam_decode(out.logits, 4, input_lengths=out.frame_lengths)
    assert torch.equal(out.labels, labels) and torch.equal(out.label_lengths, label_lengths) and torch.equal(out.frames, frames)
    assert torch.equal(out.scores, scores)
    assert bc(sig, lengths, decode="greedy", want_logits=False).logits is None
    W.check_device_flags()


def test_ragged_reads_end_to_end():
    reads = W.ragged_reads(8, lengths=(60, 120), device="cuda", generator=torch.Generator().manual_seed(5))
    net = case().model()
    shift, scale = torch.full((8,), -90.0, device=DEV), torch.full((8,), 0.05, device=DEV)           # picoamps around 90 +- 30
    out = Basecaller(net, chunk=64, batch=8)(reads.signal, reads.signal_lengths, scale=scale, shift=shift, decode="greedy")
    assert int(reads.signal_lengths.max()) > 64                       # several chunks per read; device lengths: one read-back
    assert out.logits.shape[0] == 8 and bool(torch.isfinite(out.logits).all())
    assert out.frame_lengths.tolist() == [int(n) + 2 for n in reads.signal_lengths.tolist()]
    assert bool((out.label_lengths <= out.frame_lengths).all()) and bool((out.label_lengths >= 0).all())
    W.check_device_flags()


def test_int16_input_equals_the_same_read_as_float32():
    c = case()
    bc = Basecaller(c.model(), chunk=CHUNK, batch=4)
    lengths = torch.tensor(c.lengths)
    raw = (c.signal * 80 + 500).round().clamp(-32768, 32767).to(torch.int16)
    scale = torch.linspace(0.01, 0.02, len(c.lengths))
    shift = torch.linspace(-520.0, -480.0, len(c.lengths))
    a = bc(raw.to(DEV), lengths, scale=scale.to(DEV), shift=shift.to(DEV))
    as_float = (raw.float() + shift[:, None]) * scale[:, None]
    b = bc(as_float.to(DEV), lengths)
    assert torch.equal(a.logits, b.logits)
    assert torch.equal(bc(raw.float().to(DEV), lengths, scale=scale.to(DEV), shift=shift.to(DEV)).logits, a.logits)


def test_what_cannot_be_basecalled_raises():
    c = case()
    net = c.model()
    with pytest.raises(ValueError):
        Basecaller(RawCTCNet(16, 3, 5, c.layers, 16, positions=True).to(DEV))
    with pytest.raises(ValueError):
        Basecaller(net, chunk=12)                                     # below left + right + 1 = 14
    with pytest.raises(ValueError):
        Basecaller(net, chunk=30)                                     # not a multiple of 4
    with pytest.raises(RuntimeError):
        Basecaller(RawCTCNet(16, 3, 5, c.layers, 16), chunk=CHUNK)    # a model on the CPU
    bc = Basecaller(net, chunk=CHUNK, batch=4)
    lengths = torch.tensor(c.lengths)
    with pytest.raises(RuntimeError):
        bc(c.signal, lengths)                                         # a CPU signal
    with pytest.raises(TypeError):
        bc(c.signal.double().to(DEV), lengths)
    with pytest.raises(ValueError):
        bc(c.signal.to(DEV), lengths + 1)                             # a read longer than its row
    with pytest.raises(ValueError):
        bc(c.signal.to(DEV), lengths[:-1])
    with pytest.raises(ValueError):
        bc(c.signal.to(DEV), lengths, decode="viterbi")
