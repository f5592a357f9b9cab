"""
Synthetic nanopore-like signal, on whatever device the caller asks for: a vectorised restatement
of the reference's on-line generator utils/gaussian_kmer_model.py, stage by stage:

    kmer_indices   nucleotides 1..4 -> 5-mer index sum((nt-1) * [256,64,16,4,1]) of the window starting two bases in
                   (scipy generic_filter with its centred window, then the [4:-4] trim: n-8 k-mers from n bases), each
                   k-mer held for `upsampling` samples                                               (:49, :58-64)
    gaussian_picoamps   sample ~ N(mean[kmer], stdv[kmer])                                             (:67-73)
    quantize       per-read (x - mean) / (max - min), mu-law with mu = num_levels, np.digitize against
                   linspace(-1, 1, num_levels) -- in float64 like the reference                         (:36-40, :79-86)
    one_hot        (num_levels, L) float32                                                            (:89-97)

Parity: the three deterministic stages are pinned by tests/golden/generator_00.npz, captured from the reference's own
functions (tests/golden/make_generator_golden.py); the Gaussian draw is the only random stage (the reference uses
numpy's global RNG, here the device's generator), checked statistically.

The reference reads its 1024-entry mean/stdv table from utils/r9.4_450bps.5mer.template.npz (nanopolish's r9.4 model).
That file is reference data and does not travel; without a table argument a seeded stand-in with the same ranges
(means 59.6-118.5 pA, stdvs 1.34-5.86 pA) is used.

On a GPU `gaussian_kmer_signal` runs the HIP generator (csrc/wn_synth.hip through the C ABI's wn_synth_*: Philox
nucleotides and Gaussian noise, float64 signal, per-read normalisation, mu-law, digitize, optional one-hot -- three
launches, nothing drawn or computed on the host; it fails loudly if the library is missing).  The stage functions below
are the same arithmetic as plain torch ops: the CPU form that the fixture pins, and the checker of the HIP kernels.

`ragged_reads` is the generator of the reference's RawCTCNet workloads (RawGaussianModelLoader with random_upsample=True,
RawSignalGenerator): reads of random length, every k-mer held for a random number of samples, raw float32 picoamps
zero-padded to a common length, the bases as CTC targets -- csrc/wn_reads.hip on a GPU (two launches), torch ops on the CPU.
`RawGaussianModelLoader` is the reference's loader class on top of it.
"""
import collections
import ctypes
import math

import torch

from . import _args, _flags, _lib
from ._args import _alloc_bytes, _p, _stream

KMER_WEIGHTS = (256, 64, 16, 4, 1)


def standin_kmer_table(seed=945, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    means = 59.6 + (118.5 - 59.6) * torch.rand(1024, generator=g)
    stdvs = 1.34 + (5.86 - 1.34) * torch.rand(1024, generator=g)
    return means.to(device), stdvs.to(device)


def mu_law(x, mu):
    return torch.sign(x) * torch.log1p(mu * x.abs()) / math.log1p(mu)


def kmer_indices(bases, upsampling=1):
    """bases [..., n] int64 in 1..4 -> k-mer indices [..., (n - 8) * upsampling] in 0..1023 (utils/gaussian_kmer_model.py:49,
    :58-64).  The reference slides scipy's centred 5-window over the zero-padded sequence and drops the first and last
    four outputs: what is left are the windows bases[p+2 .. p+6], p = 0 .. n-9."""
    w = torch.tensor(KMER_WEIGHTS, device=bases.device, dtype=bases.dtype)
    windows = (bases - 1).unfold(-1, 5, 1)                      # [..., n-4, 5], window i = bases[i .. i+4]
    kmers = (windows * w).sum(-1)[..., 2:-2]                    # windows 2 .. n-7
    if upsampling > 1:
        kmers = kmers.repeat_interleave(upsampling, dim=-1)
    return kmers


def gaussian_picoamps(kmers, table, generator=None):
    """N(mean[kmer], stdv[kmer]) drawn on the device of `kmers` (:67-73)"""
    means, stdvs = table
    noise = torch.randn(kmers.shape, generator=generator, device=kmers.device, dtype=means.dtype)
    return means[kmers] + stdvs[kmers] * noise


def quantize(picoamps, num_levels=256):
    """per-read normalisation, mu-law, np.digitize (:79-86); float64 like the reference's numpy arithmetic.
    Returns int64 levels in 1 .. num_levels-1 (0 is never produced: the normalised signal lies strictly inside (-1, 1))."""
    x = picoamps.double()
    span = x.amax(-1, keepdim=True) - x.amin(-1, keepdim=True)
    normalised = (x - x.mean(-1, keepdim=True)) / span
    mapped = mu_law(normalised, float(num_levels))
    edges = torch.linspace(-1.0, 1.0, num_levels, device=x.device, dtype=torch.float64)
    return torch.bucketize(mapped, edges, right=True)           # == np.digitize(mapped, edges)


def one_hot(levels, num_levels=256):
    """[..., L] int64 -> [..., num_levels, L] float32 (:89-97)"""
    out = torch.zeros(levels.shape[:-1] + (num_levels, levels.shape[-1]), device=levels.device)
    return out.scatter_(-2, levels.unsqueeze(-2), 1.0)


def _device_seed(generator, dev):
    """one 63-bit seed for the Philox streams of the HIP generator, drawn from the caller's torch generator (or torch's
    default one) so that a seeded call stays reproducible"""
    g = generator if generator is not None and torch.device(generator.device).type == "cpu" else None
    if generator is not None and g is None:
        return int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=dev).item())
    return int(torch.randint(0, 2 ** 62, (1,), generator=g).item())


def hip_signal(bases, length, num_levels=256, upsampling=3, table=None, seed=0, noise=None, want_one_hot=True, picoamps=None):
    """The HIP stages on given nucleotides (device int64 [B, n]).  `noise` (float64 [B, L]) replaces the Philox Gaussian
    draw; `picoamps` (float64 [B, L]) skips the signal stage altogether (quantize + one-hot of a given signal).
    Returns (levels, one_hot or None, picoamps)."""
    lib = _lib.load()
    dev = bases.device
    if dev.type != "cuda":
        raise RuntimeError("wavenet_speech_amd: the HIP generator needs device tensors")
    B, nb = bases.shape
    with torch.cuda.device(dev):
        ws = _alloc_bytes(lib.wn_synth_workspace_bytes(B, length), "wn_synth_workspace_bytes", dev)
        ws_bytes = ws.numel()
        means, stdvs = table if table is not None else standin_kmer_table(device=dev)
        means, stdvs = means.to(dev).double().contiguous(), stdvs.to(dev).double().contiguous()
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        given = picoamps is not None
        if given:
            # statistics of a caller's signal: run the signal stage on it as "noise" with unit tables (x = 0 + 1 * x)
            pico = torch.empty(B, length, dtype=torch.float64, device=dev)
            zeros, ones = torch.zeros(1024, dtype=torch.float64, device=dev), torch.ones(1024, dtype=torch.float64, device=dev)
            _lib.check(lib.wn_synth_signal(_p(bases.contiguous()), B, nb, length, upsampling, _p(zeros), _p(ones), 0,
                                           _p(picoamps.double().contiguous()), _p(pico), _p(ws), ws_bytes, None, _stream()),
                       "wn_synth_signal")
        else:
            pico = torch.empty(B, length, dtype=torch.float64, device=dev)
            nz = None if noise is None else noise.double().contiguous()
            _lib.check(lib.wn_synth_signal(_p(bases.contiguous()), B, nb, length, upsampling, _p(means), _p(stdvs),
                                           ctypes.c_ulonglong(seed), _p(nz), _p(pico), _p(ws), ws_bytes, _p(bad), _stream()),
                       "wn_synth_signal")
        edges = torch.linspace(-1.0, 1.0, num_levels, device=dev, dtype=torch.float64)
        levels = torch.empty(B, length, dtype=torch.int64, device=dev)
        oh = torch.empty(B, num_levels, length, dtype=torch.float32, device=dev) if want_one_hot else None
        _lib.check(lib.wn_synth_quantize(_p(pico), _p(ws), ws_bytes, B, length, num_levels, _p(edges), _p(levels), _p(oh),
                                         _stream()), "wn_synth_quantize")
        if not given and int(bad.item()):
            raise RuntimeError("wavenet_speech_amd: nucleotides outside 1..4 in the generator's input")
    return levels, oh, pico


def hip_bases(batch, nbases, seed, device):
    lib = _lib.load()
    dev = torch.device(device)
    with torch.cuda.device(dev):
        bases = torch.empty(batch, nbases, dtype=torch.int64, device=dev)
        _lib.check(lib.wn_synth_bases(ctypes.c_ulonglong(seed), batch, nbases, _p(bases), _stream()), "wn_synth_bases")
    return bases


def gaussian_kmer_signal(batch, length, num_levels=256, upsampling=3, table=None, generator=None, device="cpu",
                         want_one_hot=True):
    """Returns (levels [B, L] int64, one_hot [B, num_levels, L] float32, bases [B, n] int64 in 1..4): `convert_to_signal`
    (:99-104) for a batch of random reads, every random number drawn on `device` (pass a generator of that device).
    On a GPU this is the HIP generator (one_hot is None with want_one_hot=False: the level-index entry conv needs none)."""
    dev = torch.device(device)
    if dev.type == "cuda":
        seed = _device_seed(generator, dev)
        n_kmers = -(-length // upsampling)
        bases = hip_bases(batch, n_kmers + 8, seed, dev)
        levels, oh, _ = hip_signal(bases, length, num_levels, upsampling, table, seed, want_one_hot=want_one_hot)
        return levels, oh, bases
    if generator is not None and torch.device(generator.device).type != dev.type:
        # a CPU generator with a GPU target: draw the seed from it so the call stays reproducible, then go on-device
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator))
        generator = torch.Generator(device=dev).manual_seed(seed)
    means, stdvs = table if table is not None else standin_kmer_table(device=dev)
    n_kmers = -(-length // upsampling)
    bases = torch.randint(1, 5, (batch, n_kmers + 8), generator=generator, device=dev)
    kmers = kmer_indices(bases, upsampling)[:, :length]
    picoamps = gaussian_picoamps(kmers, (means.to(dev), stdvs.to(dev)), generator)
    levels = quantize(picoamps, num_levels).clamp_(0, num_levels - 1)
    return levels, one_hot(levels, num_levels), bases


# ---- ragged reads: random lengths, random dwell, raw picoamps, CTC targets (csrc/wn_reads.hip) ----------------------------

RaggedReads = collections.namedtuple("RaggedReads", "signal signal_lengths bases base_lengths targets dwell starts sample_kmer")
RaggedReads.__doc__ = """signal [B, 1, Lpad] float32 picoamps, 0 past signal_lengths [B] int32; bases [B, nmax] int32 in 1..4, 0
past base_lengths [B] int32; targets: the bases concatenated in read order (int32; None with pad_to on a GPU: its shape depends on
the data); dwell [B, Kmax] int32 samples per k-mer, 0 past K_b = base_lengths[b] - 4 - 2 * window; starts [B, Kmax + 1] int32:
first sample of every k-mer, = signal_lengths[b] from K_b on; sample_kmer [B, Lpad] int32: the k-mer of every sample, -1 past
the read."""

WINDOWS = {"loader": 2, "generator": 0}     # k-mer p = bases[p + window .. p + window + 4]
DWELL_MODELS = {"fixed": 0, "uniform": 1, "gamma": 2}    # WN_DWELL_*


def _dwell_spec(dwell):
    """("fixed", r) | ("uniform", r, w) | ("gamma", shape, rate, sample_rate) -> (model, p0, p1, p2), validated"""
    kind = dwell[0]
    if kind == "fixed" and len(dwell) == 2 and int(dwell[1]) >= 1:
        return 0, float(int(dwell[1])), 0.0, 0.0
    if kind == "uniform" and len(dwell) == 3:
        r, w = int(dwell[1]), int(dwell[2])
        if r >= 1 and w >= 0 and r + w > max(r - w, 1):
            return 1, float(r), float(w), 0.0
        raise ValueError("ragged_reads: the uniform dwell interval [max(r - w, 1), r + w) is empty for r = %d, w = %d" % (r, w))
    if kind == "gamma" and len(dwell) == 4:
        shape, rate, srate = (float(v) for v in dwell[1:])
        if shape > 0 and rate > 0 and srate > 0 and all(math.isfinite(v) for v in (shape, rate, srate)):
            return 2, shape, rate, srate
        raise ValueError("ragged_reads: gamma dwell needs shape, rate and sample_rate > 0")
    raise ValueError("ragged_reads: dwell is ('fixed', r), ('uniform', r, w) or ('gamma', shape, rate, sample_rate), got %r" % (dwell,))


def default_max_dwell(dwell):
    """the clamp of the dwell: r for fixed, r + w - 1 for uniform (never reached); for gamma the smallest integer m whose upper
    tail P(g * sample_rate >= m) is below 1e-12 (torch.special.gammaincc in float64, on the host)"""
    model, p0, p1, p2 = _dwell_spec(dwell)
    if model == 0:
        return int(p0)
    if model == 1:
        return int(p0) + int(p1) - 1

    def tail(m):
        return float(torch.special.gammaincc(torch.tensor(p0, dtype=torch.float64), torch.tensor(p1 * m / p2, dtype=torch.float64)))
    hi = 1
    while tail(hi) >= 1e-12:
        hi *= 2
    lo = hi // 2                                                     # tail(lo) >= 1e-12 (or lo == 0), tail(hi) < 1e-12
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if tail(mid) < 1e-12 else (mid, hi)
    return hi


def ragged_kmers(bases, base_lengths, window):
    """5-mer index of every k-mer: bases [B, nmax] (0 past the lengths) -> [B, nmax - 4 - 2 * window] int64, 0 past K_b"""
    w = torch.tensor(KMER_WEIGHTS, device=bases.device, dtype=torch.int64)
    win = (bases.long() - 1).clamp_(min=0).unfold(-1, 5, 1)          # window i = bases[i .. i + 4]
    kmax = bases.shape[1] - 4 - 2 * window
    kmers = (win * w).sum(-1)[:, window:window + kmax]
    live = torch.arange(kmax, device=bases.device)[None, :] < (base_lengths.long() - 4 - 2 * window)[:, None]
    return kmers * live


def hip_reads_plan(batch, min_bases, max_bases, window, dwell, max_dwell, seed, device, bases=None, base_lengths=None,
                   dwell_values=None):
    """wn_reads_plan.  Rows are max_bases wide; given bases / dwell_values (int32, device) must be too.  Returns a dict of the
    outputs, the workspace for hip_reads_signal and the device counters `bad` and `clamped`."""
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("wavenet_speech_amd: the HIP read generator needs a GPU device")
    model, p0, p1, p2 = _dwell_spec(dwell)
    with torch.cuda.device(dev):
        ws_bytes = lib.wn_reads_workspace_bytes(batch, max_bases)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        out = {"base_lengths": torch.empty(batch, **i32), "bases": torch.empty(batch, max_bases, **i32),
               "dwell": torch.empty(batch, max_bases, **i32), "starts": torch.empty(batch, max_bases, **i32),
               "signal_lengths": torch.empty(batch, **i32), "bad": torch.zeros(1, **i32), "clamped": torch.zeros(1, **i32),
               "workspace": ws, "max_bases": max_bases, "window": window}
        _lib.check(lib.wn_reads_plan(ctypes.c_ulonglong(seed), batch, min_bases, max_bases, window, model, p0, p1, p2, int(max_dwell),
                                     _p(base_lengths), _p(bases), _p(dwell_values), _p(out["base_lengths"]), _p(out["bases"]),
                                     _p(out["dwell"]), _p(out["starts"]), _p(out["signal_lengths"]), _p(ws), ws_bytes, _p(out["bad"]),
                                     _p(out["clamped"]), _stream()), "wn_reads_plan")
    return out


def hip_reads_signal(plan, ld, table, seed, noise=None, signal=None, sample_kmer=None):
    """wn_reads_signal on a plan of hip_reads_plan.  noise: float64 [B, ld].  signal / sample_kmer may be given (prefilled
    buffers [B, ld]); returns (signal [B, ld] float32, sample_kmer [B, ld] int32, clipped_lengths [B] int32, bad [1] int32)."""
    lib = _lib.load()
    dev = plan["bases"].device
    B = plan["bases"].shape[0]
    with torch.cuda.device(dev):
        means, stdvs = table
        means, stdvs = means.to(dev).double().contiguous(), stdvs.to(dev).double().contiguous()
        if signal is None:
            signal = torch.empty(B, ld, dtype=torch.float32, device=dev)
        if sample_kmer is None:
            sample_kmer = torch.empty(B, ld, dtype=torch.int32, device=dev)
        clipped = torch.empty(B, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if noise is not None and (noise.dtype != torch.float64 or tuple(noise.shape) != (B, ld) or not noise.is_contiguous()):
            raise RuntimeError("wavenet_speech_amd: noise must be contiguous float64 [B, ld]")
        ws = plan["workspace"]
        _lib.check(lib.wn_reads_signal(_p(plan["base_lengths"]), _p(plan["starts"]), _p(plan["signal_lengths"]), _p(ws), ws.numel(),
                                       B, plan["max_bases"], plan["window"], ld, _p(means), _p(stdvs), ctypes.c_ulonglong(seed),
                                       _p(noise), _p(signal), _p(sample_kmer), _p(clipped), _p(bad), _stream()), "wn_reads_signal")
    return signal, sample_kmer, clipped, bad


def _given_rows(x, width, dev, what):
    """a caller's [B, n] integer rows as int32 [B, width] on dev, zero-padded"""
    x = torch.as_tensor(x).to(device=dev, dtype=torch.int32)
    if x.dim() != 2 or x.shape[1] > width:
        raise ValueError("ragged_reads: %s must be [B, n] with n <= %d" % (what, width))
    out = torch.zeros(x.shape[0], width, dtype=torch.int32, device=dev)
    out[:, :x.shape[1]] = x
    return out


def _torch_reads(batch, lo, max_bases, window, dwell, max_dwell, table, generator, dev, pad_to, bases, base_lengths, dwell_values,
                 noise):
    """ragged_reads as torch ops: the arithmetic of csrc/wn_reads.hip (cumsum for the scan, searchsorted for the k-mer of a
    sample), with the draws taken from the torch generator"""
    model, p0, p1, p2 = _dwell_spec(dwell)
    nmax, trim = max_bases - 1, 4 + 2 * window
    kmax = nmax - trim
    if base_lengths is None:
        base_lengths = torch.randint(lo, max_bases, (batch,), generator=generator, device=dev)
    base_lengths = torch.as_tensor(base_lengths).to(device=dev, dtype=torch.int64)
    if bool(((base_lengths < 5 + 2 * window) | (base_lengths >= max_bases)).any()):
        raise ValueError("ragged_reads: base lengths outside [%d, %d)" % (5 + 2 * window, max_bases))
    live_b = torch.arange(nmax, device=dev)[None, :] < base_lengths[:, None]
    if bases is None:
        bases = torch.randint(1, 5, (batch, nmax), generator=generator, device=dev)
    else:
        bases = _given_rows(bases, nmax, dev, "bases").long()
        if bool((((bases < 1) | (bases > 4)) & live_b).any()):
            raise ValueError("ragged_reads: bases outside 1..4")
    bases = bases * live_b
    K = base_lengths - trim
    live_k = torch.arange(kmax, device=dev)[None, :] < K[:, None]
    if dwell_values is not None:
        d = _given_rows(dwell_values, kmax, dev, "dwell_values").long()
        if bool(((d < 1) & live_k).any()):
            raise ValueError("ragged_reads: dwell values below 1")
    elif model == 0:
        d = torch.full((batch, kmax), int(p0), dtype=torch.int64, device=dev)
    elif model == 1:
        r, w = int(p0), int(p1)
        d = torch.randint(max(r - w, 1), r + w, (batch, kmax), generator=generator, device=dev)
    else:
        g = torch._standard_gamma(torch.full((batch, kmax), p0, dtype=torch.float64, device=dev), generator=generator)
        d = (g / p1 * p2).clamp_(max=float(max_dwell) + 1.0).long().clamp_(min=1)
    d = d.clamp(max=int(max_dwell)) * live_k
    starts = torch.cat([torch.zeros(batch, 1, dtype=torch.int64, device=dev), d.cumsum(1)], 1)      # [B, kmax + 1]
    signal_lengths = starts[:, -1]
    if pad_to is None:
        ld = max(int(signal_lengths.max()), 1)
    else:
        ld = int(pad_to)
        if bool((signal_lengths > ld).any()):
            raise RuntimeError("ragged_reads: a read is longer than pad_to = %d samples" % ld)
    t = torch.arange(ld, device=dev)[None, :].expand(batch, ld).contiguous()
    p = torch.searchsorted(starts[:, 1:].contiguous(), t, right=True)                              # starts[p] <= t < starts[p + 1]
    inside = t < signal_lengths[:, None]
    kmers = ragged_kmers(bases, base_lengths, window)
    k = kmers.gather(1, p.clamp(max=kmax - 1))
    means, stdvs = table
    means, stdvs = means.to(dev).double(), stdvs.to(dev).double()
    if noise is None:
        z = torch.randn(batch, ld, generator=generator, device=dev, dtype=torch.float64)
    else:
        z = torch.as_tensor(noise).to(device=dev, dtype=torch.float64)[:, :ld]
        if z.shape != (batch, ld):
            raise ValueError("ragged_reads: noise must be [B, >= %d]" % ld)
    signal = ((means[k] + stdvs[k] * z).float() * inside).unsqueeze(1)
    sample_kmer = torch.where(inside, p, torch.full_like(p, -1)).int()
    targets = bases[live_b].int()
    return RaggedReads(signal, signal_lengths.int(), bases.int(), base_lengths.int(), targets, d.int(), starts.int(), sample_kmer)


def ragged_reads(batch, lengths=(20, 30), dwell=("uniform", 6, 2), window="loader", table=None, generator=None, device="cpu",
                 pad_to=None, max_dwell=None, bases=None, base_lengths=None, dwell_values=None, noise=None):
    """A batch of ragged synthetic reads (RaggedReads): base lengths uniform in [lengths[0], lengths[1]), random bases, every
    k-mer held for a random dwell, signal = N(mean[kmer], stdv[kmer]) in float64 rounded to float32, zero-padded.

    dwell   ("uniform", r, w): integer in [max(r - w, 1), r + w), the loader's random_upsample; ("fixed", r);
            ("gamma", shape, rate, sample_rate): max(1, int(Gamma(shape, 1 / rate) * sample_rate)), RawSignalGenerator's
    window  "loader": k-mer p = bases[p+2 .. p+6] (n - 8 k-mers from n bases); "generator": bases[p .. p+4] (n - 4 k-mers)
    pad_to  None: the signal is as long as the longest read -- one host read of signal_lengths.max() between the two launches,
            as the reference's batchify; L: rows of L samples, no host synchronisation, static shapes (usable under GraphedStep);
            a read longer than L is truncated and reported by check_device_flags()
            (the Philox seed is drawn from `generator` on the host at call time: a captured call replays the same batch)
    bases, base_lengths, dwell_values, noise   replace the corresponding draw (bases [B, n], dwell_values [B, K], noise
            float64 [B, >= Lpad]); with `bases` and no base_lengths every read has n bases
    On a GPU all of it is csrc/wn_reads.hip (no fallback); on the CPU the same arithmetic as torch ops, with the draws taken from
    the torch generator: the two agree bit for bit on given bases, dwell and noise, not on drawn ones."""
    dev = torch.device(device)
    win = WINDOWS[window] if isinstance(window, str) else int(window)
    if win not in (0, 2):
        raise ValueError("ragged_reads: window is 'loader' or 'generator'")
    lo, hi = int(lengths[0]), int(lengths[1])
    if bases is not None:
        bases = torch.as_tensor(bases)
        hi = max(hi, bases.shape[1] + 1) if base_lengths is not None else bases.shape[1] + 1
        if base_lengths is None:
            base_lengths = torch.full((bases.shape[0],), bases.shape[1], dtype=torch.int32)
        lo = min(lo, hi - 1)
    if lo < 5 + 2 * win or lo >= hi:
        raise ValueError("ragged_reads: lengths must satisfy %d <= lo < hi" % (5 + 2 * win))
    _dwell_spec(dwell)
    if max_dwell is None:
        max_dwell = default_max_dwell(dwell)
        if dwell_values is not None:
            max_dwell = 2 ** 31 // hi - 1
    if max_dwell < 1 or (hi - 5) * max_dwell >= 2 ** 31:
        raise ValueError("ragged_reads: max_dwell must be >= 1 and (max_bases - 5) * max_dwell < 2^31")
    if table is None:
        table = standin_kmer_table(device=dev)
    if dev.type != "cuda":
        if generator is not None and torch.device(generator.device).type != dev.type:
            generator = torch.Generator(device=dev).manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator)))
        return _torch_reads(batch, lo, hi, win, dwell, max_dwell, table, generator, dev, pad_to, bases, base_lengths, dwell_values,
                            noise)
    seed = _device_seed(generator, dev)
    nmax, kmax = hi - 1, hi - 1 - 4 - 2 * win
    with torch.cuda.device(dev):
        gb = None if bases is None else _given_rows(bases, hi, dev, "bases")
        gl = None if base_lengths is None else torch.as_tensor(base_lengths).to(device=dev, dtype=torch.int32).contiguous()
        gd = None if dwell_values is None else _given_rows(dwell_values, hi, dev, "dwell_values")
        plan = hip_reads_plan(batch, lo, hi, win, dwell, max_dwell, seed, dev, gb, gl, gd)
        poisoned = "wavenet_speech_amd: ragged_reads: %d read(s) with a length out of range, bases outside 1..4 or dwell below 1"
        _args.note_bad(plan["bad"], lambda n: poisoned % n, at_once=pad_to is None)
        if pad_to is None:
            ld = max(int(plan["signal_lengths"].max()), 1)             # the one host read, as batchify's max()
        else:
            ld = int(pad_to)
        nz = None
        if noise is not None:
            nz = torch.as_tensor(noise).to(device=dev, dtype=torch.float64)
            if nz.dim() != 2 or nz.shape[0] != batch or nz.shape[1] < ld:
                raise ValueError("ragged_reads: noise must be [B, >= %d]" % ld)
            nz = nz[:, :ld].contiguous()
        signal, sample_kmer, clipped, bad = hip_reads_signal(plan, ld, table, seed, nz)
        if pad_to is not None:
            _flags.WATCH.note(bad, lambda n, ld=ld: "wavenet_speech_amd: ragged_reads: %d read(s) longer than pad_to = %d samples "
                              "were truncated" % (n, ld), at_once=False)
        out_bases = plan["bases"][:, :nmax]
        targets = None
        if pad_to is None:
            targets = out_bases[torch.arange(nmax, device=dev)[None, :] < plan["base_lengths"][:, None]]
    return RaggedReads(signal.unsqueeze(1), clipped, out_bases, plan["base_lengths"], targets, plan["dwell"][:, :kmax],
                       plan["starts"][:, :kmax + 1], sample_kmer)


class RawGaussianModelLoader(object):
    """The reference's on-line loader of raw Gaussian 5-mer reads (utils/gaussian_kmer_model.py RawGaussianModelLoader) on top of
    ragged_reads: same constructor, counters and stopping rule.  kmer_model_path: an .npz with `means` and `stdvs` (1024 each),
    or None for the stand-in table.  fetch() -> (signal [B, Lmax] float32, seq int32 concatenated bases, lengths int32 [B]);
    fetch_reads() -> the full RaggedReads (dwell, starts, signal lengths).  After cuda() the batch is generated on the GPU."""

    def __init__(self, max_iters, num_epochs, epoch_size, kmer_model_path, batch_size=1, upsampling=3, random_upsample=False,
                 lengths=(20, 30)):
        self.max_iters, self.num_epochs, self.epoch_size = max_iters, num_epochs, epoch_size
        self.batch_size, self.upsampling, self.random_upsample = batch_size, upsampling, random_upsample
        self.min_length, self.max_length = lengths
        self.path_to_model = kmer_model_path
        self.counter, self.epochs, self.on_cuda = 0, 0, False
        self.generator = None
        self.num_kmers = 4 ** 5
        if kmer_model_path is None:
            self.kmer_means, self.kmer_stdvs = standin_kmer_table()
        else:
            import numpy as np
            npz = np.load(kmer_model_path)
            self.kmer_means, self.kmer_stdvs = torch.as_tensor(npz["means"]).double(), torch.as_tensor(npz["stdvs"]).double()

    def _dwell(self):
        if self.upsampling <= 1:
            return ("fixed", 1)                                          # the reference upsamples only above 1
        return ("uniform", self.upsampling, 2) if self.random_upsample else ("fixed", self.upsampling)

    def fetch_reads(self, **given):
        self.maybe_stop()
        reads = ragged_reads(self.batch_size, (self.min_length, self.max_length), self._dwell(), "loader",
                             (self.kmer_means, self.kmer_stdvs), self.generator, "cuda" if self.on_cuda else "cpu", **given)
        self.tick()
        return reads

    def fetch(self):
        reads = self.fetch_reads()
        return reads.signal[:, 0, :], reads.targets, reads.base_lengths

    def cuda(self):
        self.on_cuda = True

    def cpu(self):
        self.on_cuda = False

    def tick(self):
        self.counter += 1
        if self.counter % self.epoch_size == 0:
            self.epochs += 1

    def maybe_stop(self):
        if self.epochs == self.num_epochs or self.counter == self.max_iters:
            raise StopIteration
