"""
Realignment of reads against the called haplotypes on the device (csrc/wn_realign.hip through
wn_haplotype_windows and wn_lift_ops, around the unchanged pairwise_align): the step GATK's indel realigner and HaplotypeCaller,
longshot and margin run after the calls.  A read aligned alone against the plain reference prefers, near its end or beside a
sequencing error, mismatches or a free end gap to the gap the sample really carries.  Against the two called haplotypes it lies on
one of them without that gap; the score difference says which one, and that alignment, carried back to reference coordinates,
shows the called alleles wherever the read supports them.

    g = call_genotypes(pile, ev, index, w); sites = phase_sites(g); phasing = phase_chain(phase_links(*reads, sites), sites)
    hcalls = haplotype_calls(g, sites, phasing)                        # what each haplotype carries at every position
    r = realign(ref, ref_lengths, labels, lengths, lo, m.strand, hcalls, index)
    r.hp, r.delta                                                      # a haplotype tag that also works where only indels inform
    aln = left_align(r.alignment, ref, ref_lengths, labels, lengths, m.strand).alignment
    pile2 = pileup(aln, lo, ref_lengths, m.strand, labels, lengths, index.R, ...)      # r.alignment is an op row like any other

    hcalls = haplotype_calls(call_consensus(pile, index))              # one haplotype: a polishing round against the consensus

Everything the kernels write is an integer, so results equal the host reference of tests/realign_ref.py exactly and two runs are
bitwise identical.  Nothing here synchronises with the host, so the whole of realign() can be captured in one graph.  There is no
CPU fallback: CPU tensors raise.
Not built: phasing of heterozygous insertions (an INS_HET insertion lies on neither haplotype and comes back as the read's own
insertion columns), more than two haplotypes, a band around the read's first alignment (the DP is the full pairwise_align), new
candidate haplotypes assembled from the reads.
"""
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import (MAX_BAND, MAX_OPS, MAX_PAIR_QUERY, MAX_PAIR_REF, OP_QUERY_GAP, OP_REF_GAP, PairwiseAlignment, _alignment_ops, _clamp_band,
                       _op_rows, _pair_rows, band_from_ops, banded_align, pairwise_align)
from .genotype import Genotypes
from .phase import PhaseSites, Phasing
from .pileup import MAX_INS, ConsensusCalls, _reference_labels
from .readmap import MAX_REFERENCE, _int_in

MAX_HAPLOTYPES = 2
MAX_HAP_OPS = MAX_PAIR_REF                    # of a haplotype's window: pairwise_align's reference limit
DEFAULT_MAX_BAND = 512                        # realign(first=, band=): the widest stripe of banded_align's one-wave form

HaplotypeCalls = namedtuple("HaplotypeCalls", "call ins_len ins_bases")
HaplotypeCalls.__doc__ = """call [H, R] uint8: the label haplotype h carries at forward position p, 0 where it is deleted; ins_len [H, R] uint8:
the length of the insertion it carries after p; ins_bases [H, R, max_ins] uint8: its bases.  H is 2 (haplotype 1 and 2 of a
Phasing) or 1 (a consensus).  All on the device."""

HaplotypeWindows = namedtuple("HaplotypeWindows", "labels lengths ops ops_len used")
HaplotypeWindows.__doc__ = """labels [H, B, max_hap_ops] int32 with lengths [H, B] int32: haplotype h over the window of read b in read
orientation, pairwise_align's `ref`; ops [H, B, max_hap_ops] uint8 with ops_len [H, B] int32: the haplotype against the reference
window (1 / 2 both, 3 a reference label the haplotype lacks, 4 a haplotype label the reference lacks); used [B] int8: 1 written, 0
skipped, -1 bad.  Rows are zero behind their lengths.  All on the device."""

Realignment = namedtuple("Realignment", "alignment pick hp delta scores")
Realignment.__doc__ = """alignment: a PairwiseAlignment of every read against its REFERENCE window, through the haplotype it lies on;
pick [B] int32: that haplotype's index (the greater score, ties to 0); hp [B] uint8: 1 or 2, 0 on a tie or for a read that was
skipped or bad; delta [B] fp32: |scores[:, 0] - scores[:, 1]|; scores [B, H] fp32: pairwise_align's score against each haplotype.
All on the device."""


def _table(x, what, name, device=None):
    """a uint8 tensor of haplotype_calls, on the device of the first one"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or (device is not None and x.device != device):
        raise ValueError("wavenet_speech_amd.%s: %s must be a uint8 tensor%s" % (what, name, " on %s" % device if device is not None else ""))
    return x.detach()


def haplotype_calls(genotypes, sites=None, phasing=None):
    """What each haplotype carries at every position, built with torch ops on the device the tables are on:
    no kernel and no host synchronisation.  genotypes: the Genotypes of call_genotypes with sites, the PhaseSites, and phasing, the
    Phasing of phase_chain -> H = 2.  A position that is no site carries alleles[p, 0] on both haplotypes (LOW_DEPTH positions and
    reference labels that are no base are called (r, r)); a site s carries alleles[s, parity[s] xor h] on haplotype h -- sites with
    set_size 1 included, their parity is 0.  An insertion with ins_copies == 2 lies on both haplotypes, one with ins_copies == 1
    (INS_HET: not phased) on neither: it comes back as the read's own insertion columns.  With S == 0 both haplotypes are equal.
    genotypes: a ConsensusCalls alone -> H = 1 from its call / ins_len / ins_bases, for a polishing round against the consensus.
    Returns HaplotypeCalls.  Like the host helpers it takes tensors on any device; haplotype_windows and realign, which launch
    kernels, refuse CPU tensors."""
    what = "haplotype_calls"
    if isinstance(genotypes, ConsensusCalls):
        if sites is not None or phasing is not None:
            raise ValueError("wavenet_speech_amd.%s: a ConsensusCalls is one haplotype: it takes no sites and no phasing" % what)
        call = _table(genotypes.call, what, "calls.call")
        ins_len, ins_bases = (_table(getattr(genotypes, n), what, "calls." + n, call.device) for n in ("ins_len", "ins_bases"))
        R = int(call.shape[0]) if call.dim() == 1 else -1
        if tuple(ins_len.shape) != (R,) or ins_bases.dim() != 2 or int(ins_bases.shape[0]) != R:
            raise ValueError("wavenet_speech_amd.%s: calls must hold call (R,), ins_len (R,) and ins_bases (R, max_ins), got %s, %s, %s"
                             % (what, tuple(call.shape), tuple(ins_len.shape), tuple(ins_bases.shape)))
        return HaplotypeCalls(call.contiguous()[None], ins_len.contiguous()[None], ins_bases.contiguous()[None])
    if not isinstance(genotypes, Genotypes):
        raise ValueError("wavenet_speech_amd.%s: genotypes must be Genotypes or ConsensusCalls, got %s" % (what, type(genotypes).__name__))
    if not isinstance(sites, PhaseSites) or not isinstance(phasing, Phasing):
        raise ValueError("wavenet_speech_amd.%s: Genotypes need sites, a PhaseSites, and phasing, a Phasing" % what)
    alleles = _table(genotypes.alleles, what, "genotypes.alleles")
    dev = alleles.device
    copies, ins_len, ins_bases = (_table(getattr(genotypes, n), what, "genotypes." + n, dev) for n in ("ins_copies", "ins_len", "ins_bases"))
    R = int(alleles.shape[0]) if alleles.dim() == 2 else -1
    if tuple(alleles.shape) != (R, 2) or tuple(copies.shape) != (R,) or tuple(ins_len.shape) != (R,) or ins_bases.dim() != 2 or int(ins_bases.shape[0]) != R:
        raise ValueError("wavenet_speech_amd.%s: genotypes must hold alleles (R, 2), ins_copies (R,), ins_len (R,) and ins_bases (R, max_ins), got "
                         "%s, %s, %s, %s" % (what, tuple(alleles.shape), tuple(copies.shape), tuple(ins_len.shape), tuple(ins_bases.shape)))
    site_alleles, parity = _table(sites.alleles, what, "sites.alleles", dev), _table(phasing.parity, what, "phasing.parity", dev)
    pos = sites.pos
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int32 or pos.device != dev or pos.dim() != 1:
        raise ValueError("wavenet_speech_amd.%s: sites.pos must be an int32 tensor of shape (S,) on %s" % (what, dev))
    S = int(pos.shape[0])
    if tuple(site_alleles.shape) != (S, 2) or tuple(parity.shape) != (S,) or S > R:
        raise ValueError("wavenet_speech_amd.%s: %d sites on %d positions with alleles %s and parity %s" % (what, S, R, tuple(site_alleles.shape), tuple(parity.shape)))
    call = alleles[:, 0].unsqueeze(0).repeat(2, 1)
    at = pos.long()
    for h in range(2):
        call[h, at] = site_alleles.gather(1, (parity ^ h).long().unsqueeze(1)).squeeze(1)
    both = copies == 2
    ins_len = torch.where(both, ins_len, torch.zeros_like(ins_len)).unsqueeze(0).repeat(2, 1)
    ins_bases = (ins_bases * both.to(torch.uint8).unsqueeze(1)).unsqueeze(0).repeat(2, 1, 1)
    return HaplotypeCalls(call, ins_len, ins_bases)


def _hcalls(hcalls, what):
    """a HaplotypeCalls checked -> (H, R, max_ins, device)"""
    if not isinstance(hcalls, HaplotypeCalls):
        raise ValueError("wavenet_speech_amd.%s: hcalls must be HaplotypeCalls, got %s" % (what, type(hcalls).__name__))
    call = _args.gpu_tensor(hcalls.call, what, "hcalls.call", (torch.uint8,))
    dev = call.device
    for name in ("ins_len", "ins_bases"):
        _args.gpu_tensor(getattr(hcalls, name), what, "hcalls." + name, (torch.uint8,), device=dev)
    if call.dim() != 2 or hcalls.ins_len.shape != call.shape or hcalls.ins_bases.dim() != 3 or hcalls.ins_bases.shape[:2] != call.shape or not all(
            t.is_contiguous() for t in hcalls):
        raise ValueError("wavenet_speech_amd.%s: hcalls must hold contiguous call (H, R), ins_len (H, R) and ins_bases (H, R, max_ins), got %s, %s, %s"
                         % (what, tuple(call.shape), tuple(hcalls.ins_len.shape), tuple(hcalls.ins_bases.shape)))
    H, R, max_ins = int(call.shape[0]), int(call.shape[1]), int(hcalls.ins_bases.shape[2])
    if not 1 <= H <= MAX_HAPLOTYPES or not 1 <= R <= MAX_REFERENCE or max_ins > MAX_INS:
        raise ValueError("wavenet_speech_amd.%s: need 1 or 2 haplotypes over 1 to %d positions with max_ins at most %d, got %d over %d with %d"
                         % (what, MAX_REFERENCE, MAX_INS, H, R, max_ins))
    return H, R, max_ins, dev


def _batch_of(lo, what):
    lo = torch.as_tensor(lo)
    if lo.dim() != 1 or not 1 <= int(lo.shape[0]) <= 65535:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 reads, got lo of shape %s" % (what, tuple(lo.shape)))
    return int(lo.shape[0])


def haplotype_windows(hcalls, reference, lo, ref_lengths, strand, max_hap_ops=None):
    """Every haplotype over the window of every read, in read orientation, one launch and no host
    synchronisation.  hcalls: the HaplotypeCalls; reference: a ReadIndex or [R] labels; lo, ref_lengths, strand [B]: mapping.window(flank)
    and mapping.strand, as pileup takes them; max_hap_ops in [1, 65535]: the columns of a row (None: min(65535, R * (1 + max_ins)),
    which always suffices; the widest window times 1 + max_ins does too and is smaller).
    In forward order position p of [lo, lo + n) gives, with v = call[h, p]: v == 0: op 3 and no label; else the label v and op 1 if
    v == reference[p], else op 2; then, only for p < lo + n - 1, ins_len[h, p] labels with op 4 -- the insertion after the window's
    last position is outside the window, by pileup's rule.  On strand 1 both rows are reversed and labels 1..4 complemented: pileup's
    orientation, so `labels` goes straight into pairwise_align as `ref`.
    Returns HaplotypeWindows.  A read with strand < 0 or ref_lengths == 0 is skipped (lengths 0, used 0).  A read with strand > 1, a
    window outside [0, R], an ins_len above max_ins or a row of any haplotype that needs more than max_hap_ops ops is bad: lengths 0
    on every haplotype, used -1, never a truncated row; it is reported through check_device_flags()."""
    what = "haplotype_windows"
    H, R, max_ins, dev = _hcalls(hcalls, what)
    reference = _reference_labels(reference, R, dev, what)
    B = _batch_of(lo, what)
    lo, ref_lengths, strand = (_args.lengths(x, B, dev, what, name) for x, name in ((lo, "lo"), (ref_lengths, "ref_lengths"), (strand, "strand")))
    cap = _int_in(what, "max_hap_ops", min(MAX_HAP_OPS, R * (1 + max_ins)) if max_hap_ops is None else max_hap_ops, 1, MAX_HAP_OPS)
    with torch.cuda.device(dev):
        labels = torch.empty(H, B, cap, dtype=torch.int32, device=dev)
        ops = torch.empty(H, B, cap, dtype=torch.uint8, device=dev)
        lengths, ops_len = (torch.empty(H, B, dtype=torch.int32, device=dev) for _ in range(2))
        used = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().wn_haplotype_windows(_p(hcalls.call), _p(hcalls.ins_len), _p(hcalls.ins_bases) if max_ins else None, _p(reference),
                                                    _p(lo), _p(ref_lengths), _p(strand), H, B, R, max_ins, cap, _p(labels), _p(lengths), _p(ops),
                                                    _p(ops_len), _p(used), _p(bad), _stream()), "wn_haplotype_windows")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.%s: %d read(s) whose window does not fit: a strand above 1, a window outside [0, %d], "
                       "an ins_len above %d or a row of more than %d ops" % (what, n, R, max_ins, cap))
    return HaplotypeWindows(labels, lengths, ops, ops_len, used)


def _windows(windows, what, B, dev):
    """a HaplotypeWindows' ops, ops_len, lengths and used checked (labels are not looked at) -> (H, ops as the C ABI takes them)"""
    if not isinstance(windows, HaplotypeWindows):
        raise ValueError("wavenet_speech_amd.%s: windows must be HaplotypeWindows, got %s" % (what, type(windows).__name__))
    ops = _args.gpu_tensor(windows.ops, what, "windows.ops", (torch.uint8,), device=dev)
    for name, dtype in (("ops_len", torch.int32), ("lengths", torch.int32), ("used", torch.int8)):
        _args.gpu_tensor(getattr(windows, name), what, "windows." + name, (dtype,), device=dev)
    H = int(ops.shape[0]) if ops.dim() == 3 else 0
    if not 1 <= H <= MAX_HAPLOTYPES or int(ops.shape[1]) != B or not 1 <= int(ops.shape[2]) <= MAX_HAP_OPS or tuple(windows.ops_len.shape) != (H, B) or \
            tuple(windows.lengths.shape) != (H, B) or tuple(windows.used.shape) != (B,):
        raise ValueError("wavenet_speech_amd.%s: windows must hold ops (H, %d, n), H 1 or 2 and n in [1, %d], ops_len and lengths (H, %d) and used "
                         "(%d,), got %s, %s, %s, %s" % (what, B, MAX_HAP_OPS, B, B, tuple(ops.shape), tuple(windows.ops_len.shape),
                                                        tuple(windows.lengths.shape), tuple(windows.used.shape)))
    if ops.stride(2) != 1 and ops.shape[2] > 1 or ops.stride(0) < 0 or ops.stride(1) < 0:
        ops = ops.contiguous()
    return H, ops


def lift_alignment(alignments, windows, pick, ref, ref_lengths, query, query_lengths, match=5, mismatch=-4, gap_open=10, gap_extend=0.5,
                   end_gaps_free=True, max_ops=None):
    """Carries the alignment of every read against its picked haplotype back to reference coordinates, one
    launch and no host synchronisation.  alignments: the PairwiseAlignment of the reads against each haplotype, a list of H (one may
    be given alone), exactly as pairwise_align(windows.labels[h], windows.lengths[h], query, query_lengths) returns them; windows: the
    HaplotypeWindows; pick [B]: the haplotype of each read; ref [B, N] with ref_lengths [B]: the reference window in read orientation
    (mapping.labels(flank)); query [B, M] with query_lengths [B]: the reads; the costs: pairwise_align's, for the score of the result;
    max_ops: the columns of the result's rows (None: N + M, which always suffices).
    Row b of alignments[pick[b]] is A (1 / 2 both, 3 a haplotype label only, 4 a read label only), row b of windows.ops[pick[b]] is Hh
    (1 / 2 both, 3 a reference label only, 4 a haplotype label only).  Their composition is the loop of tests/realign_ref.py:
        while Hh's next op is 3: emit 3;  while A's next op is 4: emit 4 (always after the 3s of the same slot);  both used up: stop;
        a = A's next op is 1 or 2, g = Hh's next op is 1 or 2; take both (they share one haplotype label);
        a and g: 1 if ref[i] == query[j] else 2, compared afresh;  a only: 4;  g only: 3;  neither: nothing.
    Returns a PairwiseAlignment of the read against its reference window: ops, ops_len, matches, mismatches, gaps, length, and the
    score under the given costs with pairwise_align's end-gap rule.  It consumes exactly ref_lengths and query_lengths labels, so it
    goes unchanged into left_align, pileup, pileup_evidence, phase_links and haplotag.  NO PROMISE is made that this score is at
    least the score of the read's own alignment against the reference: where the calls and the read disagree it is lower (on the
    planted run of tests/phase_cases.py for 3 reads of 160, for 6 in the noisy variant, and equal for the rest) -- the price of
    agreeing with the calls.
    A skipped window passes through (ops_len 0, zeros).  A row with a bad window, a pick outside [0, H), a length out of range, an op
    outside 1..4, rows that do not consume exactly their labels, or a result longer than max_ops is bad: ops_len 0, counts -1, score
    -2^30 as pairwise_align's poisoned pair; it is reported through check_device_flags()."""
    what = "lift_alignment"
    costs = _args.affine_costs(what, match, mismatch, gap_open, gap_extend)
    if isinstance(alignments, PairwiseAlignment):
        alignments = [alignments]
    if not isinstance(alignments, (list, tuple)) or not 1 <= len(alignments) <= MAX_HAPLOTYPES:
        raise ValueError("wavenet_speech_amd.%s: alignments must be one PairwiseAlignment per haplotype, 1 or 2" % what)
    rows = [_alignment_ops(a, what) for a in alignments]
    ref, ref_lengths = _pair_rows(ref, ref_lengths, what, "ref")
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, N, M, dev = int(ref.shape[0]), int(ref.shape[1]), int(query.shape[1]), ref.device
    if query.shape[0] != B or query.device != dev:
        raise ValueError("wavenet_speech_amd.%s: ref and query must hold the same number of rows on one device" % what)
    if B < 1 or B > 65535 or N > MAX_PAIR_REF or M > MAX_PAIR_QUERY:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 reads of at most %d labels against at most %d, got %d of %d against %d"
                         % (what, MAX_PAIR_QUERY, MAX_PAIR_REF, B, M, N))
    H, hap_ops = _windows(windows, what, B, dev)
    if len(rows) != H:
        raise ValueError("wavenet_speech_amd.%s: %d alignment(s) beside windows of %d haplotype(s)" % (what, len(rows), H))
    rows = [_op_rows(ops, ops_len, B, dev, what, on="query") for ops, ops_len in rows]
    pick = _args.lengths(pick, B, dev, what, "pick")
    max_ops = _int_in(what, "max_ops", min(MAX_OPS, N + M) if max_ops is None else max_ops, 1, MAX_OPS)
    lib = _lib.load()
    with torch.cuda.device(dev):
        if H == 1:
            a_ops, a_len, a_hap_stride = rows[0][0], rows[0][1], 0
        else:
            width = max(r[2] for r in rows)
            a_ops = torch.stack([torch.nn.functional.pad(r[0], (0, width - r[2])) for r in rows])
            a_len, a_hap_stride = torch.stack([r[1] for r in rows]), a_ops.stride(0)
        max_hap_len = int(hap_ops.shape[2])                          # a haplotype's labels are columns of its row
        ops = torch.empty(B, max_ops, dtype=torch.uint8, device=dev)
        ops_len, score = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
        stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
        ws_bytes = lib.wn_lift_ops_workspace_bytes(B, max_hap_len)
        ws = _args._alloc_bytes(ws_bytes, "wn_lift_ops_workspace_bytes", dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_lift_ops(_p(a_ops), a_hap_stride, a_ops.stride(-2), _p(a_len), int(a_ops.shape[-1]), _p(hap_ops), hap_ops.stride(0),
                                   hap_ops.stride(1), _p(windows.ops_len.contiguous()), _p(windows.lengths.contiguous()), int(hap_ops.shape[2]),
                                   max_hap_len, _p(windows.used.contiguous()), _p(pick), _p(ref), ref.stride(0), _p(ref_lengths), _p(query),
                                   query.stride(0), _p(query_lengths), H, B, N, M, max_ops, costs[0], costs[1], costs[2], costs[3],
                                   int(bool(end_gaps_free)), _p(ops), ops.stride(0), _p(ops_len), _p(score), _p(stats), _p(ws), ws_bytes, _p(bad),
                                   _stream()), "wn_lift_ops")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.%s: %d read(s) whose rows do not compose: a bad window, a pick outside [0, %d), a length "
                       "out of range, an op outside 1..4, labels not consumed exactly or a result of more than %d ops" % (what, n, H, max_ops))
    return PairwiseAlignment(score.float() * 0.5, stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], ops, ops_len)


def realign(ref, ref_lengths, query, query_lengths, lo, strand, hcalls, reference, match=5, mismatch=-4, gap_open=10, gap_extend=0.5,
            end_gaps_free=True, max_hap_ops=None, first=None, band=None, max_band=DEFAULT_MAX_BAND):
    """Realigns every read against the haplotypes of `hcalls` and carries the better alignment back to its reference window
    (DESIGN.md section 7aa).  ref [B, N], ref_lengths, lo, strand: mapping.labels(flank), mapping.window(flank) and mapping.strand;
    query [B, M], query_lengths: the reads -- exactly what pairwise_align and pileup were given; hcalls: haplotype_calls'; reference: a
    ReadIndex or [R] labels; the costs: pairwise_align's; max_hap_ops: haplotype_windows' (None: min(65535, N * (1 + max_ins)), which
    always suffices).
    The steps: haplotype_windows; pairwise_align once per haplotype; scores [B, H]; pick, the greater score, ties to haplotype 0; hp,
    1 or 2, 0 on a tie or for a skipped or bad read; delta = |scores[:, 0] - scores[:, 1]| (0 with one haplotype); lift_alignment.
    Torch ops and three entry points, no host synchronisation: the whole of it can be captured in one graph.
    first, band: both or neither.  With them the alignment against haplotype h is banded_align's instead of
    the full matrix: first is the read's own PairwiseAlignment against `ref` (with ops) and band a margin in diagonals.  With
    (lo1, hi1) = band_from_ops(first) and n3, n4 the counts of op 3 and op 4 in row (h, b) of the windows' ops, the stripe is
    [lo1 - n4 - band, hi1 + n3 + band]: the haplotype's index differs from the reference's by at most that many labels, so the
    read's first path, carried onto the haplotype, lies inside it.  max_band (a host integer, by default 512: the widest stripe one
    wave holds) sizes the launch; a wider stripe is clamped about its centre.  A read whose better path leaves the stripe gets a
    lower score than the full matrix gives, never a higher one.  Still no host synchronisation.
    Returns Realignment.  Its alignment is lift_alignment's: see there for what its score does NOT promise."""
    what = "realign"
    if (first is None) != (band is None):
        raise ValueError("wavenet_speech_amd.%s: first and band come together" % what)
    H, R, max_ins, dev = _hcalls(hcalls, what)
    ref, ref_lengths = _pair_rows(ref, ref_lengths, what, "ref")
    if max_hap_ops is None:
        max_hap_ops = min(MAX_HAP_OPS, int(ref.shape[1]) * (1 + max_ins))
    costs = dict(match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend, end_gaps_free=end_gaps_free)
    windows = haplotype_windows(hcalls, reference, lo, ref_lengths, strand, max_hap_ops)
    if first is None:
        alignments = [pairwise_align(windows.labels[h], windows.lengths[h], query, query_lengths, **costs) for h in range(H)]
    else:
        band = _int_in(what, "band", band, 0, MAX_BAND)
        lo1, hi1 = band_from_ops(first, end_gaps_free=end_gaps_free)
        if lo1.shape[0] != ref.shape[0] or lo1.device != dev:
            raise ValueError("wavenet_speech_amd.%s: first must hold one row per read on the device of the reads" % what)
        inside = torch.arange(windows.ops.shape[2], device=dev) < windows.ops_len.unsqueeze(2)
        n3 = ((windows.ops == OP_REF_GAP) & inside).sum(2, dtype=torch.int32)
        n4 = ((windows.ops == OP_QUERY_GAP) & inside).sum(2, dtype=torch.int32)
        alignments = []
        for h in range(H):
            dlo, dhi = _clamp_band(lo1 - n4[h] - band, hi1 + n3[h] + band, max_band)
            alignments.append(banded_align(windows.labels[h], windows.lengths[h], query, query_lengths, dlo, dhi, max_band, **costs).alignment)
    with torch.cuda.device(dev):
        scores = torch.stack([a.score for a in alignments], 1)
        other = scores[:, H - 1]
        pick = (other > scores[:, 0]).to(torch.int32)
        decided = (windows.used == 1) & (other != scores[:, 0])
        hp = torch.where(decided, pick + 1, torch.zeros_like(pick)).to(torch.uint8)
        delta = (scores[:, 0] - other).abs()
    lifted = lift_alignment(alignments, windows, pick, ref, ref_lengths, query, query_lengths, **costs)
    return Realignment(lifted, pick, hp, delta, scores)
