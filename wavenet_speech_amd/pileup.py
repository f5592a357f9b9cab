"""
Pileup, consensus and variant calls on the device (csrc/wn_pileup.hip through wn_pileup, wn_consensus_call
and wn_consensus_emit): what the mapped reads of a locus show together -- the step samtools mpileup / consensus and bcftools call
run after mapping, and the counting front end of medaka and racon.

    index = read_index(reference_bases)
    m = map_reads(labels, lengths, index)
    ref, ref_lengths = m.labels(flank=8)                               # the mapped stretch in read orientation
    lo, _ = m.window(flank=8)                                          # where that stretch lies on the forward strand
    aln = pairwise_align(ref, ref_lengths, labels, lengths)
    pile = pileup(aln, lo, ref_lengths, m.strand, labels, lengths, index.R, qual=q.qual, min_qual=7, keep=m.mapq() >= 20)
    pile = pileup(aln2, ..., into=pile)                                # the pile grows over batches
    calls = call_consensus(pile, index)
    print("".join(vcf_records("chr", index, calls, pile)))             # calls.consensus goes back into read_index / pairwise_align

Everything the kernels write is an integer and every rule is an integer comparison, so results equal the host reference of
tests/pileup_ref.py exactly and two runs are bitwise identical.  pileup does not synchronise with the host; call_consensus does
once, to size the consensus.  There is no CPU fallback: CPU tensors raise (the host helpers variant_records / vcf_records take
tensors on any device).

Labels are the decoders': 1..4 = A, G, C, T (DEFAULT_ALPHABET " AGCT"), the complement of v is 5 - v.
A gap inside a repeat is placed by pairwise_align's tie rule in READ orientation, so forward and reverse reads may place it at
opposite ends of the repeat and split its support: left_align (leftalign.py) between pairwise_align and pileup normalises that.
Genotype likelihoods and diploid calls with QUAL are genotype.py's, on the same reads beside these tables.
Realignment against the called haplotypes is realign.py's.
Not built: a strand split for insertions, more than one reference ([R] positions of one row).
"""
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import DEFAULT_ALPHABET, MAX_OPS, MAX_PAIR_QUERY, MAX_QUAL, TILE, _alignment_ops, _op_rows, _pair_rows, _profile_rows
from .readmap import MAX_REFERENCE, ReadIndex, _int_in

MAX_INS = 8
MAX_DEN = 1 << 15
SCAN_TILE = TILE                              # positions per tile of the call and emit kernels
COL_A, COL_G, COL_C, COL_T, COL_DELETION, COL_OTHER = range(6)
LOW_DEPTH, AMBIGUOUS, SUBSTITUTION, DELETION, INSERTION = 1, 2, 4, 8, 16


class Pileup(namedtuple("Pileup", "counts ins_lengths ins_bases used")):
    """counts [R, 2, 6] int32: [forward position][strand of the read][A, G, C, T, deletion, other]; ins_lengths [R, max_ins + 1]
    int32: insertions between p and p + 1 by length (column l - 1: length l; the last column: longer ones), both strands together;
    ins_bases [R, max_ins, 4] int32: the k-th inserted base in forward orientation; used [B] int8 of the last batch: 1 added, 0
    skipped, -1 bad.  All on the device.  A position holds fewer than 2^31 reads."""
    __slots__ = ()

    @property
    def R(self):
        return int(self.counts.shape[0])

    @property
    def max_ins(self):
        return int(self.ins_lengths.shape[1]) - 1

    @property
    def depth(self):
        """[R] int64: the reads that show a base or a deletion at the position (`other` left out)"""
        return self.counts[:, :, :5].sum((1, 2))


ConsensusCalls = namedtuple("ConsensusCalls", "call ins_len ins_bases flags alt_count offsets consensus")
ConsensusCalls.__doc__ = """call [R] uint8: 0 deleted, else the called label (the reference's own label where it is kept); ins_len [R]
uint8 and ins_bases [R, max_ins] uint8: the insertion called after the position; flags [R] uint8: LOW_DEPTH 1, AMBIGUOUS 2,
SUBSTITUTION 4, DELETION 8, INSERTION 16; alt_count [R, 2] int32: the called candidate's count per strand; offsets [R + 1] int32:
where position p lands in the consensus; consensus [offsets[R]] int32: the label row.  All on the device.  The flag values are
class attributes too (ConsensusCalls.DELETION): the package exports the function `pileup` under this module's name."""
ConsensusCalls.LOW_DEPTH, ConsensusCalls.AMBIGUOUS, ConsensusCalls.SUBSTITUTION = LOW_DEPTH, AMBIGUOUS, SUBSTITUTION
ConsensusCalls.DELETION, ConsensusCalls.INSERTION = DELETION, INSERTION

Variant = namedtuple("Variant", "pos kind ref alt depth alt_count forward reverse")
Variant.__doc__ = """pos: the 0-based position of the first label of `ref`; kind "sub", "del" or "ins"; ref, alt: label tuples as VCF
writes them (an indel with its anchor base); depth, alt_count: DP and AC; forward, reverse: the alt count per strand (None for an
insertion: those are not split by strand)."""


def _read_args(what, alignment, lo, ref_lengths, strand, query, query_lengths, R, qual, min_qual, keep):
    """the checks and preparations of the reads of a batch that pileup and pileup_evidence (genotype.py) share: the two walk the same
    columns of the same reads, so they refuse the same inputs in the same words -> (R, min_qual, ops, ops_len, lo, ref_lengths,
    strand, query, query_lengths, qual, keep) as the C ABI takes them"""
    R = _int_in(what, "R", R, 1, MAX_REFERENCE)
    min_qual = _int_in(what, "min_qual", min_qual, 0, MAX_QUAL)
    ops, ops_len = _alignment_ops(alignment, what)
    width = int(query.shape[1]) if isinstance(query, torch.Tensor) and query.dim() == 2 else 0
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, M = int(query.shape[0]), int(query.shape[1])
    dev = query.device
    if B < 1 or B > 65535 or M > MAX_PAIR_QUERY:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 reads of at most %d labels, got %d of %d" % (what, MAX_PAIR_QUERY, B, M))
    ops, ops_len, _ = _op_rows(ops, ops_len, B, dev, what, on="query")
    lo, ref_lengths, strand = (_args.lengths(x, B, dev, what, name) for x, name in ((lo, "lo"), (ref_lengths, "ref_lengths"), (strand, "strand")))
    qual = _profile_rows(qual, B, width, torch.uint8, what, "qual")
    if qual is not None and qual.device != dev:
        raise ValueError("wavenet_speech_amd.%s: qual must be on the device of the query" % what)
    if keep is not None:
        keep = torch.as_tensor(keep)
        if keep.dtype != torch.bool or keep.shape != (B,):
            raise ValueError("wavenet_speech_amd.%s: keep must be bool of shape (%d,), got %s %s" % (what, B, keep.dtype, tuple(keep.shape)))
        keep = keep.to(device=dev, dtype=torch.uint8).contiguous()
    return R, min_qual, ops, ops_len, lo, ref_lengths, strand, query, query_lengths, qual, keep


def _note_bad_reads(bad, what, R):
    """the report of the reads pileup and pileup_evidence refuse on the device: one text, the same reads"""
    _args.note_bad(bad, lambda n: "wavenet_speech_amd.%s: %d pair(s) whose ops do not fit: an op outside 1..4, a length out of range, "
                   "labels not consumed exactly, a strand above 1, a window outside [0, %d] or a qual above %d" % (what, n, R, MAX_QUAL))


def pileup(alignment, lo, ref_lengths, strand, query, query_lengths, R, qual=None, min_qual=0, max_ins=4, keep=None, into=None):
    """Adds every read of a batch into the tables over the reference, one launch.
    alignment: a PairwiseAlignment with ops of the read against its window IN READ ORIENTATION, exactly as
    pairwise_align(*mapping.labels(flank), query, query_lengths) returns it; lo, ref_lengths, strand [B]: mapping.window(flank) and
    mapping.strand; query [B, M] int32 or int64 GPU rows (M <= 8192) with query_lengths [B]; R: the reference's length, 1 to 2^26;
    qual [B, >= M] uint8: BaseQualities.qual; min_qual in [0, 93]: a base below it counts as `other` (only with qual); max_ins in
    [0, 8]; keep [B] bool: reads to add (mapping.mapq() >= 20, ...); into: an earlier Pileup of the same R and max_ins whose tables
    are accumulated in place (and returned; `used` is replaced).
    Ops 1 and 2 are alike an aligned pair (reference labels are not needed).  End columns -- everything before the first and after
    the last aligned column -- enter nothing.  A reverse-strand read is counted as it reads on the forward strand: complemented,
    insertions in forward order.  Adds are 32-bit: a position holds fewer than 2^31 reads.
    Returns Pileup.  used is 0 for a read with strand < 0, ref_lengths == 0, keep false or no aligned column.  A pair whose ops do not
    fit (an op outside 1..4, ops_len outside its row, labels not consumed exactly, strand > 1, a window outside [0, R], a qual above
    93; a poisoned pair of pairwise_align) has used -1, adds nothing and is reported through check_device_flags()."""
    what = "pileup"
    max_ins = _int_in(what, "max_ins", max_ins, 0, MAX_INS)
    R, min_qual, ops, ops_len, lo, ref_lengths, strand, query, query_lengths, qual, keep = _read_args(
        what, alignment, lo, ref_lengths, strand, query, query_lengths, R, qual, min_qual, keep)
    B, M, max_ops, dev = int(query.shape[0]), int(query.shape[1]), int(ops.shape[1]), query.device
    if into is not None and not isinstance(into, Pileup):
        raise ValueError("wavenet_speech_amd.%s: into must be a Pileup, got %s" % (what, type(into).__name__))
    lib = _lib.load()
    with torch.cuda.device(dev):
        counts = _args.into_table(into, "counts", (R, 2, 6), dev, what, torch.int32)
        ins_lengths = _args.into_table(into, "ins_lengths", (R, max_ins + 1), dev, what, torch.int32)
        ins_bases = _args.into_table(into, "ins_bases", (R, max_ins, 4), dev, what, torch.int32)
        used = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_pileup(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_lengths), _p(strand), _p(query), query.stride(0),
                                 _p(query_lengths), _p(qual), qual.stride(0) if qual is not None else 0, _p(keep), B, M, max_ops, R,
                                 min_qual, max_ins, _p(counts), _p(ins_lengths), _p(ins_bases) if max_ins else None, _p(used), _p(bad),
                                 _stream()), "wn_pileup")
        _note_bad_reads(bad, what, R)
    return Pileup(counts, ins_lengths, ins_bases, used)


def _reference_labels(reference, R, device, what):
    """[R] int32 labels on `device` from a ReadIndex or a 1-d integer tensor / list"""
    bases = reference.bases if isinstance(reference, ReadIndex) else torch.as_tensor(reference)
    if bases.is_floating_point() or bases.dtype == torch.bool or tuple(bases.shape) != (R,):
        raise ValueError("wavenet_speech_amd.%s: reference must be a ReadIndex or integer labels of shape (%d,), got %s %s"
                         % (what, R, bases.dtype, tuple(bases.shape)))
    return bases.detach().to(device=device, dtype=torch.int32).contiguous()


def call_consensus(pileup, reference, min_depth=3, min_fraction=(1, 2)):
    """A consensus label, an insertion and flags per position of a Pileup, and the consensus row.
    reference: a ReadIndex or [R] labels; min_depth >= 1; min_fraction = (num, den), 0 <= num <= den <= 2^15.  With d = depth[p]:
    below min_depth the reference base is kept (LOW_DEPTH).  Otherwise the candidate among A, G, C, T, deletion with the greatest
    count over both strands -- ties first to the reference base, then to the smaller label, deletion last -- is called if
    count * den > num * d; else the reference base is kept (AMBIGUOUS).  SUBSTITUTION / DELETION where the call is not the reference
    base.  An insertion after p is called when d >= min_depth and n * den > num * d, n = sum(ins_lengths[p]); its length is the
    fullest column of ins_lengths[p] (ties to the shorter; the last column counts as max_ins), each base the fullest of its slot
    (ties to the smaller label), and the first slot without any count ends it (INSERTION if anything is left).
    Three launches (the calls with a total per tile, a scan of the totals, the emit) and ONE host synchronisation between the last
    two, to size `consensus`.  Returns ConsensusCalls."""
    what = "call_consensus"
    if not isinstance(pileup, Pileup):
        raise ValueError("wavenet_speech_amd.%s: pileup must be a Pileup, got %s" % (what, type(pileup).__name__))
    min_depth = _int_in(what, "min_depth", min_depth, 1, 2 ** 31 - 1)
    if not isinstance(min_fraction, (tuple, list)) or len(min_fraction) != 2:
        raise ValueError("wavenet_speech_amd.%s: min_fraction must be a pair of integers (num, den), got %r" % (what, min_fraction))
    den = _int_in(what, "min_fraction[1]", min_fraction[1], 1, MAX_DEN)
    num = _int_in(what, "min_fraction[0]", min_fraction[0], 0, den)
    counts = _args.gpu_tensor(pileup.counts, what, "pileup.counts", (torch.int32,))
    dev = counts.device
    R, max_ins = pileup.R, pileup.max_ins
    for t, name, shape in ((counts, "counts", (R, 2, 6)), (pileup.ins_lengths, "ins_lengths", (R, max_ins + 1)),
                           (pileup.ins_bases, "ins_bases", (R, max_ins, 4))):
        _args.gpu_tensor(t, what, "pileup." + name, (torch.int32,), device=dev)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("wavenet_speech_amd.%s: pileup.%s must be contiguous of shape %s" % (what, name, shape))
    if not 1 <= R <= MAX_REFERENCE or not 0 <= max_ins <= MAX_INS:
        raise ValueError("wavenet_speech_amd.%s: a pileup of %d positions with max_ins %d" % (what, R, max_ins))
    reference = _reference_labels(reference, R, dev, what)
    lib = _lib.load()
    with torch.cuda.device(dev):
        call, ins_len, flags = (torch.empty(R, dtype=torch.uint8, device=dev) for _ in range(3))
        ins_out = torch.empty(R, max_ins, dtype=torch.uint8, device=dev)
        alt_count = torch.empty(R, 2, dtype=torch.int32, device=dev)
        offsets = torch.empty(R + 1, dtype=torch.int32, device=dev)
        tile_offsets = torch.empty((R + SCAN_TILE - 1) // SCAN_TILE, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_consensus_call(_p(counts), _p(pileup.ins_lengths), _p(pileup.ins_bases) if max_ins else None, _p(reference), R,
                                         max_ins, min_depth, num, den, _p(call), _p(ins_len), _p(ins_out) if max_ins else None, _p(flags),
                                         _p(alt_count), _p(tile_offsets), _p(offsets.data_ptr() + 4 * R), _stream()), "wn_consensus_call")
        total = int(offsets[R])                                      # the one host synchronisation: the consensus is sized here
        consensus = torch.empty(total, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_consensus_emit(_p(call), _p(ins_len), _p(ins_out) if max_ins else None, _p(tile_offsets), R, max_ins, total,
                                         _p(offsets), _p(consensus) if total else None, _stream()), "wn_consensus_emit")
    return ConsensusCalls(call, ins_len, ins_out, flags, alt_count, offsets, consensus)


def variant_records(reference, calls, pileup):
    """host helper: the Variant list of a ConsensusCalls, sorted by position.  The flagged positions are found with torch ops on
    the tensors' device and only their rows are copied.  Each substitution is one record; a run of consecutive deleted positions
    is one record anchored on the preceding base (a run that starts at position 0: on the following base, as VCF 4.2 has it; a
    reference deleted whole has no anchor and an empty alt), with the depth and counts of its first position; an insertion after p
    is anchored on ref[p], with alt_count = sum(ins_lengths[p])."""
    what = "variant_records"
    if not isinstance(calls, ConsensusCalls) or not isinstance(pileup, Pileup):
        raise ValueError("wavenet_speech_amd.%s: calls must be ConsensusCalls and pileup a Pileup" % what)
    flags = calls.flags
    R = int(flags.shape[0])
    if pileup.R != R:
        raise ValueError("wavenet_speech_amd.%s: calls of %d positions beside a pileup of %d" % (what, R, pileup.R))
    ref = _reference_labels(reference, R, flags.device, what).long()
    idx = torch.nonzero(flags & (SUBSTITUTION | DELETION | INSERTION)).reshape(-1)
    if idx.numel() == 0:
        return []
    counts = pileup.counts[idx].long()
    cols = [idx, flags[idx].long(), ref[idx], ref[(idx - 1).clamp(min=0)], ref[(idx + 1).clamp(max=R - 1)], calls.call[idx].long(),
            calls.ins_len[idx].long(), counts[:, :, :5].sum((1, 2)), calls.alt_count[idx, 0].long(), calls.alt_count[idx, 1].long(),
            pileup.ins_lengths[idx].long().sum(1)]
    rows = torch.stack(cols, 1).cpu().tolist()
    inserted = calls.ins_bases[idx].cpu().tolist()
    out, q = [], 0
    while q < len(rows):
        p, f, r, before, _, label, n_ins, depth, fwd, rev, n = rows[q]
        if f & SUBSTITUTION:
            out.append(Variant(p, "sub", (r,), (label,), depth, fwd + rev, fwd, rev))
        if f & DELETION and not (q > 0 and rows[q - 1][0] == p - 1 and rows[q - 1][1] & DELETION):       # a run starts here
            e = q
            while e + 1 < len(rows) and rows[e + 1][0] == rows[e][0] + 1 and rows[e + 1][1] & DELETION:
                e += 1
            gone = tuple(rows[t][2] for t in range(q, e + 1))
            if p > 0:
                v = Variant(p - 1, "del", (before,) + gone, (before,), depth, fwd + rev, fwd, rev)
            elif rows[e][0] + 1 < R:
                v = Variant(0, "del", gone + (rows[e][4],), (rows[e][4],), depth, fwd + rev, fwd, rev)
            else:
                v = Variant(0, "del", gone, (), depth, fwd + rev, fwd, rev)
            out.append(v)
        if f & INSERTION:
            out.append(Variant(p, "ins", (r,), (r,) + tuple(inserted[q][:n_ins]), depth, n, None, None))
        q += 1
    out.sort(key=lambda v: (v.pos, ("sub", "del", "ins").index(v.kind)))
    return out


def vcf_records(ref_name, reference, calls, pileup, alphabet=DEFAULT_ALPHABET):
    """host helper: one VCF 4.2 data line per variant_records() entry, "\\n"-terminated, sorted by position: CHROM, POS (1-based), ID
    ".", REF, ALT, QUAL ".", FILTER "PASS", INFO DP=<depth>;AC=<alt count>;SF=<forward>,<reverse> (SF=.,. for an insertion: those
    are not split by strand).  A label outside 1..len(alphabet) - 1 prints as N; the empty alt of a reference deleted whole as
    <DEL>."""
    char = lambda v: alphabet[v] if 0 < v < len(alphabet) else "N"   # noqa: E731
    out = []
    for v in variant_records(reference, calls, pileup):
        sf = ".,." if v.forward is None else "%d,%d" % (v.forward, v.reverse)
        out.append("%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AC=%d;SF=%s\n" % (ref_name, v.pos + 1, "".join(char(x) for x in v.ref),
                                                                     "".join(char(x) for x in v.alt) or "<DEL>", v.depth, v.alt_count, sf))
    return out
