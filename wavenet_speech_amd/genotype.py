"""
Genotype likelihoods and diploid variant calls with QUAL on the device (csrc/wn_genotype.hip through
wn_pileup_evidence and wn_genotype_call): the step bcftools call, GATK and medaka's variant stage run after the pileup.  Every base
is weighed by its (calibrated) quality, and every position gets a genotype of two alleles with its quality, so a heterozygous site
of a diploid sample is called as one instead of coming back AMBIGUOUS.

    w = genotype_weights()
    pile = pileup(aln, lo, ref_lengths, m.strand, labels, lengths, index.R, qual=q.qual, min_qual=7, keep=keep)
    ev = pileup_evidence(aln, lo, ref_lengths, m.strand, labels, lengths, index.R, w, qual=q.qual, min_qual=7, keep=keep,
                         cap=m.mapq().clamp(max=93).to(torch.uint8))
    g = call_genotypes(pile, ev, index, w)
    print("".join(vcf_genotype_records("chr", index, g, pile, w)))

The Pileup and the Evidence must have been fed THE SAME BATCHES with the same min_qual and keep: the depth and the insertions come
from the one, the weights from the other, and nothing can check that they belong together.

Everything the kernels add or compare is an integer, so results equal the host reference of tests/genotype_ref.py exactly and two
runs are bitwise identical.  Neither function synchronises with the host.  There is no CPU fallback: CPU tensors raise (the host
helpers genotype_records / vcf_genotype_records take tensors on any device).
Read-backed phasing of the heterozygous calls and a haplotype tag per read are phase.py's.
Realignment of the reads against the called haplotypes is realign.py's.
Not built: more than one insertion allele per site, strand bias, a gap_qual derived from quality_profile.
"""
import ctypes
import math
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import DEFAULT_ALPHABET, MAX_QUAL
from .pileup import DELETION, INSERTION, LOW_DEPTH, MAX_INS, SUBSTITUTION, Pileup, _note_bad_reads, _read_args, _reference_labels
from .readmap import MAX_REFERENCE, _int_in

HOM, HET, MIS = range(3)
QUAL_COLUMNS = MAX_QUAL + 1
MAX_WEIGHT = 1 << 20
MAX_ALT_PRIOR = 1 << 30
GT_HET, INS_HET = 32, 64
GENOTYPES = tuple((a, b) for a in range(5) for b in range(a, 5))     # the 15 unordered pairs, in the order of `costs`


class GenotypeWeights(namedtuple("GenotypeWeights", "table scale")):
    """table [3, 94] int32 on the HOST: rows HOM, HET, MIS, columns qual 0..93, in units of 1 / scale Phred, every entry in
    [0, 2^20]; scale: a positive integer.  Any table in range is taken: the model lives in genotype_weights, not on the device."""
    __slots__ = ()

    def checked(self, what):
        """the table as the C ABI takes it: a ctypes array of 3 * 94 ints"""
        t = self.table
        if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (3, QUAL_COLUMNS):
            raise ValueError("wavenet_speech_amd.%s: weights.table must be a host int32 tensor of shape (3, %d)" % (what, QUAL_COLUMNS))
        if isinstance(self.scale, bool) or not isinstance(self.scale, int) or self.scale < 1:
            raise ValueError("wavenet_speech_amd.%s: weights.scale must be a positive integer, got %r" % (what, self.scale))
        flat = t.reshape(-1).tolist()
        if min(flat) < 0 or max(flat) > MAX_WEIGHT:
            raise ValueError("wavenet_speech_amd.%s: every weight must lie in [0, %d], got %d to %d" % (what, MAX_WEIGHT, min(flat), max(flat)))
        return (ctypes.c_int * len(flat))(*flat)


def genotype_weights(scale=100):
    """host helper: the weight table of the diploid model, built in float64.  With e = min(10^(-q / 10), 3 / 4) the chance that a
    base of quality q is wrong (3 / 4: a base that says nothing), a base that shows allele x costs, in Phred,
    HOM = -10 log10(1 - e) under a genotype x/x, HET = -10 log10((1 - e) / 2 + e / 6) under x/y, MIS = -10 log10(e / 3) under a
    genotype without x.  Each value times `scale` (1 to 10699 = 2^20 // 98: MIS of qual 93 is 97.77 and must stay within 2^20),
    through round().  At e = 3 / 4 the three are equal: a base of qual 0 or 1 carries no information.  Returns GenotypeWeights."""
    scale = _int_in("genotype_weights", "scale", scale, 1, MAX_WEIGHT // 98)
    rows = [[], [], []]
    for q in range(QUAL_COLUMNS):
        e = min(10.0 ** (-q / 10.0), 0.75)
        for row, v in zip(rows, (1.0 - e, (1.0 - e) / 2.0 + e / 6.0, e / 3.0)):
            row.append(int(round(-10.0 * math.log10(v) * scale)))
    w = GenotypeWeights(torch.tensor(rows, dtype=torch.int32), scale)
    w.checked("genotype_weights")
    return w


Evidence = namedtuple("Evidence", "evidence used")
Evidence.__doc__ = """evidence [R, 5, 3] int64: [forward position][A, G, C, T, deletion][HOM, HET, MIS], the sums of the weights of
the bases that show the allele; used [B] int8 of the last batch, as Pileup.used.  On the device."""

Genotypes = namedtuple("Genotypes", "alleles gq qual flags ins_copies ins_len ins_bases ins_gq ins_qual costs")
Genotypes.__doc__ = """alleles [R, 2] uint8: the two called labels in allele order A, G, C, T, deleted (0 means deleted, as in
ConsensusCalls.call); gq [R] int32: the second-least cost minus the least, in 1 / scale Phred; qual [R] int32: the cost of
reference/reference minus the least; flags [R] uint8: LOW_DEPTH 1, SUBSTITUTION 4, DELETION 8, INSERTION 16, HET 32, INS_HET 64;
ins_copies [R] uint8: 0, 1 or 2 copies of the insertion after the position, with ins_len [R] uint8, ins_bases [R, max_ins] uint8,
ins_gq and ins_qual [R] int32; costs [R, 15] int64 in the order of GENOTYPES, or None.  All on the device.  The flag values are
class attributes too (Genotypes.HET)."""
Genotypes.LOW_DEPTH, Genotypes.SUBSTITUTION, Genotypes.DELETION, Genotypes.INSERTION = LOW_DEPTH, SUBSTITUTION, DELETION, INSERTION
Genotypes.HET, Genotypes.INS_HET = GT_HET, INS_HET

GenotypeRecord = namedtuple("GenotypeRecord", "pos kind ref alts gt qual gq depth")
GenotypeRecord.__doc__ = """pos: the 0-based position of the first label of `ref`; kind "sub", "del" or "ins"; ref: a label tuple;
alts: a tuple of label tuples as VCF writes them (an indel with its anchor base), () standing for the `*` allele: deleted here, by
the record that spans it; gt: "0/1", "1/1" or "1/2"; qual, gq: in 1 / scale Phred; depth: DP."""


def pileup_evidence(alignment, lo, ref_lengths, strand, query, query_lengths, R, weights, qual=None, flat_qual=20, gap_qual=20, cap=None,
                    min_qual=0, keep=None, into=None):
    """Adds the quality-weighted evidence of every read of a batch into a table over the reference, one
    launch.  The reads, and alignment, lo, ref_lengths, strand, query, query_lengths, R, qual, min_qual and keep, are pileup's, with
    pileup's refusals; both walk the same columns.  weights: a GenotypeWeights; flat_qual in [0, 93]: the quality of every base when
    no qual is given; gap_qual in [0, 93]: the quality of a deletion column; cap [B] uint8 on the device: a ceiling on every quality
    of read b (samtools' mapq cap: mapping.mapq().clamp(max=93).to(torch.uint8)); into: an earlier Evidence of the same R whose table
    is accumulated in place (and returned; `used` is replaced).
    A column that pileup counts under base k adds weights[:, min(q, cap[b])] to evidence[p, k]; a deletion column adds
    weights[:, min(gap_qual, cap[b])] to evidence[p, 4].  min_qual is compared with the uncapped qual, as in pileup: the same columns
    go to `other` in both, and those add nothing here, as insertion columns do.  Adds are 64-bit.
    The defaults 20 and 20 are conventions (a base and a gap wrong once in a hundred), not measurements.
    Returns Evidence.  Skipped and bad reads are pileup's and are reported through check_device_flags() likewise."""
    what = "pileup_evidence"
    if not isinstance(weights, GenotypeWeights):
        raise ValueError("wavenet_speech_amd.%s: weights must be a GenotypeWeights, got %s" % (what, type(weights).__name__))
    table = weights.checked(what)
    flat_qual = _int_in(what, "flat_qual", flat_qual, 0, MAX_QUAL)
    gap_qual = _int_in(what, "gap_qual", gap_qual, 0, MAX_QUAL)
    R, min_qual, ops, ops_len, lo, ref_lengths, strand, query, query_lengths, qual, keep = _read_args(
        what, alignment, lo, ref_lengths, strand, query, query_lengths, R, qual, min_qual, keep)
    B, M, max_ops, dev = int(query.shape[0]), int(query.shape[1]), int(ops.shape[1]), query.device
    if cap is not None:
        cap = _args.gpu_tensor(cap, what, "cap", (torch.uint8,), device=dev)
        if tuple(cap.shape) != (B,):
            raise ValueError("wavenet_speech_amd.%s: cap must be uint8 of shape (%d,), got %s" % (what, B, tuple(cap.shape)))
        cap = cap.contiguous()
    if into is not None and not isinstance(into, Evidence):
        raise ValueError("wavenet_speech_amd.%s: into must be an Evidence, got %s" % (what, type(into).__name__))
    lib = _lib.load()
    with torch.cuda.device(dev):
        evidence = _args.into_table(into, "evidence", (R, 5, 3), dev, what, torch.int64)
        used = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_pileup_evidence(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_lengths), _p(strand), _p(query),
                                          query.stride(0), _p(query_lengths), _p(qual), qual.stride(0) if qual is not None else 0, _p(keep),
                                          B, M, max_ops, R, _p(cap), ctypes.cast(table, ctypes.c_void_p), flat_qual, gap_qual, min_qual,
                                          _p(evidence), _p(used), _p(bad), _stream()), "wn_pileup_evidence")
        _note_bad_reads(bad, what, R)
    return Evidence(evidence, used)


def call_genotypes(pileup, evidence, reference, weights, gap_qual=20, alt_prior=None, min_depth=3, return_costs=False):
    """A diploid genotype with its qualities, and an insertion genotype, per position, one launch and no host
    synchronisation.  pileup: the Pileup and evidence: the Evidence OF THE SAME BATCHES, fed with the same min_qual and keep (nothing
    can check that); reference: a ReadIndex or [R] labels; weights: the GenotypeWeights the evidence was added with; gap_qual in
    [0, 93]: the quality of an insertion's presence or absence in a read; alt_prior in [0, 2^30]: the cost, in 1 / scale Phred, of
    any genotype but reference/reference -- None: 30 * scale, a heterozygosity of 10^-3; min_depth >= 1.
    With E = evidence[p] and the 15 pairs a <= b of A, G, C, T, deletion in lexicographic order (GENOTYPES):
    L(a, a) = E[a, HOM] + sum of E[x, MIS] over x != a, L(a, b) = E[a, HET] + E[b, HET] + sum of E[x, MIS] over the other x, and
    cost = L + alt_prior for all but reference/reference.  The call is the least by (cost, is not reference/reference, index).
    SUBSTITUTION: a called allele is a base other than the reference's; DELETION: one is the deletion; HET: the two differ.  Below
    min_depth (the depth of call_consensus): the reference base twice, gq = qual = 0, LOW_DEPTH.  A reference label outside 1..4: the
    label twice, gq = qual = 0, no flag.
    The insertion after p is present in n = sum(ins_lengths[p]) of the d reads and absent from m = max(d - n, 0); with the weights of
    gap_qual, 0 copies cost n MIS + m HOM, 1 copy (n + m) HET + alt_prior, 2 copies n HOM + m MIS + alt_prior; ties go to fewer
    copies.  Its length and bases are call_consensus' without the fraction test; an empty sequence calls nothing.  INSERTION with at
    least one copy, INS_HET with exactly one.
    The defaults 20 and 30 are conventions, not measurements.  Returns Genotypes (costs only with return_costs)."""
    what = "call_genotypes"
    if not isinstance(pileup, Pileup) or not isinstance(evidence, Evidence):
        raise ValueError("wavenet_speech_amd.%s: pileup must be a Pileup and evidence an Evidence, got %s and %s"
                         % (what, type(pileup).__name__, type(evidence).__name__))
    if not isinstance(weights, GenotypeWeights):
        raise ValueError("wavenet_speech_amd.%s: weights must be a GenotypeWeights, got %s" % (what, type(weights).__name__))
    table = weights.checked(what)
    gap_qual = _int_in(what, "gap_qual", gap_qual, 0, MAX_QUAL)
    min_depth = _int_in(what, "min_depth", min_depth, 1, 2 ** 31 - 1)
    alt_prior = _int_in(what, "alt_prior", 30 * weights.scale if alt_prior is None else alt_prior, 0, MAX_ALT_PRIOR)
    counts = _args.gpu_tensor(pileup.counts, what, "pileup.counts", (torch.int32,))
    dev = counts.device
    R, max_ins = pileup.R, pileup.max_ins
    for t, name, shape, dtype in ((counts, "pileup.counts", (R, 2, 6), torch.int32), (pileup.ins_lengths, "pileup.ins_lengths", (R, max_ins + 1), torch.int32),
                                  (pileup.ins_bases, "pileup.ins_bases", (R, max_ins, 4), torch.int32),
                                  (evidence.evidence, "evidence.evidence", (R, 5, 3), torch.int64)):
        _args.gpu_tensor(t, what, name, (dtype,), device=dev)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("wavenet_speech_amd.%s: %s must be contiguous of shape %s" % (what, name, shape))
    if not 1 <= R <= MAX_REFERENCE or not 0 <= max_ins <= MAX_INS:
        raise ValueError("wavenet_speech_amd.%s: a pileup of %d positions with max_ins %d" % (what, R, max_ins))
    reference = _reference_labels(reference, R, dev, what)
    lib = _lib.load()
    with torch.cuda.device(dev):
        alleles = torch.empty(R, 2, dtype=torch.uint8, device=dev)
        flags, ins_copies, ins_len = (torch.empty(R, dtype=torch.uint8, device=dev) for _ in range(3))
        gq, qual, ins_gq, ins_qual = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(4))
        ins_out = torch.empty(R, max_ins, dtype=torch.uint8, device=dev)
        costs = torch.empty(R, 15, dtype=torch.int64, device=dev) if return_costs else None
        _lib.check(lib.wn_genotype_call(_p(evidence.evidence), _p(counts), _p(pileup.ins_lengths), _p(pileup.ins_bases) if max_ins else None,
                                        _p(reference), R, max_ins, min_depth, alt_prior, ctypes.cast(table, ctypes.c_void_p), gap_qual,
                                        _p(alleles), _p(gq), _p(qual), _p(flags), _p(ins_copies), _p(ins_len), _p(ins_out) if max_ins else None,
                                        _p(ins_gq), _p(ins_qual), _p(costs), _stream()), "wn_genotype_call")
    return Genotypes(alleles, gq, qual, flags, ins_copies, ins_len, ins_out, ins_gq, ins_qual, costs)


def genotype_records(reference, genotypes, pileup):
    """host helper: the GenotypeRecord list of a Genotypes, sorted by position.  The flagged positions are found with torch ops on the
    tensors' device and only their rows are copied.  A substitution is one record whose alts are the called bases other than the
    reference's, in allele order: gt 0/1 beside the reference base, 1/1 twice the same, 1/2 two bases, or a base beside the
    deletion, which is listed second as the `*` allele ().  A run of consecutive DELETION positions OF THE SAME ZYGOSITY (both
    alleles deleted, or one) is one record -- a change of zygosity starts another -- anchored as variant_records anchors it, gt 1/1
    or 0/1, with the qual, gq and depth of its first position; a position whose other allele is a substituted base is heterozygous
    in the deletion record too.  An insertion after p is anchored on ref[p]: gt 0/1 or 1/1, qual and gq the insertion's."""
    return [v for v, _ in _records_with_sites("genotype_records", reference, genotypes, pileup)]


def _records_with_sites(what, reference, genotypes, pileup):
    """genotype_records' list as pairs (record, the position whose call it reports: a substitution's own, the first deleted one of a
    deletion, an insertion's anchor); phased_records (phase.py) looks the phase up there"""
    if not isinstance(genotypes, Genotypes) or not isinstance(pileup, Pileup):
        raise ValueError("wavenet_speech_amd.%s: genotypes must be Genotypes and pileup a Pileup" % what)
    flags = genotypes.flags
    R = int(flags.shape[0])
    if pileup.R != R:
        raise ValueError("wavenet_speech_amd.%s: genotypes of %d positions beside a pileup of %d" % (what, R, pileup.R))
    ref = _reference_labels(reference, R, flags.device, what).long()
    idx = torch.nonzero(flags & (SUBSTITUTION | DELETION | INSERTION)).reshape(-1)
    if idx.numel() == 0:
        return []
    cols = [idx, flags[idx].long(), ref[idx], ref[(idx - 1).clamp(min=0)], ref[(idx + 1).clamp(max=R - 1)], genotypes.alleles[idx, 0].long(),
            genotypes.alleles[idx, 1].long(), genotypes.qual[idx].long(), genotypes.gq[idx].long(), pileup.counts[idx].long()[:, :, :5].sum((1, 2)),
            genotypes.ins_copies[idx].long(), genotypes.ins_len[idx].long(), genotypes.ins_qual[idx].long(), genotypes.ins_gq[idx].long()]
    rows = torch.stack(cols, 1).cpu().tolist()
    inserted = genotypes.ins_bases[idx].cpu().tolist()
    starts = lambda q: not (q > 0 and rows[q - 1][0] == rows[q][0] - 1 and rows[q - 1][1] & DELETION and       # noqa: E731
                            (rows[q - 1][5] == 0) == (rows[q][5] == 0))
    out, q = [], 0
    while q < len(rows):
        p, f, r, before, _, a0, a1, qual, gq, depth, copies, n_ins, ins_qual, ins_gq = rows[q]
        if f & SUBSTITUTION:
            bases = [v for v in (a0, a1) if v not in (0, r)]
            alts = tuple((v,) for v in sorted(set(bases), key=bases.index))
            if f & DELETION:
                alts, gt = alts + ((),), "1/2"
            else:
                gt = "1/2" if len(alts) == 2 else "1/1" if len(bases) == 2 else "0/1"
            out.append((GenotypeRecord(p, "sub", (r,), alts, gt, qual, gq, depth), p))
        if f & DELETION and starts(q):                               # a run starts here; alleles (0, 0) are the homozygous ones
            e = q
            while e + 1 < len(rows) and rows[e + 1][1] & DELETION and not starts(e + 1):
                e += 1
            gone = tuple(rows[t][2] for t in range(q, e + 1))
            gt = "1/1" if a0 == 0 else "0/1"
            if p > 0:
                out.append((GenotypeRecord(p - 1, "del", (before,) + gone, ((before,),), gt, qual, gq, depth), p))
            elif rows[e][0] + 1 < R:
                out.append((GenotypeRecord(0, "del", gone + (rows[e][4],), ((rows[e][4],),), gt, qual, gq, depth), p))
            else:
                out.append((GenotypeRecord(0, "del", gone, ((),), gt, qual, gq, depth), p))
        if f & INSERTION:
            out.append((GenotypeRecord(p, "ins", (r,), ((r,) + tuple(inserted[q][:n_ins]),), "1/1" if copies == 2 else "0/1", ins_qual, ins_gq,
                                       depth), p))
        q += 1
    out.sort(key=lambda v: (v[0].pos, ("sub", "del", "ins").index(v[0].kind)))
    return out


def vcf_genotype_records(ref_name, reference, genotypes, pileup, weights, alphabet=DEFAULT_ALPHABET):
    """host helper: one VCF 4.2 data line per genotype_records() entry, "\\n"-terminated, sorted by position: CHROM, POS (1-based), ID
    ".", REF, ALT (comma-separated; `*` for an allele deleted here by another record, <DEL> for the empty alt of a reference deleted
    whole), QUAL = qual // scale, FILTER "PASS", INFO DP=<depth>, FORMAT GT:GQ and the sample <gt>:<min(99, gq // scale)>.  A label
    outside 1..len(alphabet) - 1 prints as N."""
    if not isinstance(weights, GenotypeWeights):
        raise ValueError("wavenet_speech_amd.vcf_genotype_records: weights must be a GenotypeWeights, got %s" % type(weights).__name__)
    weights.checked("vcf_genotype_records")
    char = lambda v: alphabet[v] if 0 < v < len(alphabet) else "N"   # noqa: E731
    out = []
    for v in genotype_records(reference, genotypes, pileup):
        alts = ",".join("".join(char(x) for x in alt) or ("<DEL>" if v.kind == "del" else "*") for alt in v.alts)
        out.append("%s\t%d\t.\t%s\t%s\t%d\tPASS\tDP=%d\tGT:GQ\t%s:%d\n" % (ref_name, v.pos + 1, "".join(char(x) for x in v.ref), alts,
                                                                          v.qual // weights.scale, v.depth, v.gt, min(99, v.gq // weights.scale)))
    return out
