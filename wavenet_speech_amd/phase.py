"""
Read-backed phasing of diploid calls and haplotags on the device (csrc/wn_phase.hip through wn_phase_links,
wn_phase_chain and wn_haplotag): the step WhatsHap, longshot, margin or HapCUT2 run after the calls.  The reads that were piled up
each span several heterozygous sites, so they say which alleles of neighbouring sites lie on the same haplotype.

    g = call_genotypes(pile, ev, index, w)
    sites = phase_sites(g)                                             # the heterozygous positions; reads S back
    reads = (aln, lo, ref_lengths, m.strand, labels, lengths)          # exactly what pileup and pileup_evidence were given
    links = phase_links(*reads, sites, qual=q.qual, min_qual=7, keep=keep, cap=cap)
    links = phase_links(*reads2, sites, ..., into=links)               # over batches
    phasing = phase_chain(links, sites)
    tags = haplotag(*reads, sites, phasing, qual=q.qual, min_qual=7, keep=keep, cap=cap)   # hp 1 / 2 / 0 and ps per read
    print("".join(vcf_phased_records("chr", index, g, pile, sites, phasing, w)))          # 0|1 ... GT:GQ:PS

Everything the kernels add or compare is an integer, so results equal the host reference of tests/phase_ref.py exactly and two
runs are bitwise identical.  phase_sites synchronises with the host once (the number of sites sizes every later table); nothing
else does.  There is no CPU fallback: CPU tensors raise (the host helpers phased_records / vcf_phased_records take tensors on any
device).
Not built: phasing of heterozygous insertions, a per-set tally for reads that span sets (a read is tagged in the set of its most
confident observation), a weighted-MEC optimum (this is greedy best-link chaining), a phase quality beyond the link margin.
Realignment against the two haplotypes is realign.py's.
"""
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import DEFAULT_ALPHABET, MAX_QUAL
from .genotype import GT_HET, Genotypes, GenotypeWeights, _records_with_sites
from .pileup import _note_bad_reads, _read_args
from .readmap import MAX_REFERENCE, _int_in

MAX_REACH = 8
CIS, TRANS = 0, 1                              # the last index of PhaseLinks.links
NEITHER = 2                                   # the column of PhaseLinks.observed beside the two alleles'

PhaseSites = namedtuple("PhaseSites", "pos alleles site_of")
PhaseSites.__doc__ = """pos [S] int32: the heterozygous positions, ascending; alleles [S, 2] uint8: their two called labels in allele
order (0: deleted); site_of [R] int32: the site of a position, or -1.  All on the device."""

PhaseLinks = namedtuple("PhaseLinks", "links observed used")
PhaseLinks.__doc__ = """links [S, reach, 2] int64: [site s][d - 1][cis, trans], the summed weights of the reads that show sites s - d and s
on the same (cis: both first alleles or both second) or on opposite haplotypes; observed [S, 3] int32: the reads that show the
first allele, the second, neither; used [B] int8 of the last batch, as Pileup.used.  On the device."""

Phasing = namedtuple("Phasing", "parent flip margin root parity ps set_size")
Phasing.__doc__ = """parent [S] int32: the site a site is linked to (itself: a root); flip [S] uint8: 1 where the link is trans; margin [S]
int32: |cis - trans| of that link, 0 at a root; root [S] int32; parity [S] uint8: the xor of the flips up to the root -- haplotype 1
carries alleles[s][parity[s]], haplotype 2 the other; ps [S] int32: pos[root], the phase set's name; set_size [S] int32: the sites of
the set (1: unphased).  On the device."""

Haplotags = namedtuple("Haplotags", "hp ps weight n_sites")
Haplotags.__doc__ = """hp [B] uint8: 1 or 2, the haplotype the read lies on, 0 undecided; ps [B] int32: the phase set it was tagged in
(a 0-based position), -1 without one; weight [B, 2] int32: the summed weights of its observations for haplotype 1 and 2 in that set;
n_sites [B, 2] int32: its observations in that set, and in other sets.  On the device."""

PhasedRecord = namedtuple("PhasedRecord", "pos kind ref alts gt qual gq depth ps")
PhasedRecord.__doc__ = """a GenotypeRecord with ps: the phase set (the 0-based position of its first site) where gt is phased ("0|1",
"1|0", "1|2", "2|1": the allele on haplotype 1, then on haplotype 2), else None beside the unphased gt."""


def phase_sites(genotypes):
    """The heterozygous positions of a Genotypes as sites: every p with flags[p] & HET, which leaves out
    LOW_DEPTH positions and reference labels that are no base.  Heterozygous insertions (INS_HET) are not sites.  Built with torch
    ops on the device; S, the number of sites, is READ BACK ONCE because it sizes every later table -- the only host
    synchronisation of the phasing functions.  S == 0 is legal.  Returns PhaseSites."""
    what = "phase_sites"
    if not isinstance(genotypes, Genotypes):
        raise ValueError("wavenet_speech_amd.%s: genotypes must be Genotypes, got %s" % (what, type(genotypes).__name__))
    flags = _args.gpu_tensor(genotypes.flags, what, "genotypes.flags", (torch.uint8,))
    alleles = _args.gpu_tensor(genotypes.alleles, what, "genotypes.alleles", (torch.uint8,), device=flags.device)
    R = int(flags.shape[0])
    if flags.dim() != 1 or tuple(alleles.shape) != (R, 2) or not 1 <= R <= MAX_REFERENCE:
        raise ValueError("wavenet_speech_amd.%s: genotypes.flags must have shape (R,) and alleles (R, 2), 1 <= R <= %d, got %s and %s"
                         % (what, MAX_REFERENCE, tuple(flags.shape), tuple(alleles.shape)))
    pos = torch.nonzero(flags & GT_HET).reshape(-1)                  # the one host synchronisation: S sizes the tables
    site_of = torch.full((R,), -1, dtype=torch.int32, device=flags.device)
    site_of[pos] = torch.arange(pos.shape[0], dtype=torch.int32, device=flags.device)
    return PhaseSites(pos.to(torch.int32), alleles[pos].contiguous(), site_of)


def _sites(sites, what, dev, R=None):
    """a PhaseSites on `dev` checked -> (S, R)"""
    if not isinstance(sites, PhaseSites):
        raise ValueError("wavenet_speech_amd.%s: sites must be PhaseSites, got %s" % (what, type(sites).__name__))
    for t, name, dtype in ((sites.pos, "pos", torch.int32), (sites.alleles, "alleles", torch.uint8), (sites.site_of, "site_of", torch.int32)):
        _args.gpu_tensor(t, what, "sites." + name, (dtype,), device=dev)
    S = int(sites.pos.shape[0])
    if sites.pos.dim() != 1 or tuple(sites.alleles.shape) != (S, 2) or sites.site_of.dim() != 1 or not all(
            t.is_contiguous() for t in sites):
        raise ValueError("wavenet_speech_amd.%s: sites must hold contiguous pos (S,), alleles (S, 2) and site_of (R,), got %s, %s, %s"
                         % (what, tuple(sites.pos.shape), tuple(sites.alleles.shape), tuple(sites.site_of.shape)))
    if R is not None and int(sites.site_of.shape[0]) != R:
        raise ValueError("wavenet_speech_amd.%s: sites of a reference of %d positions beside R = %d" % (what, int(sites.site_of.shape[0]), R))
    if S > int(sites.site_of.shape[0]):
        raise ValueError("wavenet_speech_amd.%s: %d sites on %d positions" % (what, S, int(sites.site_of.shape[0])))
    return S, int(sites.site_of.shape[0])


def _phase_reads(what, alignment, lo, ref_lengths, strand, query, query_lengths, sites, qual, flat_qual, gap_qual, cap, min_qual, keep):
    """the arguments phase_links and haplotag share, checked as pileup_evidence checks them -> (the C ABI's leading arguments up to
    n_sites as a list, the prepared tensors those pointers point into -- the caller holds them until its call is made --, B, S, R,
    dev)"""
    flat_qual = _int_in(what, "flat_qual", flat_qual, 0, MAX_QUAL)
    gap_qual = _int_in(what, "gap_qual", gap_qual, 0, MAX_QUAL)
    if not isinstance(sites, PhaseSites) or not isinstance(sites.site_of, torch.Tensor) or sites.site_of.dim() != 1:
        raise ValueError("wavenet_speech_amd.%s: sites must be PhaseSites, got %s" % (what, type(sites).__name__))
    R, min_qual, ops, ops_len, lo, ref_lengths, strand, query, query_lengths, qual, keep = _read_args(
        what, alignment, lo, ref_lengths, strand, query, query_lengths, int(sites.site_of.shape[0]), qual, min_qual, keep)
    B, M, max_ops, dev = int(query.shape[0]), int(query.shape[1]), int(ops.shape[1]), query.device
    S, _ = _sites(sites, what, dev, R)
    if cap is not None:
        cap = _args.gpu_tensor(cap, what, "cap", (torch.uint8,), device=dev)
        if tuple(cap.shape) != (B,):
            raise ValueError("wavenet_speech_amd.%s: cap must be uint8 of shape (%d,), got %s" % (what, B, tuple(cap.shape)))
        cap = cap.contiguous()
    held = (ops, ops_len, lo, ref_lengths, strand, query, query_lengths, qual, keep, cap)
    args = [_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_lengths), _p(strand), _p(query), query.stride(0), _p(query_lengths), _p(qual),
            qual.stride(0) if qual is not None else 0, _p(keep), B, M, max_ops, R, _p(cap), flat_qual, gap_qual, min_qual, _p(sites.site_of),
            _p(sites.alleles), S]
    return args, held, B, S, R, dev


def phase_links(alignment, lo, ref_lengths, strand, query, query_lengths, sites, qual=None, flat_qual=20, gap_qual=20, cap=None, min_qual=0,
                keep=None, reach=4, into=None):
    """Adds what every read of a batch shows at the sites, and how it links neighbouring sites, into tables over the sites (DESIGN.md
    section 7w), one launch and no host synchronisation.  The reads, and alignment, lo, ref_lengths, strand, query, query_lengths,
    qual, flat_qual, gap_qual, cap, min_qual and keep, are pileup_evidence's with its refusals (R is the sites' own); sites: the
    PhaseSites; reach in [1, 8]: how many sites back a site is linked; into: an earlier PhaseLinks of the same S and reach whose
    tables are accumulated in place (and returned; `used` is replaced).
    An OBSERVATION is a column for which pileup_evidence adds -- a base counted under its label, or a deletion -- at a position that
    is a site s.  Its weight is q' = min(q, cap[b]), q the base's qual, flat_qual without qual, gap_qual for a deletion; its allele
    x is 0 if the label (0 for a deletion) equals sites.alleles[s, 0], 1 if it equals alleles[s, 1], else neither.  observed[s, x]
    counts it (column 2: neither).  For every two observations of one read at sites s - d and s, 1 <= d <= reach, both with x in
    {0, 1}, min(q'(s - d), q'(s)) is added to links[s, d - 1, x(s - d) xor x(s)]: 0 cis, 1 trans.  Adds are 64-bit integer atomics.
    Returns PhaseLinks; with S == 0 empty tables, without a launch (`used` is then None: no read was looked at).  Skipped and bad
    reads are pileup's and are reported through check_device_flags() likewise."""
    what = "phase_links"
    reach = _int_in(what, "reach", reach, 1, MAX_REACH)
    args, held, B, S, R, dev = _phase_reads(what, alignment, lo, ref_lengths, strand, query, query_lengths, sites, qual, flat_qual, gap_qual,
                                                 cap, min_qual, keep)
    if into is not None and not isinstance(into, PhaseLinks):
        raise ValueError("wavenet_speech_amd.%s: into must be a PhaseLinks, got %s" % (what, type(into).__name__))
    with torch.cuda.device(dev):
        links = _args.into_table(into, "links", (S, reach, 2), dev, what, torch.int64)
        observed = _args.into_table(into, "observed", (S, 3), dev, what, torch.int32)
        if S == 0:
            return PhaseLinks(links, observed, None)
        used = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().wn_phase_links(*args, reach, _p(links), _p(observed), _p(used), _p(bad), _stream()), "wn_phase_links")
        _note_bad_reads(bad, what, R)
    return PhaseLinks(links, observed, used)


def phase_chain(links, sites, min_margin=1):
    """Chains the sites into phase sets by their best links: greedy, no host synchronisation, 3 +
    ceil(log2 S) launches.  links: a PhaseLinks (any table of shape [S, reach, 2] will do); sites: the PhaseSites; min_margin in
    [0, 2^31 - 1]: the least |cis - trans| that links a site.
    For site s, margin_d = |cis - trans| of links[s, d - 1] over d = 1..min(reach, s); d* has the greatest, ties to the least d.
    s == 0 or margin_d* < min_margin: a root (parent s, flip 0, margin 0); else parent = s - d*, flip = trans > cis, margin =
    min(margin_d*, 2^31 - 1).  root and parity follow the parents to the root by pointer doubling; ps = pos[root]; set_size counts the
    sites of the tree (an integer atomic at the root, then a gather).  The root's alleles[., 0] lies on haplotype 1: haplotype 1
    carries alleles[s, parity[s]], haplotype 2 the other.  A site with set_size 1 is unphased.
    Returns Phasing; with S == 0 empty tables, without a launch."""
    what = "phase_chain"
    if not isinstance(links, PhaseLinks):
        raise ValueError("wavenet_speech_amd.%s: links must be a PhaseLinks, got %s" % (what, type(links).__name__))
    min_margin = _int_in(what, "min_margin", min_margin, 0, 2 ** 31 - 1)
    table = _args.gpu_tensor(links.links, what, "links.links", (torch.int64,))
    dev = table.device
    S, _ = _sites(sites, what, dev)
    if table.dim() != 3 or int(table.shape[0]) != S or not 1 <= int(table.shape[1]) <= MAX_REACH or int(table.shape[2]) != 2 or not table.is_contiguous():
        raise ValueError("wavenet_speech_amd.%s: links.links must be contiguous of shape (%d, reach, 2), reach in [1, %d], got %s"
                         % (what, S, MAX_REACH, tuple(table.shape)))
    reach = int(table.shape[1])
    with torch.cuda.device(dev):
        parent, margin, root, ps, set_size = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(5))
        flip, parity = (torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(2))
        if S:
            work = torch.empty(2 * S, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().wn_phase_chain(_p(table), _p(sites.pos), S, reach, min_margin, _p(parent), _p(flip), _p(margin), _p(root),
                                                  _p(parity), _p(ps), _p(set_size), _p(work), _stream()), "wn_phase_chain")
    return Phasing(parent, flip, margin, root, parity, ps, set_size)


def haplotag(alignment, lo, ref_lengths, strand, query, query_lengths, sites, phasing, qual=None, flat_qual=20, gap_qual=20, cap=None,
             min_qual=0, keep=None):
    """A haplotype tag per read, one launch and no host synchronisation.  The reads and their arguments are
    phase_links'; sites: the PhaseSites; phasing: the Phasing of phase_chain.
    Only a read's observations (phase_links) with x in {0, 1} at sites with set_size > 1 count.  The read's set is the root of the one
    with the greatest weight q', ties to the least site.  weight[b, x xor parity[s]] sums q' over those in that set; n_sites[b]
    counts those in that set, and those in other sets; hp is 1 if weight[b, 0] > weight[b, 1], 2 if less, 0 on a tie or without an
    observation; ps is the set's position, -1 without one.  A read that spans two sets is tagged in the set of its most confident
    observation only: WhatsHap's tally per set is not built.  A skipped or bad read has hp 0, ps -1 and zeros; bad reads are reported
    through check_device_flags() as pileup's are.
    Returns Haplotags; with S == 0 every read is untagged, without a launch."""
    what = "haplotag"
    args, held, B, S, R, dev = _phase_reads(what, alignment, lo, ref_lengths, strand, query, query_lengths, sites, qual, flat_qual, gap_qual,
                                                 cap, min_qual, keep)
    if not isinstance(phasing, Phasing):
        raise ValueError("wavenet_speech_amd.%s: phasing must be a Phasing, got %s" % (what, type(phasing).__name__))
    for name, dtype in (("root", torch.int32), ("parity", torch.uint8), ("set_size", torch.int32)):
        t = _args.gpu_tensor(getattr(phasing, name), what, "phasing." + name, (dtype,), device=dev)
        if tuple(t.shape) != (S,) or not t.is_contiguous():
            raise ValueError("wavenet_speech_amd.%s: phasing.%s must be contiguous of shape (%d,), got %s" % (what, name, S, tuple(t.shape)))
    with torch.cuda.device(dev):
        hp = torch.zeros(B, dtype=torch.uint8, device=dev)
        ps = torch.full((B,), -1, dtype=torch.int32, device=dev)
        weight, n_sites = (torch.zeros(B, 2, dtype=torch.int32, device=dev) for _ in range(2))
        if S:
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().wn_haplotag(*args, _p(sites.pos), _p(phasing.root), _p(phasing.parity), _p(phasing.set_size), _p(hp), _p(ps),
                                               _p(weight), _p(n_sites), _p(bad), _stream()), "wn_haplotag")
            _note_bad_reads(bad, what, R)
    return Haplotags(hp, ps, weight, n_sites)


def phased_records(reference, genotypes, pileup, sites, phasing):
    """host helper: genotype_records' list as PhasedRecords.  A "sub" record whose position, and a "del" record whose first deleted
    position, is a site with set_size > 1 gets ps and a phased gt "h1|h2": the indices, within the record's (ref, alts...) list, of
    the alleles on haplotype 1 and 2 -- 0|1, 1|0, 1|2 or 2|1; in a deletion record the deleted allele is 1 and the other 0.  A
    heterozygous deletion of n bases is n adjacent sites; its record takes the phase of the first.  Every other record -- homozygous
    ones, insertions, sites left alone by the chain -- keeps its `/` form with ps None."""
    what = "phased_records"
    if not isinstance(sites, PhaseSites) or not isinstance(phasing, Phasing):
        raise ValueError("wavenet_speech_amd.%s: sites must be PhaseSites and phasing a Phasing" % what)
    pairs = _records_with_sites(what, reference, genotypes, pileup)
    R, S = int(genotypes.flags.shape[0]), int(sites.pos.shape[0])
    if int(sites.site_of.shape[0]) != R or any(tuple(t.shape) != (S,) for t in (phasing.parity, phasing.ps, phasing.set_size)):
        raise ValueError("wavenet_speech_amd.%s: sites of %d positions and a phasing of %d sites beside genotypes of %d positions and %d sites"
                         % (what, int(sites.site_of.shape[0]), int(phasing.ps.shape[0]), R, S))
    if not pairs:
        return []
    at = torch.tensor([p for _, p in pairs], dtype=torch.long, device=sites.site_of.device)
    s = sites.site_of[at].long()
    safe = s.clamp(min=0)
    if S == 0:
        rows = [[-1, 0, 0, 0, 0, 0]] * len(pairs)
    else:
        rows = torch.stack([s, phasing.set_size[safe].long(), phasing.parity[safe].long(), phasing.ps[safe].long(),
                            sites.alleles[safe, 0].long(), sites.alleles[safe, 1].long()], 1).cpu().tolist()
    out = []
    for (v, _), (site, size, parity, ps, a0, a1) in zip(pairs, rows):
        if v.kind == "ins" or site < 0 or size <= 1:
            out.append(PhasedRecord(*v, None))
            continue
        first, second = (a1, a0) if parity else (a0, a1)             # the labels on haplotype 1 and 2
        if v.kind == "del":
            index = lambda label: 1 if label == 0 else 0             # noqa: E731
        else:
            listed = [v.ref] + list(v.alts)
            index = lambda label: listed.index((label,) if label else ())      # noqa: E731
        out.append(PhasedRecord(*v._replace(gt="%d|%d" % (index(first), index(second))), ps))
    return out


def vcf_phased_records(ref_name, reference, genotypes, pileup, sites, phasing, weights, alphabet=DEFAULT_ALPHABET):
    """host helper: vcf_genotype_records' lines with FORMAT GT:GQ:PS and the sample <gt>:<min(99, gq // scale)>:<ps + 1> (PS is
    1-based, the POS of the set's first site), `.` for PS where the record is unphased."""
    if not isinstance(weights, GenotypeWeights):
        raise ValueError("wavenet_speech_amd.vcf_phased_records: weights must be a GenotypeWeights, got %s" % type(weights).__name__)
    weights.checked("vcf_phased_records")
    char = lambda v: alphabet[v] if 0 < v < len(alphabet) else "N"   # noqa: E731
    out = []
    for v in phased_records(reference, genotypes, pileup, sites, phasing):
        alts = ",".join("".join(char(x) for x in alt) or ("<DEL>" if v.kind == "del" else "*") for alt in v.alts)
        out.append("%s\t%d\t.\t%s\t%s\t%d\tPASS\tDP=%d\tGT:GQ:PS\t%s:%d:%s\n"
                   % (ref_name, v.pos + 1, "".join(char(x) for x in v.ref), alts, v.qual // weights.scale, v.depth, v.gt,
                      min(99, v.gq // weights.scale), "." if v.ps is None else "%d" % (v.ps + 1)))
    return out
