"""
CIGAR runs and SAM text (csrc/wn_cigar.hip through wn_cigar_encode and wn_cigar_decode): the op rows of
pairwise_align / banded_align / left_align / realign as the run tables SAM and BAM carry, and the run tables of reads another
mapper aligned as op rows for left_align, pileup, pileup_evidence, phase_links, haplotag and quality_profile.

    rows = cigar_runs(aln, lo, ref_lengths, m.strand, lengths, index.R)          # on the device: only the run table leaves it
    text = sam_header("chr", index.R) + sam_records(names, labels, lengths, rows, "chr", reference=index, qual=q.qual,
                                                    mapq=m.mapq(), hp=tags.hp, ps=tags.ps)
    r = parse_sam(open("reads.sam"))                                             # reads minimap2 or dorado aligned
    c = cigar_ops(r.cigar.cuda(), r.n_cigar, r.pos, r.strand, index, r.labels.cuda(), r.lengths)
    pile = pileup(c.alignment, c.lo, c.ref_lengths, r.strand, r.labels.cuda(), r.lengths, index.R)

Everything the kernels write is an integer, so results equal the host reference of tests/cigar_ref.py exactly and two runs are
bitwise identical.  Neither kernel synchronises with the host; both capture into a graph.  There is no CPU fallback: CPU tensors
raise (the text helpers take tensors on any device, like fastq_records).  A run is one 32-bit word, len << 4 | code with BAM's codes
M 0, I 1, D 2, N 3, S 4, H 5, P 6, = 7, X 8, held in int32 tensors as its bit pattern.
Not built: BAM / BGZF bytes, coordinate sorting and indexing, more than one reference sequence, spliced N runs, stitching of
supplementary alignments, text formatting on the device.
"""
import math
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import DEFAULT_ALPHABET, MAX_OPS, MAX_PAIR_QUERY, MAX_QUAL, PairwiseAlignment, _alignment_ops, _op_rows, _pair_rows
from .pileup import _reference_labels
from .readmap import MAX_REFERENCE, ReadIndex, _int_in

MAX_CIGAR = 65535                             # runs of a row: BAM's own limit
CIGAR_CODES = "MIDNSHP=X"
UNMAPPED, REVERSE, SECONDARY, SUPPLEMENTARY = 4, 16, 256, 2048

CigarRows = namedtuple("CigarRows", "cigar n_cigar pos ref_span clip_front clip_back nm used eqx strand")
CigarRows.__doc__ = """cigar [B, max_cigar] int32: the runs, zero behind n_cigar [B]; pos [B]: the 0-based forward position of the first
aligned column; ref_span [B]: the reference labels from there to the last aligned column; clip_front, clip_back [B]: the soft clips in
forward orientation; nm [B]: the mismatch, insertion and deletion columns between the two; used [B] int8: 1 written, 0 skipped (n_cigar
0, pos -1), -1 a bad pair, -2 a row that needs n_cigar > max_cigar runs (nothing of it is written); eqx: whether matches and
mismatches are '=' and 'X' (else 'M'); strand [B]: as it was handed in.  All tensors int32 on the device but `used`."""

CigarAlignment = namedtuple("CigarAlignment", "alignment lo ref_lengths used")
CigarAlignment.__doc__ = """alignment: a PairwiseAlignment with ops [B, max_ops] uint8 in READ orientation, ops_len, matches, mismatches,
gaps and length as pairwise_align counts them, and a score of NaN (SAM carries none); lo [B]: the window's start, the records' pos;
ref_lengths [B]: the reference labels the runs consume; used [B] int8: 1 written, 0 skipped, -1 bad.  All on the device."""

SamReads = namedtuple("SamReads", "names flags pos mapq strand cigar n_cigar labels lengths qual hp ps")
SamReads.__doc__ = """what parse_sam returns, host tensors: names (a list), flags, pos (0-based, -1 unmapped), mapq [B] int32; strand [B]
int32 (0, 1, or -1 for an unmapped record); cigar [B, max n_cigar] int32 with n_cigar [B]; labels [B, L] int32 and lengths [B] in READ
orientation; qual [B, L] uint8 in READ orientation, or None when no record has one; hp, ps [B] int32 (0 where absent), or None when
no record carries the tag."""


def cigar_runs(alignment, lo, ref_lengths, strand, query_lengths, R, eqx=True, max_cigar=None, keep=None):
    """The CIGAR runs, POS, soft clips and NM of every read of a batch, one launch.
    alignment, lo, ref_lengths, strand, query_lengths, R, keep: as pileup takes them (the query labels are not needed; a row of n
    columns is held to at most M = min(n, 8192) query labels).  eqx: '=' and 'X' runs (True) or 'M' runs.  max_cigar in [1, 65535]:
    the columns of the run table; None is min(max_ops, 2 M + 1) + 2, which can never overflow: deletion runs must be separated by
    query-consuming columns, so a row of n_query labels has at most 2 n_query + 1 runs between two clips, and never more runs than
    columns.
    Everything is in FORWARD orientation: a reverse-strand row is walked back to front, as pileup walks it.  Columns before the
    first and after the last aligned column enter nothing: a query label there is soft-clipped, a reference label only moves pos.
    Returns CigarRows.  A read that pileup would skip, or without an aligned column, has used 0; a pair that pileup calls bad (an
    op outside 1..4, a length out of range, labels not consumed exactly, strand > 1, a window outside [0, R]) has used -1, a row that
    needs more than max_cigar runs used -2 with n_cigar the number needed; both are reported through check_device_flags()."""
    what = "cigar_runs"
    R = _int_in(what, "R", R, 1, MAX_REFERENCE)
    if not isinstance(eqx, bool):
        raise ValueError("wavenet_speech_amd.%s: eqx must be True or False, got %r" % (what, eqx))
    ops, ops_len = _alignment_ops(alignment, what)
    B, dev = int(ops.shape[0]) if ops.dim() == 2 else 0, ops.device
    if B < 1 or B > 65535:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 reads, got %d" % (what, B))
    ops, ops_len, max_ops = _op_rows(ops, ops_len, B, dev, what)
    M = min(max_ops, MAX_PAIR_QUERY)
    max_cigar = min(max_ops, 2 * M + 1) + 2 if max_cigar is None else _int_in(what, "max_cigar", max_cigar, 1, MAX_CIGAR)
    if max_cigar > MAX_CIGAR:
        raise ValueError("wavenet_speech_amd.%s: rows of %d columns may need %d runs, above BAM's %d: pass max_cigar" % (what, max_ops, max_cigar, MAX_CIGAR))
    lo, ref_lengths, strand, query_lengths = (_args.lengths(x, B, dev, what, name) for x, name in (
        (lo, "lo"), (ref_lengths, "ref_lengths"), (strand, "strand"), (query_lengths, "query_lengths")))
    if keep is not None:
        keep = torch.as_tensor(keep)
        if keep.dtype != torch.bool or keep.shape != (B,):
            raise ValueError("wavenet_speech_amd.%s: keep must be bool of shape (%d,), got %s %s" % (what, B, keep.dtype, tuple(keep.shape)))
        keep = keep.to(device=dev, dtype=torch.uint8).contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        cigar = torch.empty(B, max_cigar, dtype=torch.int32, device=dev)
        n_cigar = torch.empty(B, dtype=torch.int32, device=dev)
        fields = torch.empty(B, 5, dtype=torch.int32, device=dev)
        used = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_cigar_encode(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_lengths), _p(strand), _p(query_lengths), _p(keep), B,
                                       M, max_ops, R, int(eqx), max_cigar, _p(cigar), cigar.stride(0), _p(n_cigar), _p(fields), _p(used),
                                       _p(bad), _stream()), "wn_cigar_encode")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.cigar_runs: %d pair(s) whose ops do not fit (an op outside 1..4, a length out of "
                       "range, labels not consumed exactly, a strand above 1 or a window outside [0, %d]) or that need more than %d runs"
                       % (n, R, max_cigar))
    return CigarRows(cigar, n_cigar, fields[:, 0], fields[:, 1], fields[:, 2], fields[:, 3], fields[:, 4], used, eqx, strand)


def cigar_ops(cigar, n_cigar, pos, strand, reference, query, query_lengths, max_ops=None, strict=False):
    """The op rows of reads given by their CIGAR runs, one launch: what parse_sam returns, turned into what
    left_align, pileup, pileup_evidence, phase_links, haplotag and quality_profile take.
    cigar [B, max_cigar] int32 GPU rows (max_cigar <= 65535) with n_cigar, pos (0-based), strand [B]; reference: a ReadIndex or [R]
    labels, as call_consensus takes it; query [B, M] int32 or int64 GPU rows in READ orientation (M <= 8192) with query_lengths [B];
    max_ops: the columns of the op rows, None is min(2 M, 65535 + 8192) (a read whose deletions need more is bad: pass a wider
    row); strict: hold '=' and 'X' runs to the labels.
    M, = and X columns become op 1 where the reference label at the column equals the read's label on the forward strand (on
    strand 1 the complement 5 - v, taken from the read's far end) and op 2 elsewhere; I and S become op 4, D op 3; H, P and runs of
    length 0 vanish.  The row is written in read orientation and consumes exactly ref_lengths and query_lengths labels.
    Returns CigarAlignment.  A read with strand < 0 or n_cigar == 0 is skipped (used 0, ops_len 0, ref_lengths 0).  A read whose runs
    do not fit -- strand > 1, n_cigar or query_lengths outside its row, pos < 0, a code above 8 or N, more than max_ops columns, no
    reference label consumed, pos + the labels consumed > R, the query labels consumed differ from query_lengths, or with strict an
    '=' / 'X' column that is not one -- has used -1, ops_len 0, counts -1 and is reported through check_device_flags()."""
    what = "cigar_ops"
    if not isinstance(strict, bool):
        raise ValueError("wavenet_speech_amd.%s: strict must be True or False, got %r" % (what, strict))
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, M, dev = int(query.shape[0]), int(query.shape[1]), query.device
    if B < 1 or B > 65535 or M > MAX_PAIR_QUERY:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 reads of at most %d labels, got %d of %d" % (what, MAX_PAIR_QUERY, B, M))
    cigar = _args.int_rows(cigar, what, "cigar", B=B, shape="(%d, max_cigar)" % B, dtypes=(torch.int32,), device=dev, pad_empty=True,
                           lone_column_in_place=False)
    max_cigar = int(cigar.shape[1])
    if max_cigar > MAX_CIGAR:
        raise ValueError("wavenet_speech_amd.%s: at most %d runs per read, got %d" % (what, MAX_CIGAR, max_cigar))
    max_ops = min(2 * M, MAX_OPS) if max_ops is None else _int_in(what, "max_ops", max_ops, 1, MAX_OPS)
    n_cigar, pos, strand = (_args.lengths(x, B, dev, what, name) for x, name in ((n_cigar, "n_cigar"), (pos, "pos"), (strand, "strand")))
    bases = reference.bases if isinstance(reference, ReadIndex) else torch.as_tensor(reference)
    R = _int_in(what, "the reference's length", int(bases.shape[0]) if bases.dim() == 1 else 0, 1, MAX_REFERENCE)
    reference = _reference_labels(reference, R, dev, what)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ops = torch.empty(B, max_ops, dtype=torch.uint8, device=dev)
        ops_len, ref_lengths = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
        stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
        used = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        ws_bytes = lib.wn_cigar_decode_workspace_bytes(B, max_cigar)
        ws = _args._alloc_bytes(ws_bytes, "wn_cigar_decode_workspace_bytes", dev)
        _lib.check(lib.wn_cigar_decode(_p(cigar), cigar.stride(0), _p(n_cigar), _p(pos), _p(strand), _p(reference), R, _p(query),
                                       query.stride(0), _p(query_lengths), B, max_cigar, M, max_ops, int(strict), _p(ops), ops.stride(0),
                                       _p(ops_len), _p(ref_lengths), _p(stats), _p(used), _p(ws), ws_bytes, _p(bad), _stream()),
                   "wn_cigar_decode")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.cigar_ops: %d read(s) whose runs do not fit: a strand above 1, a length or a "
                       "position out of range, a code above 8 or N, more than %d columns, a window outside [0, %d], labels not consumed "
                       "exactly%s" % (n, max_ops, R, " or an = / X column that is not one" if strict else ""))
        score = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    alignment = PairwiseAlignment(score, stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], ops, ops_len)
    return CigarAlignment(alignment, pos, ref_lengths, used)


# ---- host text ------------------------------------------------------------------------------------------------------------------------

def _host_rows(rows, what):
    """(runs per read as [(len, code)], and the [B] columns of a CigarRows as lists)"""
    if not isinstance(rows, CigarRows):
        raise ValueError("wavenet_speech_amd.%s: rows must be the CigarRows of cigar_runs" % what)
    words = torch.as_tensor(rows.cigar).cpu().tolist()
    cols = [torch.as_tensor(t).cpu().reshape(-1).tolist() for t in (rows.n_cigar, rows.pos, rows.ref_span, rows.clip_front, rows.clip_back,
                                                                   rows.nm, rows.used, rows.strand)]
    runs = [[((v & 0xFFFFFFFF) >> 4, v & 15) for v in row[:n]] if u == 1 else [] for row, n, u in zip(words, cols[0], cols[6])]
    return runs, cols


def _cigar_text(runs, eqx):
    """the text of [(len, code)]; = and X runs merge into M when eqx is false; no runs: '*'"""
    if not eqx:
        merged = []
        for n, c in runs:
            c = 0 if c in (7, 8) else c
            if merged and merged[-1][1] == c:
                merged[-1] = (merged[-1][0] + n, c)
            else:
                merged.append((n, c))
        runs = merged
    return "".join("%d%s" % (n, CIGAR_CODES[c] if c < len(CIGAR_CODES) else "?") for n, c in runs) or "*"


def cigar_strings(rows, eqx=None):
    """host helper: the CIGAR text of every row of a CigarRows, '*' for a row that was not written.  eqx=False merges '=' and 'X'
    into 'M' in the text; None keeps the rows' own form."""
    runs, _ = _host_rows(rows, "cigar_strings")
    return [_cigar_text(r, rows.eqx if eqx is None else eqx) for r in runs]


def _letters(reference, alphabet, what):
    bases = reference.bases if isinstance(reference, ReadIndex) else torch.as_tensor(reference)
    if bases.dim() != 1 or bases.is_floating_point():
        raise ValueError("wavenet_speech_amd.%s: reference must be a ReadIndex or a row of integer labels" % what)
    return "".join(alphabet[v] if 0 < v < len(alphabet) else "N" for v in bases.cpu().tolist())


def _md(runs, pos, letters):
    out, u, at = [], 0, pos
    for n, c in runs:
        if c == 7:
            u, at = u + n, at + n
        elif c == 8:
            for _ in range(n):
                out.append("%d%s" % (u, letters[at]))
                u, at = 0, at + 1
        elif c == 2:
            out.append("%d^%s" % (u, letters[at:at + n]))
            u, at = 0, at + n
    return "".join(out) + "%d" % u


def md_strings(rows, reference, alphabet=DEFAULT_ALPHABET):
    """host helper: the MD:Z text of every written row of an eqx CigarRows against the reference (a ReadIndex or [R] labels), None for
    the others.  A run of '=' counts, every 'X' base prints the count and the reference letter, a 'D' run the count, '^' and the
    reference letters; insertions and clips are invisible; the count closes the text: 10A5^AC6, 0A5, 5A0."""
    what = "md_strings"
    runs, cols = _host_rows(rows, what)
    if not rows.eqx:
        raise ValueError("wavenet_speech_amd.%s: MD needs the '=' / 'X' runs of cigar_runs(eqx=True)" % what)
    letters = _letters(reference, alphabet, what)
    return [_md(r, p, letters) if u == 1 else None for r, p, u in zip(runs, cols[1], cols[6])]


def sam_header(ref_name, ref_length, sort_order="unknown", program=None):
    """host helper: the header lines of a SAM file over one reference sequence: @HD, @SQ and, with `program`, @PG"""
    if sort_order not in ("unknown", "unsorted", "queryname", "coordinate"):
        raise ValueError("wavenet_speech_amd.sam_header: sort_order must be unknown, unsorted, queryname or coordinate, got %r" % (sort_order,))
    out = ["@HD\tVN:1.6\tSO:%s\n" % sort_order, "@SQ\tSN:%s\tLN:%d\n" % (ref_name, int(ref_length))]
    if program is not None:
        out.append("@PG\tID:%s\tPN:%s\n" % (program, program))
    return out


def _tag_column(x, B, what, name):
    if x is None:
        return None
    x = torch.as_tensor(x).cpu().reshape(-1).tolist()
    if len(x) != B:
        raise ValueError("wavenet_speech_amd.%s: %s must hold %d values, got %d" % (what, name, B, len(x)))
    return x


def sam_records(names, labels, lengths, rows, ref_name, reference=None, qual=None, mapq=None, hp=None, ps=None, alphabet=DEFAULT_ALPHABET,
                eqx=None):
    """host helper: one SAM line per read, "\\n"-terminated, from the reads as they were decoded (labels [B, L], lengths [B], qual
    [B, L] or None: READ orientation) and the CigarRows of cigar_runs.
    FLAG 0 or 16; POS pos + 1; MAPQ floor(mapq + 0.5) as paf_records rounds it, 255 without one; RNEXT *, PNEXT 0, TLEN 0; SEQ the
    letters of the labels, reverse-complemented on strand 1 (a label outside the alphabet prints N); QUAL chr(qual + 33), reversed on
    strand 1, * without qual.  A read that was skipped (used 0) is written unmapped: FLAG 4, RNAME *, POS 0, MAPQ 0, CIGAR *, SEQ
    and QUAL as read.  Tags: NM:i always; MD:Z with a reference (a ReadIndex or [R] labels; needs eqx rows); HP:i and PS:i from
    haplotag's hp / ps where hp > 0.  eqx=False merges '=' and 'X' into 'M' in the text; None keeps the rows' own form.
    A row with used < 0 raises."""
    what = "sam_records"
    names = [str(n) for n in names]
    B = len(names)
    runs, (n_cigar, pos, _, _, _, nm, used, strand) = _host_rows(rows, what)
    seq_rows = torch.as_tensor(labels).cpu().tolist()
    ns = [int(n) for n in torch.as_tensor(lengths).cpu().reshape(-1).tolist()]
    quals = None if qual is None else torch.as_tensor(qual).cpu().tolist()
    if not (len(seq_rows) == len(ns) == len(used) == B) or (quals is not None and len(quals) != B):
        raise ValueError("wavenet_speech_amd.%s: %d names, %d label rows, %d lengths, %d cigar rows" % (what, B, len(seq_rows), len(ns), len(used)))
    text_eqx = rows.eqx if eqx is None else bool(eqx)
    if text_eqx and not rows.eqx:
        raise ValueError("wavenet_speech_amd.%s: rows of 'M' runs cannot be written with '=' and 'X'" % what)
    if reference is not None and not rows.eqx:
        raise ValueError("wavenet_speech_amd.%s: MD needs the '=' / 'X' runs of cigar_runs(eqx=True)" % what)
    letters = None if reference is None else _letters(reference, alphabet, what)
    mapq, hp, ps = (_tag_column(x, B, what, name) for x, name in ((mapq, "mapq"), (hp, "hp"), (ps, "ps")))
    char = lambda v: alphabet[v] if 0 < v < len(alphabet) else "N"   # noqa: E731
    out = []
    for b, name in enumerate(names):
        if used[b] < 0:
            raise ValueError("wavenet_speech_amd.%s: read %r has no CIGAR (used %d): a bad pair, or a row that needs more than max_cigar "
                             "runs" % (what, name, used[b]))
        row = [int(v) for v in seq_rows[b][:ns[b]]]
        q = None if quals is None else [int(v) for v in quals[b][:ns[b]]]
        if q is not None and any(not 0 <= v <= MAX_QUAL for v in q):
            raise ValueError("wavenet_speech_amd.%s: a quality outside [0, %d] in read %r" % (what, MAX_QUAL, name))
        mapped = used[b] == 1
        if mapped and strand[b] == 1:
            row = [5 - v if 1 <= v <= 4 else v for v in row[::-1]]
            q = None if q is None else q[::-1]
        seq = "".join(char(v) for v in row) or "*"
        qual_text = "*" if q is None or not q else "".join(chr(v + 33) for v in q)
        if not mapped:
            out.append("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (name, seq, qual_text))
            continue
        tags = ["NM:i:%d" % nm[b]]
        if letters is not None:
            tags.append("MD:Z:%s" % _md(runs[b], pos[b], letters))
        if hp is not None and hp[b] > 0:
            tags.append("HP:i:%d" % hp[b])
            if ps is not None:
                tags.append("PS:i:%d" % ps[b])
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\t%s\n" % (
            name, REVERSE if strand[b] == 1 else 0, ref_name, pos[b] + 1, 255 if mapq is None else int(math.floor(mapq[b] + 0.5)),
            _cigar_text(runs[b], text_eqx), seq, qual_text, "\t".join(tags)))
    return out


def parse_sam(lines, alphabet=DEFAULT_ALPHABET):
    """host helper: the records of SAM text (an iterable of lines; header lines are skipped) as the arguments of cigar_ops.
    Returns SamReads: pos is POS - 1; strand 1 with flag 16, -1 with flag 4 (cigar_ops skips those); labels, lengths and qual are
    turned back into READ orientation (reverse-complemented / reversed with flag 16); a letter outside the alphabet is label 0.
    Secondary and supplementary records (flags 256 and 2048) come back with their flags for the caller to filter."""
    what = "parse_sam"
    label_of = {ch: v for v, ch in enumerate(alphabet) if v > 0}
    label_of.update({ch.lower(): v for ch, v in label_of.items()})
    names, flags, pos, mapq, strand, runs, seqs, quals, hps, pss = [], [], [], [], [], [], [], [], [], []
    for line in lines:
        line = line.rstrip("\r\n")
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        if len(f) < 11:
            raise ValueError("wavenet_speech_amd.%s: a record of %d fields: %r" % (what, len(f), line[:80]))
        flag = int(f[1])
        rev = bool(flag & REVERSE)
        row, n = [], ""
        for ch in "" if f[5] == "*" else f[5]:
            if ch.isdigit():
                n += ch
            elif ch in CIGAR_CODES and n and int(n) < 1 << 28:
                v = (int(n) << 4) | CIGAR_CODES.index(ch)
                row.append(v - (1 << 32) if v >= 1 << 31 else v)     # the 32-bit word as int32
                n = ""
            else:
                raise ValueError("wavenet_speech_amd.%s: CIGAR %r of read %r" % (what, f[5], f[0]))
        if n:
            raise ValueError("wavenet_speech_amd.%s: CIGAR %r of read %r" % (what, f[5], f[0]))
        seq = [] if f[9] == "*" else [label_of.get(ch, 0) for ch in f[9]]
        q = None if f[10] == "*" else [ord(ch) - 33 for ch in f[10]]
        if q is not None and (len(q) != len(seq) or any(not 0 <= v <= MAX_QUAL for v in q)):
            raise ValueError("wavenet_speech_amd.%s: QUAL of read %r does not fit its SEQ" % (what, f[0]))
        if rev:
            seq = [5 - v if 1 <= v <= 4 else v for v in seq[::-1]]
            q = None if q is None else q[::-1]
        tags = {t[:2]: t[5:] for t in f[11:] if len(t) >= 5 and t[2] == ":" and t[4] == ":"}
        names.append(f[0]); flags.append(flag); pos.append(int(f[3]) - 1); mapq.append(int(f[4]))
        strand.append(-1 if flag & UNMAPPED else int(rev))
        runs.append(row); seqs.append(seq); quals.append(q)
        hps.append(int(tags["HP"]) if "HP" in tags else None); pss.append(int(tags["PS"]) if "PS" in tags else None)
    B = len(names)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)               # noqa: E731

    def padded(rows, dtype):
        t = torch.zeros(B, max([len(r) for r in rows] + [1]), dtype=dtype)
        for b, r in enumerate(rows):
            t[b, :len(r)] = torch.tensor(r, dtype=dtype)
        return t

    qual = None if all(q is None for q in quals) else padded([q or [] for q in quals], torch.uint8)
    if qual is not None and qual.shape[1] < max([len(s) for s in seqs] + [1]):
        qual = torch.nn.functional.pad(qual, (0, max(len(s) for s in seqs) - qual.shape[1]))
    tag = lambda col: None if all(v is None for v in col) else i32([v or 0 for v in col])      # noqa: E731
    return SamReads(names, i32(flags), i32(pos), i32(mapq), i32(strand), padded(runs, torch.int32), i32([len(r) for r in runs]),
                    padded(seqs, torch.int32), i32([len(s) for s in seqs]), qual, tag(hps), tag(pss))
