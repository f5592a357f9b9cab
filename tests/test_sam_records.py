"""CPU: the SAM text of wavenet_speech_amd/sam.py on host tensors: parse_sam(sam_records(...)) returns what
went in -- the reverse strand, the reversed qualities, unmapped reads, the tags, the M and the = / X forms -- the MD strings against
the reference's, and paf_records with and without cigars."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import cigar_cases as K
from tests import cigar_ref as C

LABEL = {ch: v for v, ch in enumerate(" AGCT")}
LETTERS = "".join(" AGCT"[v] for v in K.reference_labels())


def _reads(eqx=True):
    """a small batch on both strands with one skipped read -> (Batch, reference Rows, CigarRows, names, qual)"""
    rng = np.random.default_rng(8)
    rows = [("r%d" % b, [4] * (b % 3) + K.random_walk(rng, 20 + 7 * b) + [3, 4][:b % 2 + 1], b & 1) for b in range(6)]
    rows.append(("all_insertion", [4] * 9, 0))                       # skipped: written unmapped
    t = K.assemble(rows, K.reference_labels(), 19, lo_step=11)
    enc = C.encode_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query_len, t.query.shape[1], len(t.reference), eqx=eqx)
    qual = rng.integers(0, 94, size=t.query.shape).astype(np.uint8)
    return t, enc, K.cigar_rows(enc, t.strand, eqx), qual


def test_round_trip_through_the_text():
    t, enc, rows, qual = _reads()
    B = len(t.names)
    hp, ps, mapq = [1, 2, 0, 1, 0, 2, 0], [101, 101, 0, 7, 0, 7, 0], [60.0, 0.4, 0.5, 17.49, 3.0, 59.5, 0.0]
    lines = W.sam_records(t.names, t.query, t.query_len, rows, "chr", reference=t.reference, qual=qual, mapq=mapq, hp=hp, ps=ps)
    assert len(lines) == B and all(l.endswith("\n") and l.count("\n") == 1 for l in lines)
    text = "".join(W.sam_header("chr", len(t.reference), program="wavenet_speech_amd") + lines)
    assert text.startswith("@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr\tLN:%d\n@PG\tID:wavenet_speech_amd\tPN:wavenet_speech_amd\n" % len(t.reference))
    r = W.parse_sam(text.splitlines(True))                           # header lines are skipped
    assert r.names == t.names and r.flags.tolist() == [0, 16, 0, 16, 0, 16, 4] and r.strand.tolist() == [0, 1, 0, 1, 0, 1, -1]
    assert r.pos.tolist() == enc.fields[:, 0].tolist() and r.pos[6] == -1
    assert r.mapq.tolist() == [60, 0, 1, 17, 3, 60, 0]               # floor(mapq + 0.5), as paf_records rounds; 0 unmapped
    assert r.n_cigar.tolist() == enc.n_cigar.tolist() and r.cigar[:, :enc.cigar.shape[1]].tolist() == enc.cigar[:, :r.cigar.shape[1]].tolist()
    assert r.lengths.tolist() == t.query_len.tolist() and r.labels.tolist() == t.query[:, :r.labels.shape[1]].tolist()       # READ orientation again
    for b in range(B):
        assert r.qual[b, :t.query_len[b]].tolist() == qual[b, :t.query_len[b]].tolist(), b
    assert r.hp.tolist() == hp and r.ps.tolist() == [101, 101, 0, 7, 0, 7, 0]
    # the fields of one reverse read, by hand
    f = lines[1].rstrip("\n").split("\t")
    n = int(t.query_len[1])
    fwd = [5 - int(v) for v in t.query[1, :n][::-1]]
    assert f[:9] == ["r1", "16", "chr", str(enc.fields[1, 0] + 1), "0", C.text(C.unpack(enc.cigar[1, :enc.n_cigar[1]])), "*", "0", "0"]
    assert f[9] == "".join(" AGCT"[v] for v in fwd) and f[10] == "".join(chr(int(q) + 33) for q in qual[1, :n][::-1])
    assert f[11] == "NM:i:%d" % enc.fields[1, 4] and f[12] == "MD:Z:" + C.md_ref(C.unpack(enc.cigar[1, :enc.n_cigar[1]]), int(enc.fields[1, 0]), LETTERS)
    assert f[13:] == ["HP:i:2", "PS:i:101"] and lines[2].rstrip("\n").split("\t")[13:] == []
    # the unmapped read: * / 0 in the placement fields, SEQ and QUAL as read
    u = lines[6].rstrip("\n").split("\t")
    assert u[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] and u[9] == "".join(" AGCT"[int(v)] for v in t.query[6, :9]) and len(u) == 11
    assert u[10] == "".join(chr(int(q) + 33) for q in qual[6, :9])
    # the decoder on what came back returns the rows' spans
    d = C.decode_ref(r.cigar.numpy(), r.n_cigar.numpy(), r.pos.numpy(), r.strand.numpy(), t.reference, r.labels.numpy(), r.lengths.numpy(), t.ops.shape[1],
                     strict=True)
    assert d.used.tolist() == [1] * 6 + [0] and d.ref_lengths.tolist() == enc.fields[:, 1].tolist()


def test_m_form_and_missing_fields():
    t, enc, rows, _ = _reads()
    tm, encm, rowsm, _ = _reads(eqx=False)
    as_m = W.sam_records(t.names, t.query, t.query_len, rows, "chr", eqx=False)
    assert as_m == W.sam_records(tm.names, tm.query, tm.query_len, rowsm, "chr")
    f = as_m[0].rstrip("\n").split("\t")
    assert f[5] == C.text(C.unpack(encm.cigar[0, :encm.n_cigar[0]])) and "=" not in f[5] and "X" not in f[5] and "M" in f[5]
    assert f[4] == "255" and f[10] == "*" and f[11:] == ["NM:i:%d" % enc.fields[0, 4]]         # no mapq, no qual, no reference, no tags
    assert W.cigar_strings(rows) == [C.text(C.unpack(enc.cigar[b, :enc.n_cigar[b]])) or "*" for b in range(len(t.names))]
    assert W.cigar_strings(rows, eqx=False) == W.cigar_strings(rowsm) and W.cigar_strings(rows)[6] == "*"
    r = W.parse_sam(as_m)
    assert r.qual is None and r.hp is None and r.ps is None and r.n_cigar.tolist() == encm.n_cigar.tolist()
    md = W.md_strings(rows, t.reference)
    assert md[6] is None and md[:6] == [C.md_ref(C.unpack(enc.cigar[b, :enc.n_cigar[b]]), int(enc.fields[b, 0]), LETTERS) for b in range(6)]
    for call, msg in ((lambda: W.md_strings(rowsm, t.reference), "MD needs"), (lambda: W.sam_records(t.names, t.query, t.query_len, rowsm, "chr", eqx=True), "cannot be written"),
                      (lambda: W.sam_records(t.names, t.query, t.query_len, rowsm, "chr", reference=t.reference), "MD needs"),
                      (lambda: W.sam_records(t.names[:2], t.query, t.query_len, rows, "chr"), "2 names"),
                      (lambda: W.sam_records(t.names, t.query, t.query_len, rows._replace(used=torch.tensor([1, -2, 1, 1, 1, 1, 0])), "chr"), "has no CIGAR"),
                      (lambda: W.sam_records(t.names, t.query, t.query_len, None, "chr"), "rows must be the CigarRows"),
                      (lambda: W.sam_header("chr", 10, sort_order="sorted"), "sort_order")):
        with pytest.raises(ValueError, match=msg):
            call()


def test_md_strings_of_the_tag_specification():
    reference = [LABEL[ch] for ch in K.MD_LETTERS]
    cases = (("10=1X5=2D6=", 0, "10A5^AC6"), ("1X5=", 10, "0A5"), ("5=1X", 5, "5A0"), ("2X", 16, "0A0C0"), ("3=2D1X2=", 13, "3^AC0T2"),
             ("3S4=2I1=1S", 0, "5"))
    width = max(len(C.parse(c)) for c, _, _ in cases)
    cigar = torch.tensor([C.pack(C.parse(c)) + [0] * (width - len(C.parse(c))) for c, _, _ in cases], dtype=torch.int32)
    zeros = torch.zeros(len(cases), dtype=torch.int32)
    rows = W.CigarRows(cigar, torch.tensor([len(C.parse(c)) for c, _, _ in cases]), torch.tensor([p for _, p, _ in cases]), zeros, zeros, zeros, zeros,
                       torch.ones(len(cases), dtype=torch.int8), True, zeros)
    assert W.md_strings(rows, reference) == [md for _, _, md in cases]
    assert W.cigar_strings(rows) == [c for c, _, _ in cases]


def test_the_specification_reads_parse():
    lines = ["@HD\tVN:1.6\tSO:coordinate\n", "@SQ\tSN:ref\tLN:45\n"]
    lines += ["%s\t%d\tref\t%d\t30\t%s\t*\t0\t0\t%s\t*\n" % (name, 16 if name == "r003s" else 0, pos, cigar, seq)
              for name, pos, cigar, seq in K.SPEC_READS]
    lines.append("r004\t256\tref\t16\t30\t6M14N5M\t*\t0\t0\tATAGCTTCAGC\t*\tNM:i:0\n")
    lines.append("r005\t2048\tref\t1\t3\t*\t*\t0\t0\t*\t*\n")
    r = W.parse_sam(lines)
    assert r.names == [n for n, _, _, _ in K.SPEC_READS] + ["r004", "r005"] and r.flags.tolist() == [0, 0, 0, 0, 16, 256, 2048]
    assert r.pos.tolist() == [6, 8, 8, 8, 28, 15, 0] and r.n_cigar.tolist() == [5, 5, 2, 2, 2, 3, 0] and r.lengths.tolist() == [17, 14, 11, 6, 5, 11, 0]
    assert C.text(C.unpack(r.cigar[1, :5].tolist())) == "3S6M1P1I4M" and C.text(C.unpack(r.cigar[5, :3].tolist())) == "6M14N5M"
    assert r.labels[4, :5].tolist() == [LABEL[ch] for ch in "GCCTA"]                 # SEQ TAGGC with flag 16: the read itself was GCCTA
    d = C.decode_ref(r.cigar.numpy(), r.n_cigar.numpy(), r.pos.numpy(), r.strand.numpy(), [LABEL[ch] for ch in K.SPEC_REFERENCE], r.labels.numpy(),
                     r.lengths.numpy(), 64)
    assert d.used.tolist() == [1, 1, 1, 1, 1, -1, 0] and d.ops[4, :5].tolist() == [1] * 5       # the spliced N run is refused
    for bad in ("r\t0\tref\t1\t3\t4Q\t*\t0\t0\tACGT\t*\n", "r\t0\tref\t1\t3\t4\t*\t0\t0\tACGT\t*\n", "r\t0\tref\t1\t3\t4M\t*\t0\t0\tACGT\t!!\n", "r\t0\tref\n"):
        with pytest.raises(ValueError, match="wavenet_speech_amd.parse_sam"):
            W.parse_sam([bad])


def test_paf_records_with_and_without_cigars():
    t, enc, rows, _ = _reads()
    B = len(t.names)
    table = torch.tensor([[1600, int(t.strand[b]), 100 + b, 200 + b, 0, 30, 20, 160] if b < 6 else [-2 ** 31, -1, -1, -1, -1, -1, 0, -2 ** 31] for b in range(B)],
                         dtype=torch.int32)
    anchors = W.Anchors(None, None, None, None, torch.as_tensor(t.query_len), 15, 1000, None)
    m = W.ReadMapping(*(table[:, k] for k in range(8)), None, None, anchors=anchors)
    plain = W.paf_records(t.names, t.query_len, m, "chr", ref_length=len(t.reference))
    assert plain[0] == "r0\t%d\t0\t30\t+\tchr\t%d\t100\t200\t30\t100\t60\n" % (t.query_len[0], len(t.reference)) and len(plain) == 6
    tagged = W.paf_records(t.names, t.query_len, m, "chr", ref_length=len(t.reference), cigars=rows)
    for b, (a, c) in enumerate(zip(plain, tagged)):
        inner = [(n, k) for n, k in C.unpack(enc.cigar[b, :enc.n_cigar[b]]) if k != C.S]
        assert c == a[:-1] + "\tNM:i:%d\tcg:Z:%s\n" % (enc.fields[b, 4], C.text(inner)), b
    with pytest.raises(ValueError, match="wavenet_speech_amd.paf_records: a mapped read has no CIGAR"):
        W.paf_records(t.names, t.query_len, m, "chr", ref_length=len(t.reference), cigars=rows._replace(used=torch.tensor([1, -1, 1, 1, 1, 1, 0])))
