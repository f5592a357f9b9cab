"""CPU: the host reference of the CIGAR encoder and decoder (tests/cigar_ref.py) held to the worked example of
include/wavenet_amd.h, to the SAM specification's own example reads, to the MD strings of the SAM tag specification, and -- over
every op row of up to six columns on both strands -- to what a run table must consume and to both round trips."""
import numpy as np
import pytest

from tests import cigar_cases as K
from tests import cigar_ref as C
from tests import pileup_ref as P

LABEL = {ch: v for v, ch in enumerate(" AGCT")}


def _encode_example(strand, eqx):
    ops = np.array([K.EXAMPLE], dtype=np.uint8)
    return C.encode_row(ops[0], len(K.EXAMPLE), len(K.EXAMPLE), 10, 9, strand, 9, 9, 100, eqx=eqx)


@pytest.mark.parametrize("strand, eqx, want", [(0, True, ("2S2=1X1I1=2D1=1S", 11, 7, 2, 1, 4)), (0, False, ("2S3M1I1M2D1M1S", 11, 7, 2, 1, 4)),
                                                (1, True, ("1S1=2D1=1I1X2=2S", 11, 7, 1, 2, 4))])
def test_the_worked_example(strand, eqx, want):
    e = _encode_example(strand, eqx)
    assert (C.text(e.runs), e.pos, e.ref_span, e.clip_front, e.clip_back, e.nm) == want and e.used == 1


def _spec_read(name):
    _, pos, cigar, seq = next(r for r in K.SPEC_READS if r[0] == name)
    reference = [LABEL[ch] for ch in K.SPEC_REFERENCE]
    query = [LABEL[ch] for ch in seq]
    runs = C.parse(cigar)
    d = C.decode_row(C.pack(runs), len(runs), pos - 1, 0, reference, query, len(query), len(runs), len(query), 64)
    return d, reference, query, pos - 1


def test_the_specification_read_r001():
    """8M2I4M1D3M at position 7: NM 3, MD 12^G3"""
    d, reference, query, pos = _spec_read("r001")
    assert d.used == 1 and d.ops == [1] * 8 + [4, 4] + [1] * 4 + [3] + [1] * 3 and d.ref_len == 16 and d.stats == [15, 0, 3, 18]
    e = C.encode_row(d.ops, len(d.ops), len(d.ops), pos, d.ref_len, 0, len(query), len(query), len(reference))
    assert (C.text(e.runs), e.pos + 1, e.nm) == ("8=2I4=1D3=", 7, 3)
    assert C.md_ref(e.runs, e.pos, K.SPEC_REFERENCE) == "12^G3"
    m = C.encode_row(d.ops, len(d.ops), len(d.ops), pos, d.ref_len, 0, len(query), len(query), len(reference), eqx=False)
    assert C.text(m.runs) == "8M2I4M1D3M"


@pytest.mark.parametrize("name, ops, back", [("r002", [4] * 3 + [1] * 6 + [4] + [1] * 4, "3S6=1I4="), ("r003", [4] * 5 + [1, 1, 2, 1, 1, 1], "5S2=1X3="),
                                             ("r003h", [1, 1, 2, 1, 1, 1], "2=1X3="), ("r003s", [1] * 5, "5=")])
def test_the_specification_reads_with_clips_and_pads(name, ops, back):
    """P and H emit nothing on decode; S is an op 4 at the row's end and a clip again on the way back"""
    d, reference, query, pos = _spec_read(name)
    assert d.used == 1 and d.ops == ops
    e = C.encode_row(d.ops, len(d.ops), len(d.ops), pos, d.ref_len, 0, len(query), len(query), len(reference))
    assert C.text(e.runs) == back and e.pos == pos


def test_md_strings_of_the_tag_specification():
    letters = K.MD_LETTERS
    P_ = C.parse
    assert C.md_ref(P_("10=1X5=2D6="), 0, letters) == "10A5^AC6"
    assert C.md_ref(P_("1X5="), 10, letters) == "0A5"
    assert C.md_ref(P_("5=1X"), 5, letters) == "5A0"
    assert C.md_ref(P_("2X"), 16, letters) == "0A0C0"                # ... A0C ...: a 0 between two mismatches
    assert C.md_ref(P_("3=2D1X2="), 13, letters) == "3^AC0T2"        # ... ^AC0T ...: a 0 between a deletion and a mismatch
    assert C.md_ref(P_("3S4=2I1=1S"), 0, letters) == "5"             # insertions and clips are invisible
    with pytest.raises(ValueError):
        C.md_ref(P_("4M"), 0, letters)


def _enumerated(strand):
    """every row of up to six columns as one Batch"""
    return K.assemble([("".join(map(str, row)), row, strand) for row in K.all_rows(6)], K.reference_labels(64), 3, lo_step=0, width=6)


@pytest.mark.parametrize("strand", [0, 1])
def test_every_short_row(strand):
    t = _enumerated(strand)
    B, Rr = len(t.names), len(t.reference)
    assert B == sum(4 ** n for n in range(1, 7))
    enc = C.encode_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query_len, 6, Rr)
    dec = C.decode_ref(enc.cigar.view(np.int32), enc.n_cigar, enc.fields[:, 0], t.strand, t.reference, t.query, t.query_len, 6)
    again = C.encode_ref(dec.ops, dec.ops_len, enc.fields[:, 0], dec.ref_lengths, t.strand, t.query_len, 6, Rr)
    assert enc.bad == dec.bad == again.bad == 0
    for b in range(B):
        walk = K.walk_of(t, b)
        runs = C.unpack(enc.cigar[b, :enc.n_cigar[b]])
        aligned = [w for w, v in enumerate(walk) if v <= 2]
        if int(t.ref_len[b]) == 0 or not aligned:
            assert enc.used[b] == 0 and not runs and enc.fields[b].tolist() == [-1, 0, 0, 0, 0] and dec.used[b] == 0, walk
            continue
        pos, ref_span, clip_front, clip_back, nm = (int(v) for v in enc.fields[b])
        assert enc.used[b] == 1 and all(n > 0 for n, _ in runs) and all(a[1] != c[1] for a, c in zip(runs, runs[1:])), walk
        assert sum(n for n, c in runs if c in (C.EQ, C.X, C.I, C.S)) == t.query_len[b], walk            # what each code consumes
        assert sum(n for n, c in runs if c in (C.EQ, C.X, C.D)) == ref_span, walk
        assert sum(n for n, c in runs if c in (C.X, C.I, C.D)) == nm, walk
        assert [c for _, c in runs].count(C.S) == (clip_front > 0) + (clip_back > 0) and runs[0][1] in (C.S, C.EQ, C.X), walk
        assert pos == t.lo[b] + sum(v != 4 for v in walk[:aligned[0]]), walk
        # decode(encode(A)): the clips, then the span, in read orientation; lo' = pos, n_ref' = ref_span
        want = K.round_trip_row(walk, enc.fields[b])
        assert dec.used[b] == 1 and dec.ref_lengths[b] == ref_span, walk
        assert dec.ops[b, :dec.ops_len[b]].tolist() == (want[::-1] if strand else want), walk
        assert dec.stats[b].tolist() == [want.count(1), want.count(2), want.count(3) + want.count(4), len(want)], walk
        # encode(decode(C)) == C: an encoder's output is canonical
        assert again.used[b] == 1 and again.n_cigar[b] == enc.n_cigar[b] and again.cigar[b].tolist() == enc.cigar[b].tolist(), walk
        assert again.fields[b].tolist() == enc.fields[b].tolist(), walk
    # end columns enter nothing: the piles of the decoded rows are the piles of the original rows
    pile = P.pileup_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query, t.query_len, Rr)
    back = P.pileup_ref(dec.ops, dec.ops_len, enc.fields[:, 0], dec.ref_lengths, t.strand, t.query, t.query_len, Rr)
    for name in ("counts", "ins_lengths", "ins_bases", "used"):
        assert np.array_equal(getattr(pile, name), getattr(back, name)), name
    assert pile.bad == back.bad == 0


def test_m_runs_merge_matches_and_mismatches():
    t = _enumerated(0)
    eqx = C.encode_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query_len, 6, len(t.reference))
    m = C.encode_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query_len, 6, len(t.reference), eqx=False)
    assert np.array_equal(eqx.fields, m.fields) and np.array_equal(eqx.used, m.used)
    for b in range(len(t.names)):
        merged = []
        for n, c in C.unpack(eqx.cigar[b, :eqx.n_cigar[b]]):
            c = C.M if c in (C.EQ, C.X) else c
            merged = merged[:-1] + [(merged[-1][0] + n, c)] if merged and merged[-1][1] == c else merged + [(n, c)]
        assert C.unpack(m.cigar[b, :m.n_cigar[b]]) == merged


def test_hand_made_run_tables():
    """the decoder's verdicts on tests/cigar_cases.decode_batch, one by one; the canonical ones come back from the encoder"""
    t = K.decode_batch()
    d = C.decode_ref(t.cigar, t.n_cigar, t.pos, t.strand, t.reference, t.query, t.query_len, t.max_ops)
    s = C.decode_ref(t.cigar, t.n_cigar, t.pos, t.strand, t.reference, t.query, t.query_len, t.max_ops, strict=True)
    used = dict(zip(t.names, d.used.tolist()))
    strict = dict(zip(t.names, s.used.tolist()))
    good = ["plain", "vanishing", "m_runs", "eq_over_mismatch", "x_over_match", "other_label"]
    for name, u in used.items():
        want = 1 if name.split("/")[0] in good + ["pos_last", "only_deletion", "columns_at_max"] else 0 if name in ("strand_-1", "n_cigar_0") else -1
        assert u == want, name
        assert strict[name] == (-1 if name.split("/")[0] in ("eq_over_mismatch", "x_over_match", "other_label") else want), name
    assert d.bad == sum(u < 0 for u in used.values()) and s.bad == d.bad + 6
    b = t.names.index("vanishing/0")
    assert d.ops[b, :d.ops_len[b]].tolist() == [4] * 3 + [1] * 4 + [4] * 2 + [2] * 3 + [3] * 2 + [1] + [4] * 2 and d.ref_lengths[b] == 10
    b = t.names.index("eq_over_mismatch/1")
    assert sorted(d.ops[b, :d.ops_len[b]].tolist()) == [1] * 12 + [2] + [4, 4]
    for name in ("plain/0", "plain/1"):                              # encode(decode(C)) == C for a canonical C
        b = t.names.index(name)
        e = C.encode_row(d.ops[b], int(d.ops_len[b]), t.max_ops, int(t.pos[b]), int(d.ref_lengths[b]), int(t.strand[b]), int(t.query_len[b]),
                         t.query.shape[1], len(t.reference))
        assert C.text(e.runs) == "5S10=2X3I4=2D6=1S" and e.pos == t.pos[b]


def test_a_row_that_does_not_fit_is_never_truncated():
    t, max_cigar = K.overflow_batch()
    e = C.encode_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query_len, t.query.shape[1], len(t.reference), max_cigar=max_cigar)
    assert e.used.tolist() == [1, -2, 1, -2] and e.n_cigar.tolist() == [600, 601, 600, 601] and e.bad == 2
    assert not e.cigar[1].any() and not e.cigar[3].any() and e.cigar[0].all() and e.fields[1, 2] == 1 and e.fields[3, 3] == 1
