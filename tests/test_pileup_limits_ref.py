"""CPU: what the cases of tests/pileup_limits_cases.py reach, proved from tests/pileup_ref.py and the op strings alone (the library
is never loaded), so that tests/test_gpu_pileup_limits.py cannot pass vacuously.  Every assertion is a CONDITION on the
construction: if a case misses one, the case is changed, not the assertion.

Walk index: the pileup kernel walks a forward read front to back and a reverse-strand read back to front, in tiles of T = 256
columns and waves of 64; a seam is a walk index that is a multiple of 64."""
import numpy as np
import pytest

from tests import pileup_limits_cases as L
from tests import pileup_ref as P

T, WAVE = L.T, L.WAVE


def _walk(string, strand):
    """the columns in walk order and what the kernel's second pass meets between the first and the last aligned column:
    dict first, last, runs [(start, length)] of op 4, deletions {walk index}"""
    w = list(string[::-1] if strand else string)
    aligned = [c for c, v in enumerate(w) if v <= 2]
    first, last = aligned[0], aligned[-1]
    runs, c = [], first
    while c <= last:
        if w[c] == 4:
            e = c
            while w[e] == 4:
                e += 1
            runs.append((c, e - c))
            c = e
        else:
            c += 1
    return dict(walk=w, first=first, last=last, runs=runs, deletions={c for c in range(first, last + 1) if w[c] == 3})


# ---- the seam grid --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_the_grid_reaches_every_wave_and_tile_seam(strand):
    facts = {(v, s): _walk(L.grid_string(v, s), strand) for v in L.GRID_VARIANTS for s in L.GRID_OFFSETS}
    runs3 = {start for (v, s), f in facts.items() if v == "run3" for start, n in f["runs"] if n == 3}
    starts = {start for f in facts.values() for start, n in f["runs"]}
    ends = {start + n - 1 for f in facts.values() for start, n in f["runs"]}
    deletions = set().union(*(f["deletions"] for f in facts.values()))
    firsts, lasts = {f["first"] for f in facts.values()}, {f["last"] for f in facts.values()}
    assert L.GRID_MAX_INS == 4 and L.SEAMS == (64, 128, 192, 256, 320, 384, 448, 512)
    for q in L.SEAMS:
        assert q - 1 in runs3 and q - 2 in runs3, q                  # 1 and 2 columns before the seam; every slot is below max_ins
        assert q - 1 in ends and q in starts and q in deletions, q
        assert {q - 1, q} <= firsts and {q - 1, q} <= lasts, q
    # runs of max_ins and max_ins + 1 cross every seam too, and a read may start with end columns
    for variant, n in (("run_max", L.GRID_MAX_INS), ("run_over", L.GRID_MAX_INS + 1)):
        crossing = {start for (v, s), f in facts.items() if v == variant for start, m in f["runs"] if m == n}
        assert all(q - k in crossing for q in L.SEAMS for k in range(1, n)), variant
    assert all(f["first"] > 0 for (v, s), f in facts.items() if v == "ends" and not strand)


@pytest.mark.parametrize("strand", [0, 1])
def test_the_grid_is_used_whole(strand):
    pile = L.grid_pile(strand)
    B = len(L.GRID_VARIANTS) * len(L.GRID_OFFSETS)
    assert pile.used.tolist() == [1] * B and pile.bad == 0
    assert pile.counts[:, 1 - strand].sum() == 0 and pile.ins_lengths[:, L.GRID_MAX_INS].sum() >= len(L.GRID_OFFSETS)
    labels = L.grid().query[L.grid().query != 0]
    assert ((labels < 1) | (labels > 4)).sum() > 10                  # a few labels are no base


def _single(variant, s, strand):
    string, query = L.grid_string(variant, s), L.shifted_query(variant, s)
    return L.reference_pile(L.pack([string], [query], [0], [strand], L.GRID_MAX_INS))


@pytest.mark.parametrize("variant", L.GRID_SHIFTED)
@pytest.mark.parametrize("strand", [0, 1])
def test_shift_property(variant, strand):
    """The pile of offset s is the pile of offset 0 with the motif's cells moved by s positions: outside the four positions of
    the motif a read shows grid_reference_labels() whatever its offset, inside them what the read of offset 0 shows in its own.
    The expected pile of every offset so follows from ONE walk, that of offset 0, whose motif cells are written out by hand."""
    R = L.GRID_REF
    G = list(L.grid_reference_labels())
    plain = L.reference_pile(L.pack([[1] * R], [G], [0], [strand], L.GRID_MAX_INS))
    zero = _single(variant, 0, strand)
    window = lambda s: slice(R - 4 - s, R - s) if strand else slice(s, s + 4)            # noqa: E731  (the motif's positions)
    run = {"run3": 3, "run_max": 4, "run_over": 5}[variant]
    # offset 0 by hand, in forward order of the strand: aligned G, the run, aligned C, a deletion, the run of 1, `other`
    comp = lambda v: 5 - v if strand else v                                                # noqa: E731
    cells = np.zeros((4, 2, 6), dtype=np.int64)
    order = [3, 2, 1, 0] if strand else [0, 1, 2, 3]
    cells[order[0], strand, comp(L.MOTIF_ALIGNED[0]) - 1] = 1
    cells[order[1], strand, comp(L.MOTIF_ALIGNED[1]) - 1] = 1
    cells[order[2], strand, P.DEL] = 1
    cells[order[3], strand, P.OTHER] = 1
    assert np.array_equal(zero.counts[window(0)], cells)
    lengths = np.zeros((4, L.GRID_MAX_INS + 1), dtype=np.int64)
    after_run, after_single = (2, 0) if strand else (0, 2)           # a reverse run lies after the lower forward position
    lengths[after_run, min(run, L.GRID_MAX_INS + 1) - 1] = 1
    lengths[after_single, 0] = 1
    assert np.array_equal(zero.ins_lengths[window(0)], lengths)
    bases = np.zeros((4, L.GRID_MAX_INS, 4), dtype=np.int64)
    labels = L.MOTIF_RUN[:run][::-1] if strand else L.MOTIF_RUN[:run]
    for k, v in enumerate(labels[:L.GRID_MAX_INS]):
        if 1 <= v <= 4:
            bases[after_run, k, comp(v) - 1] = 1
    bases[after_single, 0, comp(L.MOTIF_SINGLE) - 1] = 1
    assert np.array_equal(zero.ins_bases[window(0)], bases)
    for s in L.GRID_OFFSETS:
        pile = _single(variant, s, strand)
        assert pile.used.tolist() == [1]
        inside = np.zeros(R, dtype=bool)
        inside[window(s)] = True
        for name in ("counts", "ins_lengths", "ins_bases"):
            got = getattr(pile, name)
            assert np.array_equal(got[inside], getattr(zero, name)[window(0)]), (name, s)
            assert np.array_equal(got[~inside], getattr(plain, name)[~inside]), (name, s)


# ---- whole tiles and waves of one op --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_whole_tiles_and_waves_of_one_op(strand):
    facts = [_walk(s, strand) for s in L.WHOLE_STRINGS]
    for op, f in ((4, facts[0]), (3, facts[1]), (4, facts[4])):      # a tile that is all op 4 (all op 3), between aligned columns
        w = f["walk"]
        assert any(all(v == op for v in w[t:t + T]) for t in range(T, f["last"] - T, T)) and f["first"] < T
    assert sum(all(v == 4 for v in facts[4]["walk"][t:t + T]) for t in range(0, L.MAX_QUERY, T)) == 30
    assert facts[0]["runs"] == [(7 if strand else 5, 3 * T + 10)] and facts[4]["runs"] == [(1, L.MAX_QUERY - 2)]
    waves = set()
    for f in facts[2:4]:                                             # op 4 in exactly one wave, aligned columns on either side
        (start, n), w = f["runs"][0], f["walk"]
        assert n == WAVE and start % WAVE == 0 and w[start - 1] == 1 and w[start + WAVE] == 1 and len(w) <= 2 * T
        waves.add(start // WAVE % 4)
    assert waves == {1, 2} if strand else waves == {1, 3}
    pile = L.whole_pile(strand)
    assert pile.used.tolist() == [1] * len(L.WHOLE_STRINGS) and pile.ins_lengths[:, L.WHOLE_MAX_INS].sum() == 4
    assert pile.counts[:, strand, P.DEL].sum() == 3 * T + 10


# ---- the size limits ------------------------------------------------------------------------------------------------------------

def test_the_size_limits_are_reached():
    reads = L.size()
    assert reads.ops.shape == (4, L.MAX_OPS) == (4, 73727) and reads.query.shape == (4, L.MAX_QUERY) == (4, 8192)
    assert reads.n_ref.tolist() == [65535] * 4 and reads.query_len.tolist() == [8192] * 4 and reads.ops_len.tolist() == [73725, 73725, 65535, 65535]
    assert all((row[n:] == L.PAD).all() and row[n:].size > 0 for row, n in zip(reads.ops, reads.ops_len))
    assert sorted(zip(reads.strand.tolist(), (reads.lo == 0).tolist(), (reads.lo + reads.n_ref == reads.R).tolist())) == \
        [(0, False, True), (0, False, True), (1, True, False), (1, True, False)]
    for string in L.SIZE_STRINGS:
        for strand in (0, 1):
            f = _walk(string, strand)
            w = f["walk"]
            assert sum(v != 4 for v in w[:f["last"]]) == 65534 and sum(v != 3 for v in w[:f["last"]]) == 8191    # i and j of the last column
            assert f["first"] == 0 and f["last"] == len(w) - 1
    assert -(-len(L.SIZE_STRINGS[0]) // T) == 288 and len(L.SIZE_STRINGS[0]) == 73725
    w = L.SIZE_STRINGS[1]
    assert all(any(v <= 2 for v in w[t:t + T]) for t in range(0, len(w), T))             # an aligned column in every tile
    pile = L.size_pile()
    assert pile.used.tolist() == [1] * 4 and pile.bad == 0
    # the long run: column max_ins of ins_lengths, its first max_ins bases in forward order on both strands
    q = reads.query[0]
    forward_at, reverse_at = int(reads.lo[0]) + 65533, int(reads.lo[1])
    assert pile.ins_lengths[forward_at].tolist() == [0] * 8 + [1] and pile.ins_lengths[reverse_at].tolist() == [0] * 8 + [1]
    assert pile.ins_lengths.sum() == 2
    for at, labels in ((forward_at, [int(v) for v in q[1:9]]), (reverse_at, [5 - int(v) for v in q[8190:8182:-1]])):
        want = np.zeros((8, 4), dtype=np.int64)
        for k, v in enumerate(labels):
            if 1 <= v <= 4:
                want[k, v - 1] = 1
        assert np.array_equal(pile.ins_bases[at], want) and want.sum() >= 6
    assert pile.counts[:, :, P.DEL].sum() == 2 * 65533 + 2 * (7 * 8191 + 6)


# ---- the batch limit ------------------------------------------------------------------------------------------------------------

def test_the_batch_limit_case():
    reads, pile = L.batch(), L.batch_pile()
    assert len(reads.ops_len) == 65535 == L.MAX_BATCH and reads.R == 2
    assert reads.strand[:4].tolist() == [0, 1, 0, 1] and reads.lo[:4].tolist() == [0, 0, 1, 1]
    good = L.MAX_BATCH - len(L.BATCH_BAD) - len(L.BATCH_SKIPPED)
    assert not set(L.BATCH_BAD) & set(L.BATCH_SKIPPED) and pile.bad == len(L.BATCH_BAD) == 7
    assert pile.counts.sum() == good == (pile.used == 1).sum() and (pile.used == -1).sum() == 7 and (pile.used == 0).sum() == 5
    assert (pile.counts.sum(2) > 16000).all() and pile.counts[:, :, P.OTHER].sum() > 100 and pile.ins_lengths.sum() == 0


# ---- the scan -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", L.SCAN_R)
def test_the_scan_case(R):
    n_tiles = -(-R // T)
    chunk = -(-n_tiles // 256)
    assert (n_tiles, chunk) == {L.SCAN_R[0]: (257, 2), L.SCAN_R[1]: (513, 3)}[R]
    owned = [max(0, min(n_tiles, (t + 1) * chunk) - min(n_tiles, t * chunk)) for t in range(256)]
    if R == L.SCAN_R[0]:
        assert owned[:128] == [2] * 128 and owned[128] == 1 and owned[129:] == [0] * 127
    else:
        assert owned[:171] == [3] * 171 and owned[171:] == [0] * 85
    calls = L.scan_calls(R)
    emitted = (calls.call != 0).astype(np.int64) + calls.ins_len
    assert set(emitted.tolist()) == set(range(10))
    totals = np.add.reduceat(emitted, np.arange(0, R, T))
    assert totals[L.SCAN_DELETED_TILE] == 0 and totals[L.SCAN_BREAK_TILE] == 0 and totals[L.SCAN_FULL_TILE] == 2304 == 9 * T
    assert (calls.flags[L.SCAN_DELETED_TILE * T:(L.SCAN_DELETED_TILE + 1) * T] == P.DELETION).all()
    assert (calls.flags[L.SCAN_BREAK_TILE * T:(L.SCAN_BREAK_TILE + 1) * T] == P.LOW_DEPTH).all()
    # a second route to the offsets besides the loop of call_consensus_ref
    assert np.array_equal(calls.offsets, np.concatenate([[0], np.cumsum(emitted)])) and calls.offsets[R] == emitted.sum() == len(calls.consensus)
    assert calls.offsets[R] < 2 ** 31


# ---- counts beside 2^31 ---------------------------------------------------------------------------------------------------------

def _i32(v):
    return np.array([v], dtype=np.int64).astype(np.int32)            # wraps as a 32-bit register does


def test_the_count_rows_sit_on_both_sides_of_the_threshold():
    """A pair is a row whose two products are equal and its twin whose count is one more.  With num = 2^15 - 1 and den = 2^15
    equality means c = num K, d = den K, and d < 2^31 means K <= 65535.  A product formed in 32 bits against the other in 64
    calls neither row of such a pair.  Both products wrapped to int32 keep the order of the exact ones for EVERY such K, though:
    they differ by 2^15, which reorders only if c den = 2^31 - 2^15 mod 2^32, that is K = 98305 mod 2^17.  The pairs `_2`
    are the same form under num = 2^15 - 2, where K = 81921 does just that."""
    rows = L.count_rows()
    assert L.COUNT_NAMES[:8] == tuple(p[0] for p in L.COUNT_PAIRS) and len(rows.ref) == len(L.COUNT_NAMES)
    assert (L.NUM, L.DEN, L.K) == (2 ** 15 - 1, 2 ** 15, 65535)
    assert L.COUNT_PAIRS[0][2:4] == ((2 ** 15 - 1) * 65535, 2 ** 15 * 65535)
    reordered = {}
    for p, (name, rule, c, d, (num, den), diff) in enumerate(L.COUNT_PAIRS):
        counts, lengths = rows.pile.counts[p], rows.pile.ins_lengths[p]
        assert int(counts[:, :5].sum()) == d < 2 ** 31 and c < 2 ** 31 and counts.max() < 2 ** 31 and lengths.max() < 2 ** 31
        assert (int(counts[:, 1].sum()) if rule == "base" else int(lengths.sum())) == c
        assert c * den - num * d == diff and diff == (den if "called" in name else 0)
        with np.errstate(over="ignore"):
            left, right = _i32(c) * _i32(den), _i32(num) * _i32(d)
            delta = left - right
        assert int(delta[0]) == diff                                 # the difference survives the wrap; the order need not
        reordered[name] = bool(left[0] > right[0]) != (c * den > num * d)
        narrow = (c * den) % 2 ** 32                                 # one product in 32 bits unsigned, the other exact
        assert not narrow > num * d
        call, inserted, flags, _ = P.call_position(counts, lengths, rows.pile.ins_bases[p], rows.ref[p], 3, num, den)
        want = (P.SUBSTITUTION if rule == "base" else P.INSERTION) if "called" in name else (P.AMBIGUOUS if rule == "base" else 0)
        assert flags == want, name
    assert not any(reordered[n] for n in ("base_equal", "base_called", "ins_equal", "ins_called"))
    assert reordered["base_called_2"] and reordered["ins_called_2"]
    assert not any((32767 * k) % 2 ** 17 == 65535 for k in range(1, 65536))


def test_the_count_rows_by_hand():
    rows = L.count_rows()
    at = L.COUNT_NAMES.index
    top = 2 ** 31 - 1
    call = lambda name, *rules: P.call_position(rows.pile.counts[at(name)], rows.pile.ins_lengths[at(name)], rows.pile.ins_bases[at(name)],        # noqa: E731
                                                rows.ref[at(name)], *rules)
    assert call("deletion_called", 3, L.NUM, L.DEN) == (0, [], P.DELETION, (L.NUM * L.K - 6, 7))
    assert call("deletion_called", 3, L.DEN, L.DEN)[2] == P.AMBIGUOUS
    d = lambda name: int(rows.pile.counts[at(name)][:, :5].sum())    # noqa: E731
    assert (d("depth_below"), d("depth_at"), d("strand_split")) == (top - 1, top, top)
    assert call("depth_below", top, 1, 2) == (2, [], P.LOW_DEPTH, (0, 0))
    assert call("depth_at", top, 1, 2) == (1, [3, 4], P.SUBSTITUTION | P.INSERTION, (2 ** 30, 2 ** 30 - 1))
    assert call("depth_at", top, L.DEN, L.DEN) == (2, [], P.AMBIGUOUS, (0, 0))            # c == d == n: nothing is above the whole
    assert call("strand_split", 3, L.NUM, L.DEN) == (2, [], P.SUBSTITUTION, L.SPLIT) and sum(L.SPLIT) == top
    assert call("strand_split", top, L.DEN, L.DEN)[2] == P.AMBIGUOUS and call("strand_split", 3, 0, 1)[2] == P.SUBSTITUTION | P.INSERTION
    assert (3, L.NUM, L.DEN) in L.COUNT_RULES and (3, L.DEN, L.DEN) in L.COUNT_RULES and (3, 0, 1) in L.COUNT_RULES
    assert {r[0] for r in L.COUNT_RULES} == {3, top}


# ---- every kind of record -------------------------------------------------------------------------------------------------------

def test_the_variants_case_has_every_kind_of_record():
    rows, calls = L.variants(), L.variant_calls()
    R, ref = L.VARIANT_R, [int(v) for v in rows.ref]
    assert R == T + 3 and (calls.flags & (P.SUBSTITUTION | P.DELETION | P.INSERTION) != 0).sum() * 3 >= R
    deleted = lambda p: bool(calls.flags[p] & P.DELETION)            # noqa: E731
    for p, what in L.VARIANT_FORCED.items():
        assert deleted(p) == ("del" in what) and bool(calls.flags[p] & P.SUBSTITUTION) == ("sub" in what), p
        assert bool(calls.flags[p] & P.INSERTION) == ("ins" in what), p
    records = P.variants_ref(rows.ref, calls, rows.pile)
    assert {r[1] for r in records} == {"sub", "del", "ins"}
    by_key = {(r[0], r[1]): r for r in records}
    assert by_key[(0, "del")][2:4] == ((ref[0], ref[1], ref[2]), (ref[2],))               # anchored on the FOLLOWING base
    assert by_key[(R - 3, "del")][2:4] == ((ref[R - 3], ref[R - 2], ref[R - 1]), (ref[R - 3],))
    assert by_key[(9, "del")][2:4] == ((ref[9], ref[10], ref[11]), (ref[9],)) and by_key[(12, "del")][2:4] == ((ref[12], ref[13]), (ref[12],))
    assert (19, "del") in by_key and (21, "sub") in by_key and (21, "del") in by_key and (23, "ins") in by_key and (23, "del") in by_key
    assert (31, "sub") in by_key and (31, "ins") in by_key and by_key[(31, "ins")][2] == (ref[31],)
    assert (35, "del") in by_key and (36, "ins") in by_key and len(by_key[(36, "ins")][3]) >= 2
    assert len(by_key) == len(records) and [r[:2] for r in records] == sorted(by_key, key=lambda k: (k[0], ("sub", "del", "ins").index(k[1])))
