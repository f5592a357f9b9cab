"""GPU: left_align (csrc/wn_leftalign.hip through wavenet_speech_amd/leftalign.py) against the reference of tests/leftalign_ref.py.
Labels are only compared, so every comparison is exact equality of ops, passes and settled; tests/test_leftalign_ref.py holds the
reference itself on the CPU, and the shared inputs are built once in tests/leftalign_cases.py.  The kernel works in tiles of 256
columns and waves of 64; a case is a few hundred columns and says in walk orientation where its run, its barrier and its shift
lie.  A case for strand 1 is the mirror of the one for strand 0, so that the walk meets the same seams."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import leftalign_cases as K
from tests import leftalign_ref as L
from tests import pileup_cases as C
from tests.gpu_calls import alignment as _alignment
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu
A_, G_, C_, T_ = 1, 2, 3, 4


def _assert_equal(got, want):
    assert got.alignment.ops.dtype == torch.uint8 and got.passes.dtype == torch.int32 and got.settled.dtype == torch.int8
    assert got.passes.cpu().tolist() == want.passes.tolist() and got.settled.cpu().tolist() == want.settled.tolist()
    assert np.array_equal(got.alignment.ops.cpu().numpy(), want.ops)


def _both(rows, strand, max_passes=8, mirror=True):
    """[(ops, a, b)] in WALK orientation through the reference and the kernel on one strand (a list: per row); they must agree
    exactly -> (LeftAligned, Aligned)"""
    strand = [strand] * len(rows) if isinstance(strand, int) else strand
    if mirror:
        rows = [(o[::-1], a[::-1], b[::-1]) if s == 1 else (o, a, b) for (o, a, b), s in zip(rows, strand)]
    ops, ops_len, a, a_len, b, b_len = K.batch(rows)
    want = L.left_align_ref(ops, ops_len, a, a_len, b, b_len, strand, max_passes)
    aln = _alignment(ops, ops_len)
    got = W.left_align(aln, _dev(a), _i32(a_len), _dev(b), _i32(b_len), _i32(strand), max_passes=max_passes)
    _assert_equal(got, want)
    assert got.alignment.ops_len is not None and torch.equal(got.alignment.ops_len, aln.ops_len) and torch.equal(aln.ops, _dev(ops))
    return got, want


def _row(*segments):
    """(ops, a, b) from ("m", labels) both sequences get the labels, ("d", labels) deleted from the read (op 3), ("i", labels)
    inserted into it (op 4)"""
    ops, a, b = [], [], []
    for kind, labels in segments:
        if kind == "m":
            ops, a, b = ops + [1] * len(labels), a + labels, b + labels
        elif kind == "d":
            ops, a = ops + [3] * len(labels), a + labels
        else:
            ops, b = ops + [4] * len(labels), b + labels
    return ops, a, b


def _filler(rng, n):
    return [int(v) for v in rng.integers(1, 5, size=n)]


def _site(rng, c, unit, before, edited, kind, tail=9, barrier=None):
    """a run of `edited` copies of `unit` at walk column c, `before` copies in front of it, after a label that differs from the
    unit's last one (or, with barrier=k, a gap of the other kind that cannot move, k columns in front of the run) -> (ops, a, b)"""
    stretch = unit * before
    other = [unit[-1] % 4 + 1]
    if barrier is None:
        head = [("m", _filler(rng, c - len(stretch) - 1) + other), ("m", stretch)]
    else:
        assert 1 <= barrier <= len(stretch) + 1
        cut = len(stretch) + 1 - barrier
        head = [("m", _filler(rng, c - barrier - cut - 1) + other), ("m", stretch[:cut]),
                ("i" if kind == "del" else "d", [stretch[cut - 1] % 4 + 1 if cut else other[0] % 4 + 1]), ("m", stretch[cut:])]
    row = _row(*head, ("d" if kind == "del" else "i", unit * edited), ("m", [unit[0] % 4 + 1] + _filler(rng, tail)))
    assert _start(row[0], 3 if kind == "del" else 4) == c
    return row


def _start(ops, v):
    """the walk column at which the last run of op v starts"""
    c = len(ops) - 1 - ops[::-1].index(v)
    while c > 0 and ops[c - 1] == v:
        c -= 1
    return c


def _shift(rows, want, strand, v, r):
    before = rows[r][0]
    after = want.ops[r, :len(before)].tolist()
    after = after[::-1] if strand == 1 else after
    return _start(before, v) - _start(after, v)


def test_every_short_row_on_both_strands():
    rows = K.short_rows()
    for strand in (0, 1):
        got, want = _both(rows, strand, mirror=False)
        assert want.bad == 0 and int(want.passes.max()) >= 3 and set(want.settled.tolist()) == {1}
    _both(rows, [r % 2 for r in range(len(rows))], mirror=False)
    W.check_device_flags()


def test_runs_at_every_wave_and_tile_seam():
    rng = np.random.default_rng(1)
    for strand in (0, 1):
        rows, shifts = [], []
        for q in range(64, 513, 64):
            for c in (q - 3, q, q - 1):                              # a run of three that ends on q - 1, starts on q, straddles q
                rows.append(_site(rng, c, [A_, G_, C_], 2, 1, "del"))
                rows.append(_site(rng, c, [T_], 5, 3, "ins"))
                shifts += [6, 5]
        got, want = _both(rows, strand)
        assert [_shift(rows, want, strand, 3 if r % 2 == 0 else 4, r) for r in range(len(rows))] == shifts
        assert want.passes.tolist() == [1] * len(rows)
    W.check_device_flags()


def test_barriers_in_an_earlier_wave_and_tile_and_a_territory_over_three_tiles():
    rng = np.random.default_rng(2)
    rows = [_site(rng, 230, [A_], 200, 1, "del", barrier=130),       # the barrier at column 100: two waves below the run
            _site(rng, 300, [A_], 100, 2, "del", barrier=50),        # at 250: in the tile before
            _site(rng, 600, [A_], 500, 1, "ins", barrier=400),       # at 200: the territory (200, 601) spans three tiles
            _site(rng, 600, [G_, T_], 250, 1, "del", barrier=400),
            _site(rng, 700, [C_], 650, 1, "del")]                    # no barrier but the sequence, three tiles away
    for strand in (0, 1):
        got, want = _both(rows, strand)
        assert [_shift(rows, want, strand, v, r) for r, v in enumerate((3, 3, 4, 3, 3))] == [129, 49, 399, 399, 650]
        assert want.passes.tolist() == [1] * 5
    W.check_device_flags()


def test_shift_lengths_cut_short_by_the_sequence_and_by_the_barrier():
    rng = np.random.default_rng(3)
    sizes = (0, 1, 63, 64, 65, 300)
    rows = [_site(rng, 320, [A_], s, 1, "del") for s in sizes] + [_site(rng, 320, [C_], s, 2, "ins") for s in sizes]
    rows += [_site(rng, 320, [A_], s + 5, 1, "del", barrier=s + 1) for s in sizes] + [_site(rng, 320, [C_], s + 7, 2, "ins", barrier=s + 1) for s in sizes]
    for strand in (0, 1):
        got, want = _both(rows, strand)
        assert [_shift(rows, want, strand, 3 if (r // 6) % 2 == 0 else 4, r) for r in range(24)] == list(sizes) * 4
        assert want.passes.tolist()[:12] == [0] + [1] * 5 + [0] + [1] * 5
    W.check_device_flags()


def test_run_lengths_over_a_periodic_stretch():
    rng = np.random.default_rng(4)
    rows, shifts = [], []
    for l in (1, 2, 3, 70, 300):
        while True:
            unit = _filler(rng, l)
            if K._primitive(unit):
                break
        rows += [_site(rng, 2 * l + 20, unit, 2, 1, "del"), _site(rng, l + 20, unit, 1, 1, "ins"), _site(rng, 60, [G_], 40, l, "del"),
                 _site(rng, 60, [G_], 40, l, "ins")]
        shifts += [2 * l, l, 40, 40]
    for strand in (0, 1):
        got, want = _both(rows, strand)
        assert [_shift(rows, want, strand, 3 if r % 2 == 0 else 4, r) for r in range(len(rows))] == shifts
    # s < l, s == l, s > l with the run on the tile seam, and landing on it
    rows = [_site(rng, c, [A_], s, 4, kind) for c in (256, 256 + 2, 256 + 4, 256 + 9) for s in (2, 4, 9) for kind in ("del", "ins")]
    for strand in (0, 1):
        got, want = _both(rows, strand)
        assert [_shift(rows, want, strand, 3 if r % 2 == 0 else 4, r) for r in range(len(rows))] == [2, 2, 4, 4, 9, 9] * 4
    W.check_device_flags()


def _five_passes(rng, at):
    """insertions and deletions by turns in a homopolymer: every pass moves the whole chain one column on"""
    return _row(("m", _filler(rng, at) + [G_, A_, A_]), ("i", [A_]), ("d", [A_]), ("i", [A_]), ("d", [A_]), ("i", [A_]), ("m", [A_, C_] + _filler(rng, 5)))


def test_passes_one_at_a_time_and_merges():
    rng = np.random.default_rng(5)
    rows = [_five_passes(rng, at) for at in (0, 57, 250, 251, 252, 253, 254, 255, 256)]
    for strand in (0, 1):
        seen = []
        for max_passes in range(1, 7):
            got, want = _both(rows, strand, max_passes=max_passes)
            assert want.passes.tolist() == [min(max_passes, 5)] * len(rows) and want.settled.tolist() == [int(max_passes > 5)] * len(rows)
            seen.append(want.ops)
        assert all(not np.array_equal(x, y) for x, y in zip(seen[:5], seen[1:5])) and np.array_equal(seen[4], seen[5])
    merges = [_row(("m", _filler(rng, at) + [G_, A_]), ("d", [A_]), ("m", [A_] * 3), ("d", [A_]), ("m", [T_] + _filler(rng, 4))) for at in (3, 253, 254, 255, 256)]
    merges += [_row(("m", _filler(rng, at) + [G_, A_]), ("i", [A_, A_]), ("m", [A_] * 70), ("i", [A_]), ("m", [A_] * 70), ("i", [A_] * 3), ("m", [T_] + _filler(rng, 4)))
               for at in (3, 120)]
    beside = [_row(("m", _filler(rng, at) + [G_]), ("d", [C_]), ("m", [A_] * 3), ("i", [A_]), ("m", [T_] + _filler(rng, 4))) for at in (3, 250, 252, 254)]
    for strand in (0, 1):
        got, want = _both(merges + beside, strand)
        for r, row in enumerate(merges + beside):
            out = want.ops[r, :len(row[0])].tolist()
            out = out[::-1] if strand == 1 else out
            gaps = [c for c, v in enumerate(out) if v > 2]
            assert gaps == list(range(gaps[0], gaps[0] + len(gaps)))                   # side by side in the end
            assert (out[gaps[0]:gaps[0] + 2] == [3, 4]) == (r >= len(merges))          # the 4-run stopped beside the 3-run
        assert want.passes.tolist()[:5] == [2] * 5
    W.check_device_flags()


def test_skipped_reads_are_not_looked_at():
    rng = np.random.default_rng(6)
    good = _site(rng, 12, [A_], 4, 1, "del")
    n, n_ref, n_query = len(good[0]), len(good[1]), len(good[2])
    ops, ops_len = C.rows([good[0], [9] * n, [200] * n, good[0], [0] * n], dtype=np.uint8)
    a, _ = C.rows([good[1]] * 5)
    b, _ = C.rows([good[2]] * 5)
    args = (ops, [n, 10 ** 6, -5, n, n], a, [n_ref, -3, 0, n_ref, 0], b, [n_query, 10 ** 6, -1, n_query, n_query], [0, -1, 7, 1, -2])
    want = L.left_align_ref(*args)
    got = W.left_align(_alignment(ops, args[1]), _dev(a), _i32(args[3]), _dev(b), _i32(args[5]), _i32(args[6]))
    _assert_equal(got, want)
    assert want.settled.tolist() == [1] * 5 and want.passes.tolist() == [1, 0, 0, 0, 0] and want.bad == 0
    W.check_device_flags()                                           # nothing is reported


def test_bad_pairs_stay_as_they_are_and_are_counted_once():
    rng = np.random.default_rng(7)
    ops, a, b = _site(rng, 12, [A_], 4, 1, "del")
    n, n_ref, n_query = len(ops), len(a), len(b)
    bad = [dict(ops=ops[:4] + [0] + ops[5:]), dict(ops=ops[:4] + [5] + ops[5:]), dict(ops=ops[:4] + [255] + ops[5:]), dict(ops_len=n + 4),
           dict(ops_len=-1), dict(ops_len=n - 1), dict(ops=ops[:-1] + [3]), dict(ops=ops[:-1] + [4]), dict(n_ref=n_ref + 1), dict(n_ref=n_ref - 1),
           dict(n_ref=n_ref + 3), dict(n_ref=-2), dict(query_len=n_query - 1), dict(query_len=n_query + 1), dict(query_len=n_query + 3),
           dict(query_len=-1), dict(strand=2), dict(strand=7)]
    rows = [dict(ops=ops, ops_len=n, n_ref=n_ref, query_len=n_query, strand=r & 1) for r in range(len(bad) + 4)]
    for r, change in enumerate(bad):
        rows[r + 2].update(change)                                   # good reads before, between and after
    ops_rows, _ = C.rows([r["ops"] + [1, 1] for r in rows], dtype=np.uint8)            # max_ops = n + 2, N = n_ref + 2, M = n_query + 2
    a_rows, _ = C.rows([a + [A_, A_]] * len(rows))
    b_rows, _ = C.rows([b + [A_, A_]] * len(rows))
    args = (ops_rows, [r["ops_len"] for r in rows], a_rows, [r["n_ref"] for r in rows], b_rows, [r["query_len"] for r in rows], [r["strand"] for r in rows])
    want = L.left_align_ref(*args)
    assert want.bad == len(bad) and want.settled.tolist() == [1, 1] + [-1] * len(bad) + [1, 1]
    assert want.passes.tolist() == [1, 0] + [0] * len(bad) + [1, 0]  # the row is written for strand 0: walked back to front it is settled
    W.check_device_flags()
    got = W.left_align(_alignment(ops_rows, args[1]), _dev(a_rows), _i32(args[3]), _dev(b_rows), _i32(args[5]), _i32(args[6]))
    _assert_equal(got, want)
    assert torch.equal(got.alignment.ops[2:-2], _dev(ops_rows)[2:-2])
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.left_align: %d pair\\(s\\) whose ops do not fit" % len(bad)):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once


def test_pairs_poisoned_by_pairwise_align_are_bad_pairs():
    rng = np.random.default_rng(8)
    ref = _filler(rng, 12) + [A_] * 6 + _filler(rng, 12)
    ref_rows, query = _i32([ref] * 3), _i32([ref[2:14] + ref[15:28]] * 3)
    ref_len, query_len = _i32([30, 31, 30]), _i32([25, 25, -1])      # pair 1: a reference length past its row; pair 2: a negative length
    W.check_device_flags()
    aln = W.pairwise_align(ref_rows, ref_len, query, query_len)
    with pytest.raises(RuntimeError, match="pairwise_align"):
        W.check_device_flags()
    assert aln.ops_len.cpu().tolist()[1:] == [0, 0]
    got = W.left_align(aln, ref_rows, ref_len, query, query_len, _i32([0, 0, 0]))
    want = L.left_align_ref(aln.ops.cpu().numpy(), aln.ops_len.cpu().numpy(), ref_rows.cpu().numpy(), [30, 31, 30], query.cpu().numpy(), [25, 25, -1], [0] * 3)
    _assert_equal(got, want)
    assert want.settled.tolist() == [1, -1, -1] and want.bad == 2
    assert got.alignment.score is aln.score and got.alignment.matches is aln.matches and got.alignment.length is aln.length
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.left_align: 2 pair"):
        W.check_device_flags()


def test_strided_rows_int64_labels_and_two_runs_bitwise_equal():
    rng = np.random.default_rng(9)
    rows = [_site(rng, 100 + 40 * r, [A_, C_][:1 + r % 2], 6, 1, "del" if r & 1 else "ins") for r in range(6)]
    strand = [0, 1, 1, 0, 1, 0]
    rows = [(o[::-1], a[::-1], b[::-1]) if s else (o, a, b) for (o, a, b), s in zip(rows, strand)]
    ops, ops_len, a, a_len, b, b_len = K.batch(rows)
    want = L.left_align_ref(ops, ops_len, a, a_len, b, b_len, strand)
    assert want.passes.tolist() == [1] * 6
    wide = lambda x, fill: _dev(np.concatenate([x, np.full((x.shape[0], 37), fill, dtype=x.dtype)], axis=1))      # noqa: E731
    ops_wide, a_wide, b_wide = wide(ops, 7), wide(a.astype(np.int64), 2), wide(b.astype(np.int64), 3)
    aln = W.PairwiseAlignment(None, None, None, None, None, ops_wide[:, :ops.shape[1]], _i32(ops_len))
    assert not aln.ops.is_contiguous()
    call = lambda: W.left_align(aln, a_wide[:, :a.shape[1]], torch.tensor(a_len.tolist(), device=DEV), b_wide[:, :b.shape[1]], _i32(b_len),      # noqa: E731
                                torch.tensor(strand, device=DEV))
    got, again = call(), call()
    _assert_equal(got, want)
    assert got.alignment.ops.is_contiguous() and int(ops_wide[:, ops.shape[1]:].min()) == 7
    for name in ("passes", "settled"):
        assert torch.equal(getattr(got, name), getattr(again, name))
    assert torch.equal(got.alignment.ops, again.alignment.ops)
    W.check_device_flags()


def test_captured_into_a_graph():
    rng = np.random.default_rng(10)
    rows = [_five_passes(rng, at) for at in (3, 254)] + [_site(rng, 300, [A_, C_], 20, 2, "del")]
    ops, ops_len, a, a_len, b, b_len = K.batch(rows)
    want = L.left_align_ref(ops, ops_len, a, a_len, b, b_len, [0, 0, 0])
    aln = _alignment(ops, ops_len)
    args = (_dev(a), _i32(a_len), _dev(b), _i32(b_len), _i32([0, 0, 0]))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        eager = W.left_align(aln, *args)                             # warms the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.left_align(aln, *args)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(captured, want)
    assert torch.equal(captured.alignment.ops, eager.alignment.ops) and want.passes.tolist() == [5, 5, 1]
    aln.ops.copy_(captured.alignment.ops)                            # the settled rows go in: the replay reads nothing back on the host
    graph.replay()
    torch.cuda.synchronize()
    assert captured.passes.cpu().tolist() == [0, 0, 0] and torch.equal(captured.alignment.ops, eager.alignment.ops)
    W.check_device_flags()


def test_rows_at_the_size_limits():
    """n_ref 65535 beside n_query 8192 with a run of 57343 columns, and a run of 8190: homopolymers, so that every column asks"""
    rows = [([1] * 100 + [3] * 57343 + [1] * 8092, [A_] * 65535, [A_] * 8192), ([1] * 2 + [3] * 8190 + [1] * 8190, [A_] * 16382, [A_] * 8192),
            ([1] * 8000 + [4] * 190 + [1, 1], [A_] * 8002, [A_] * 8192)]
    for strand in (0, 1):
        got, want = _both(rows, strand)
        assert want.passes.tolist() == [1, 1, 1] and want.settled.tolist() == [1, 1, 1]
        out = want.ops[0, :65535].tolist()
        assert (out[::-1] if strand else out)[:2] == [1, 3]
    W.check_device_flags()


# ---- the closed loop ------------------------------------------------------------------------------------------------------------

def _chain(run, left):
    labels, lengths = _dev(run["labels"]), _dev(run["lengths"])
    index = W.read_index(_i32(run["ref"]), k=11, w=5)
    m = W.map_reads(labels, lengths, index)
    assert m.strand.cpu().tolist() == run["strand"]
    lo, length = m.window(K.PLANT_FLANK)
    ref_rows, ref_len = m.labels(K.PLANT_FLANK)
    aln = W.pairwise_align(ref_rows, ref_len, labels, lengths)
    want = None
    if left:
        got = W.left_align(aln, ref_rows, ref_len, labels, lengths, m.strand)
        want = L.left_align_ref(aln.ops.cpu().numpy(), aln.ops_len.cpu().numpy(), ref_rows.cpu().numpy(), ref_len.cpu().tolist(),
                                labels.cpu().numpy(), lengths.cpu().tolist(), m.strand.cpu().tolist())
        _assert_equal(got, want)                                     # the reference fed with the GPU's own windows and ops
        assert W.quality_profile(got.alignment, ref_rows, ref_len, labels, lengths).read_counts.min() >= 0     # accepted as it stands
        aln = got.alignment
    pile = W.pileup(aln, lo, ref_len, m.strand, labels, lengths, index.R)
    calls = W.call_consensus(pile, index)
    return index, pile, calls, want, aln


@pytest.mark.parametrize("noisy", [False, True])
def test_closed_loop_on_the_repeat_planted_run(noisy):
    run = K.repeat_planted(noisy)
    index, pile, calls, want, _ = _chain(run, True)
    assert want.bad == 0 and want.settled.tolist() == [1] * K.PLANT_READS and 10 <= int((want.passes > 0).sum()) <= 30
    assert calls.consensus.cpu().tolist() == run["sample"]           # the committed seeds' condition (i)
    records = W.variant_records(index, calls, pile)
    assert [tuple(v)[:4] for v in records] == run["records"]
    lines = W.vcf_records("chr", index, calls, pile)
    assert [int(l.split("\t")[1]) for l in lines] == [r[0] + 1 for r in run["records"]]
    # without the left-alignment: what the host chain without it returns, which is not the planted records (condition (ii))
    index, pile, calls, _, _ = _chain(run, False)
    host = K.repeat_host(noisy, False)
    assert [tuple(v) for v in W.variant_records(index, calls, pile)] == host["variants"]
    assert calls.consensus.cpu().tolist() == [int(v) for v in host["calls"].consensus]
    assert [v[:4] for v in host["variants"]] != run["records"] and calls.consensus.cpu().tolist() != run["sample"]
    W.check_device_flags()


@pytest.mark.parametrize("noisy", [False, True])
def test_the_planted_runs_without_repeats_pass_unchanged(noisy):
    run, host = C.planted(noisy), C.planted_host(noisy)
    windows, n_ref = C.rows([C.window_labels(run["ref"], w[0], w[1], s) for w, s in zip(run["window"], run["strand"])])
    aln = _alignment(host["ops"], host["ops_len"])
    got = W.left_align(aln, _dev(windows), _i32(n_ref), _dev(run["labels"]), _dev(run["lengths"]), _i32(run["strand"]))
    assert torch.equal(got.alignment.ops, aln.ops) and got.passes.cpu().tolist() == [0] * C.PLANT_READS
    assert got.settled.cpu().tolist() == [1] * C.PLANT_READS
    W.check_device_flags()
