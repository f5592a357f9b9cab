"""GPU: detect_events (csrc/wn_eventdetect.hip), event_align (csrc/wn_eventalign.hip), read_index / seed_anchors / chain_anchors /
map_reads (csrc/wn_readmap.hip) and demux_scores / demultiplex (csrc/wn_demux.hip) at the window, halo and size limits their header
comments state, against tests/event_detect_ref.py, tests/event_align_ref.py, tests/readmap_ref.py and tests/demux_ref.py.
Everything these kernels write is an integer and every comparison is exact equality.  The inputs and their references are built
once in tests/tool_limits_cases.py; tests/test_tool_limits_ref.py asserts on the CPU that they reach what each test below names
(both corners of the trace window, the outermost halo sample on every kind of seam, bit 31 of a k-mer code, 64 hits at every
position of a tile, the 1024th predecessor)."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import event_align_ref as EAR
from tests import event_detect_cases as ED
from tests import readmap_cases as RC
from tests import readmap_ref as RR
from tests import tool_limits_cases as C
from tests.gpu_labels import INT_MIN, PAD, assert_pick as _assert_pick, assert_scores as _assert_scores, kit as _kit, kw as _kw
from tests.gpu_signal import assert_detected as _assert_events, assert_event_alignment as _assert_alignment, assert_move_counts as _assert_counts
from tests.gpu_signal import detect_events as _detect, event_align as _align
from tests.gpu_util import DEV, dev as _dev, no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu


# ================================================================================================================ event alignment
@pytest.mark.parametrize("name", [n for n in C.EVENT_ALIGN if not n.startswith("largest")])
def test_steep_paths_through_the_trace_window(name):
    """d = 0..3 leading moves of 2 (or stays), then moves of 3: full chunks that end at every s_end mod 4, among them the two that
    read byte 0 of a window which does not start at byte 0 of the row -- with byte 48 (s_end = 0) and up to byte 47 (s_end = 3) --
    at E = 65..68, 129 and 193 (a last chunk of 1 to 4 events), bands 64 and 2048, alone and beside a short noisy read"""
    case, ref = C.event_align_case(name), C.event_align_reference(name)
    got = _align(case)
    _assert_alignment(got, ref)
    _assert_counts(got, case, ref)
    for b, want in enumerate(C.planted_moves(name)):
        if want is not None:
            assert got.moves[b].tolist() == want
    W.check_device_flags()


@pytest.mark.parametrize("name", list(C.LARGEST_MOVES))
def test_the_largest_and_the_most_negative_score(name):
    """256 events of 65536 samples, T_b = 2^24: 1.5 * 2^55 at the clamp and the largest offset, -2^54 at the most negative offset (a
    score, not the bad-read sentinel), move costs of 2^30 - 1; the read that ends at 2^24 + 1 is bad, counted and not aligned"""
    case, ref = C.event_align_case(name), C.event_align_reference(name)
    got = _align(case)
    _assert_alignment(got, ref)
    _assert_counts(got, case, ref)
    score = got.score.tolist()
    assert score[0] > 1 << 55 and EAR.BAD_READ < score[1] < -(1 << 53)
    assert score[3] == EAR.BAD_READ and got.states[3].eq(-1).all() and got.starts[3].eq(-1).all() and got.moves[3].eq(-1).all()
    with pytest.raises(RuntimeError, match="1 bad read"):
        W.check_device_flags()
    W.check_device_flags()


# ================================================================================================================ event detection
def test_the_widest_halo_across_every_kind_of_seam():
    """w_0 = w_1 = 16, r_0 = 64: position i is decided by the samples [i - 96, i + 95].  Pairs of reads that differ in the one
    sample i + 95, or i - 96, and in whether i is a boundary, with i the last position before and the first after the seam 256 at
    chunk 256 (workgroups), 768 at the automatic chunk of 768 and at 1024 (tiles inside a workgroup), 768 and 1536 at 16384; beside
    each pair the read altered one sample further out, which equals the plain one.  Every output equals the reference at every
    chunk, so the chunks agree"""
    case, ref = C.reach_case(), C.reach_reference()
    first = None
    for chunk in C.REACH_CHUNKS:
        got = _detect(case, chunk=chunk)
        _assert_events(got, ref)
        first = got if first is None else first
        assert all(torch.equal(u, v) for u, v in zip(got, first)), chunk
        dev = dict(n_events=got.n_events.cpu().numpy(), starts=got.starts.cpu().numpy(), kind=got.kind.cpu().numpy())
        for p, (side, seam, i, at, beyond) in enumerate(C.reach_pairs()):
            plain, altered, further = (ED.boundaries(dev, 3 * p + u) for u in range(3))
            assert ((i, 2) in plain) == (side == "left") and ((i, 2) in altered) == (side == "right") and further == plain, (chunk, side, i)
    W.check_device_flags()


def test_the_widest_halo_in_the_int16_form():
    sub, raw, ss, want, rows = C.reach_int16()
    for chunk in (256, None):
        _assert_events(_detect(sub, signal=_dev(raw), scale_shift=ss, chunk=chunk), want)
    W.check_device_flags()


@pytest.mark.parametrize("M", [32, 33])
def test_event_sums_at_the_lane_wave_hand_over(M):
    """max_event_len 32 (a lane sums every event) and 33 (the wave does), last events of 1, 31, 32 and 33 samples, samples of
    +-(2^23 - 1): the reference, and the closed forms n (2^23 - 1) and n (2^23 - 1)^2"""
    (case, lasts), ref = C.sums_case(M), C.sums_reference(M)
    got = _detect(case, chunk=None)
    _assert_events(got, ref)
    n = C.SUMS_EVENTS + 1
    for b in range(len(case.signal_lengths)):
        sign, lens = (1 if b < len(lasts) else -1), [M] * C.SUMS_EVENTS + [lasts[b % len(lasts)]]
        assert got.n_events[b].item() == n and got.length[b, :n].tolist() == lens
        assert got.sum[b, :n].tolist() == [sign * m * C.QMAX for m in lens] and got.sumsq[b, :n].tolist() == [m * C.QMAX * C.QMAX for m in lens]
    W.check_device_flags()


# =================================================================================================================== read mapping
def _assert_mapping(m, want, cap):
    """every field of a ReadMapping with want_pred, and of its anchors, against the reference's result dicts"""
    assert np.array_equal(torch.stack(list(m[:8]), dim=1).cpu().numpy(), RC.result_rows(want))
    a = m.anchors
    assert a.n_anchors.tolist() == [r["n_kept"] for r in want] and a.n_minimizers.tolist() == [r["n_minimizers"] for r in want]
    assert a.truncated.tolist() == [r["truncated"] for r in want] and tuple(a.keys.shape) == (len(want), cap)
    keys = a.keys.cpu().numpy()
    for b, r in enumerate(want):
        n = r["n_kept"]
        assert keys[b, :n].tolist() == r["keys"] and (keys[b, n:] == PAD).all()
        assert m.f[b, :n].tolist() == r["f"] and m.pred[b, :n].tolist() == r["pred"]
        assert m.f[b, n:].eq(INT_MIN).all() and m.pred[b, n:].eq(-1).all()


@pytest.mark.parametrize("w", C.K16_W)
def test_k16_codes_with_bit_31_through_index_seeds_and_chains(w):
    """k = 16: a quarter of the canonical codes do not fit 31 bits.  The index entries, the anchor keys and counts of eight reads
    with 4 % errors on both strands, and the result rows with f and pred, at w = 1 and w = 10"""
    ref, reads = C.k16()
    index = W.read_index(ref, k=16, w=w, device=DEV)
    host = C.k16_index(w)
    want_index = [(c << 28) | (p << 1) | s for c, p, s in host]
    assert index.n_entries == len(want_index) and index.entries[:index.n_entries].tolist() == want_index
    labels, lengths = RC.rows(reads)
    want = C.k16_results(w)
    cap = RR.DEFAULTS["anchors_per_read"]
    seeds = W.seed_anchors(_dev(labels), _dev(lengths), index)
    keys = seeds.keys.cpu().numpy()
    for b, r in enumerate(want):
        assert keys[b, :r["n_kept"]].tolist() == r["keys"] and (keys[b, r["n_kept"]:] == PAD).all()
    assert seeds.n_anchors.tolist() == [r["n_kept"] for r in want] and seeds.n_minimizers.tolist() == [r["n_minimizers"] for r in want]
    _assert_mapping(W.map_reads(_dev(labels), _dev(lengths), index, want_pred=True), want, cap)
    W.check_device_flags()


@pytest.mark.parametrize("cap", C.OCC_CAPS)
def test_the_longest_read_at_max_occ_64(cap):
    """k = w = 1, max_occ = 64, one code with 64 index entries and one with 65: reads of 65535 bases (64 hits at every position, 2^14
    a tile under the minimizer count of the packed scan, 65535 * 64 anchors in all; and one whose kept reverse-strand anchors reach
    q' = 65534 and 0), 65534 and 257 bases.  The kept prefix, sorted; n_anchors, truncated, n_minimizers; then the chains"""
    ref, reads = C.occ()
    index = W.read_index(ref, k=1, w=1, device=DEV)
    assert index.n_entries == 129 and index.entries[:129].tolist() == [(c << 28) | (p << 1) | s for c, p, s in C.occ_index()]
    labels, lengths = RC.rows([reads[n].tolist() for n in C.OCC_READS])
    want = C.occ_results(cap)
    got = W.seed_anchors(_dev(labels), _dev(lengths), index, max_occ=64, anchors_per_read=cap)
    keys = got.keys.cpu().numpy()
    for b, r in enumerate(want):
        n = r["n_anchors"]
        assert np.array_equal(keys[b, :n], np.array(r["keys"], dtype=np.int64)) and (keys[b, n:] == PAD).all(), C.OCC_READS[b]
    assert got.n_anchors.tolist() == [r["n_anchors"] for r in want] and got.truncated.tolist() == [r["truncated"] for r in want]
    assert got.n_minimizers.tolist() == [r["n_minimizers"] for r in want] == [65535, 65535, 65534, 257]
    m = W.chain_anchors(got, h=C.OCC_H[cap], want_pred=True)
    assert np.array_equal(torch.stack(list(m[:8]), dim=1).cpu().numpy(), RC.result_rows([r["chain"] for r in want]))
    for b, r in enumerate(want):
        n = r["n_anchors"]
        assert np.array_equal(m.f[b, :n].cpu().numpy(), np.array(r["chain"]["f"])) and np.array_equal(m.pred[b, :n].cpu().numpy(), np.array(r["chain"]["pred"]))
    W.check_device_flags()


@pytest.mark.parametrize("h", C.WINDOW_H)
def test_the_full_window_of_predecessors(h):
    """h = 1024 and 1000 over 1400 seeded anchors of one strand: the ring of 1024 wraps, all sixteen rounds of lanes are walked and
    best predecessors lie up to 1007 anchors back; f and pred of every anchor.  Beside them rows whose only predecessor sits 999 to
    1025 anchors back: reachable up to h and not beyond"""
    rows = [C.window_anchors()] + [C.reach_anchors(d) for d in C.WINDOW_REACH]
    want = [C.window_reference(h)] + [RR.chain_ref(sorted(r), 20000, C.WINDOW_K, h=h, **C.WINDOW_REACH_KW) for r in rows[1:]]
    for part, refs, kw in ((rows[:1], want[:1], C.WINDOW_KW), (rows[1:], want[1:], C.WINDOW_REACH_KW)):
        cap = max(len(r) for r in part)
        table = np.zeros((len(part), cap, 3), dtype=np.int64)
        for b, r in enumerate(part):
            table[b, :len(r)] = np.array(r, dtype=np.int64)
        anchors = W.Anchors.from_table(table, [len(r) for r in part], [20000] * len(part), C.WINDOW_K, device=DEV)
        got = W.chain_anchors(anchors, h=h, want_pred=True, **kw)
        assert np.array_equal(torch.stack(list(got[:8]), dim=1).cpu().numpy(), RC.result_rows(refs))
        for b, r in enumerate(refs):
            n = len(r["f"])
            assert got.f[b, :n].tolist() == r["f"] and got.pred[b, :n].tolist() == r["pred"], b
            assert got.f[b, n:].eq(INT_MIN).all() and got.pred[b, n:].eq(-1).all()
    assert [r["pred"][-1] for r in want[1:]] == [0 if d <= h else -1 for d in C.WINDOW_REACH]
    W.check_device_flags()


# ================================================================================================================= demultiplexing
def test_1024_patterns_and_picks_past_lane_63():
    """kDxMaxPatterns: 513 front and 511 rear patterns of 1 to 12 labels (nine and eight waves per read and end, the last front wave
    with one pattern), three reads; then the pick over nine rounds of the strided loop: equal best scores at the indices 70 and
    134 (two groups), 75 and 139 (one group), 3 and 67 (two groups), runner-up included, at three thresholds and with both ends
    required"""
    case, ref = C.demux_case(), C.demux_reference()
    kit, kw = _kit(case), _kw(case)
    labels, lengths = _dev(case.labels), _dev(case.lengths)
    _assert_scores(W.demux_scores(labels, lengths, kit, **kw), ref)
    for (num, den, margin), both in [(t, False) for t in C.DX_PICKS] + [(C.DX_PICKS[0], True)]:
        got = W.demultiplex(labels, lengths, kit, min_fraction=num / den, min_margin=margin, require_both=both, **kw)
        _assert_scores(got.scores, ref)
        _assert_pick(got, C.demux_pick_reference(num, den, margin, both))
    assert got.hits[:, 0, 0].tolist() == [lo for lo, _ in C.DX_PLANTS]
    W.check_device_flags()
