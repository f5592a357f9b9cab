"""CPU: the C ABI of the demultiplexing (csrc/wn_demux.hip): the exported symbols, the ctypes rows against the header argument by
argument, and every host-side rejection on both sides of every limit and in its documented order (shape, unsupported, NULL), with
fake pointers: every call below returns before anything would be launched.  And the host side of the Python surface: the pattern
table of a BarcodeSet, reverse_complement and trim_reads (torch ops, here on the CPU), the refusals, and "no CPU fallback"."""
import numpy as np
import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_UNSUPPORTED, Entry
from tests.abi_util import lib  # noqa: F401

SCORES = Entry("wn_demux_scores", dict(labels=FAKE, labels_stride=400, lengths=FAKE, patterns=FAKE, pattern_stride=40, pattern_lengths=FAKE, batch=2,
                                       max_len=400, n_patterns=24, n_front=12, max_pattern_len=40, window=150, match=6, mismatch=-12, gap_open=10,
                                       gap_extend=4, score=FAKE, start=FAKE, end=FAKE, bad=None, stream=None))
PICK = Entry("wn_demux_pick", dict(score=FAKE, start=FAKE, end=FAKE, lengths=FAKE, pattern_group=FAKE, min_score=FAKE, batch=2, n_patterns=24,
                                   n_front=12, min_margin=12, require_both=0, barcode=FAKE, trim=FAKE, hits=FAKE, runner_up=FAKE, stream=None))


def test_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    SCORES.check_exported(lib)
    PICK.check_exported(lib)
    assert "wn_demux_workspace_bytes" not in _lib.SIGNATURES         # no workspace is needed


def test_signature_rows_match_the_header():
    SCORES.check_declared()                                          # 21 arguments
    PICK.check_declared()                                            # 16


def test_scores_rejects_on_the_host_in_order(lib):
    SCORES.rejects(lib, "labels",
                   shape=(dict(batch=0), dict(batch=-1), dict(n_patterns=0), dict(n_front=-1), dict(n_front=25), dict(max_len=0),
                          dict(max_pattern_len=0), dict(window=0), dict(window=-3), dict(labels_stride=-1), dict(pattern_stride=-1)),
                   unsupported=(dict(batch=65536), dict(max_len=2 ** 24 + 1), dict(n_patterns=1025), dict(max_pattern_len=129), dict(window=513),
                                dict(gap_extend=-1), dict(gap_extend=11), dict(gap_open=1025, gap_extend=0), dict(match=1025), dict(match=-1025),
                                dict(mismatch=1025), dict(mismatch=-1025)),
                   accepted=(dict(batch=1), dict(batch=65535), dict(max_len=2 ** 24), dict(max_len=1), dict(n_patterns=1024), dict(n_patterns=12),
                             dict(n_front=0), dict(n_front=24), dict(max_pattern_len=128), dict(max_pattern_len=1), dict(window=512), dict(window=1),
                             dict(gap_extend=0), dict(gap_extend=10), dict(gap_open=1024, gap_extend=1024), dict(gap_open=0, gap_extend=0),
                             dict(match=1024), dict(match=-1024), dict(mismatch=1024), dict(mismatch=-1024), dict(labels_stride=0),
                             dict(pattern_stride=0)),
                   required=("labels", "lengths", "patterns", "pattern_lengths", "score", "start", "end"))
    # the order: shape, then unsupported, then NULL
    assert SCORES(lib, batch=0, window=513, labels=None) == WN_ERR_BAD_SHAPE
    assert SCORES(lib, n_front=1026, n_patterns=1025, score=None) == WN_ERR_BAD_SHAPE
    assert SCORES(lib, labels_stride=-1, match=2000, lengths=None) == WN_ERR_BAD_SHAPE
    assert SCORES(lib, window=513, labels=None) == WN_ERR_UNSUPPORTED
    assert SCORES(lib, gap_extend=11, end=None) == WN_ERR_UNSUPPORTED


def test_pick_rejects_on_the_host_in_order(lib):
    PICK.rejects(lib, "score", shape=(dict(batch=0), dict(batch=-1), dict(n_patterns=0), dict(n_front=-1), dict(n_front=25)),
                 unsupported=(dict(batch=65536), dict(n_patterns=1025), dict(min_margin=-1)),
                 accepted=(dict(batch=1), dict(batch=65535), dict(n_patterns=1024), dict(n_front=0), dict(n_front=24), dict(min_margin=0),
                           dict(min_margin=2 ** 31 - 1), dict(require_both=1)),
                 required=("score", "start", "end", "lengths", "pattern_group", "min_score", "barcode", "trim", "hits", "runner_up"))
    assert PICK(lib, batch=0, min_margin=-1, score=None) == WN_ERR_BAD_SHAPE
    assert PICK(lib, min_margin=-1, score=None) == WN_ERR_UNSUPPORTED


def test_barcode_set_builds_the_table():
    import wavenet_speech_amd as W
    kit = W.BarcodeSet(["AAGC", "TTG"], front_flank="GG", rear_flank="C", extra_front=["ACGTA"], extra_rear=["TT", "A"])
    # " AGCT": A 1, G 2, C 3, T 4.  front: GG + AAGC + C, GG + TTG + C, the adapter; rear: their reverse complements, then the adapters
    assert kit.patterns.tolist() == [[2, 2, 1, 1, 2, 3, 3], [2, 2, 4, 4, 2, 3, 0], [1, 3, 2, 4, 1, 0, 0],
                                     [2, 2, 3, 4, 4, 3, 3], [2, 3, 1, 1, 3, 3, 0], [4, 4, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0]]
    assert kit.pattern_lengths.tolist() == [7, 6, 5, 7, 6, 2, 1] and kit.pattern_end.tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert kit.pattern_group.tolist() == [0, 1, 2, 0, 1, 3, 4] and (kit.n_front, kit.n_patterns, kit.max_pattern_len) == (3, 7, 7)
    assert kit.group_names == ["barcode01", "barcode02", "front_adapter01", "rear_adapter01", "rear_adapter02"]
    assert kit.min_scores(0.6, 3) == [26, 22, 18, 26, 22, 8, 4]      # ceil(0.6 * 6 * P): 25.2, 21.6, 18, ., ., 7.2, 3.6
    assert kit.min_scores(0.5, 2.5) == [18, 15, 13, 18, 15, 5, 3]    # ceil(0.5 * 5 * P): 17.5, 15, 12.5, ., ., 5, 2.5
    # integer rows with lengths, names, the front only; adapters alone
    rows = W.BarcodeSet(np.array([[1, 2, 3, 0], [4, 4, 4, 4]]), lengths=[3, 4], names=["a", "b"], both_ends=False)
    assert rows.patterns.tolist() == [[1, 2, 3, 0], [4, 4, 4, 4]] and rows.n_front == 2 and rows.group_names == ["a", "b"]
    only = W.BarcodeSet(extra_front=["ACGT"], extra_rear=["ACGT"])
    assert only.pattern_group.tolist() == [0, 1] and only.n_front == 1 and only.group_names == ["front_adapter01", "rear_adapter01"]
    made = W.BarcodeSet.from_table([[1, 2], [3, 0], [4, 4]], [2, 1, 2], [1, 0, 1], [0, 0, 1])
    assert made.patterns.tolist() == [[3, 0], [1, 2], [4, 4]] and made.pattern_group.tolist() == [0, 0, 1] and made.n_front == 1
    for kw in (dict(barcodes=[]), dict(barcodes=["AXG"]), dict(barcodes=["A" * 129]), dict(barcodes=["A"], front_flank="G" * 128),
               dict(barcodes=["A"] * 513), dict(barcodes=["A", "G"], names=["x"]), dict(barcodes=[""]), dict(barcodes=[[1, 7]]),
               dict(barcodes=np.zeros((2, 3), dtype=np.int64), lengths=[1, 4])):
        with pytest.raises(ValueError, match="BarcodeSet"):
            W.BarcodeSet(**kw)
    assert W.BarcodeSet(["A"] * 512).n_patterns == 1024 and W.BarcodeSet(["A" * 128]).max_pattern_len == 128
    for args in (([[1, 2]], [3], [0], [0]), ([[1, 2]], [2], [2], [0]), ([[1, 2]], [2], [0], [-1]), ([[1, 2]], [0], [0], [0])):
        with pytest.raises(ValueError, match="BarcodeSet"):
            W.BarcodeSet.from_table(*args)


def test_reverse_complement_and_trim_reads_on_the_host():
    import wavenet_speech_amd as W
    labels = torch.tensor([[1, 2, 3, 4, 4, 0], [4, 1, 0, 0, 0, 0], [2, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    n = torch.tensor([5, 2, 6, 0])
    rc = W.reverse_complement(labels, n)
    assert rc.dtype == torch.int32 and rc.tolist() == [[1, 1, 2, 3, 4, 0], [4, 1, 0, 0, 0, 0], [3] * 6, [0] * 6]
    assert torch.equal(W.reverse_complement(rc, n), torch.where(torch.arange(6)[None] < n[:, None], labels, torch.zeros_like(labels)))
    assert W.reverse_complement(labels[:1], [3], complement=(0, 1, 2, 3, 4)).tolist() == [[3, 2, 1, 0, 0, 0]]
    qual = torch.arange(24, dtype=torch.uint8).reshape(4, 6)
    rows, new, q = W.trim_reads(labels, n, torch.tensor([[1, 4], [0, 2], [4, 2], [0, 0]]), qual=qual)
    assert rows.tolist() == [[2, 3, 4, 0, 0, 0], [4, 1, 0, 0, 0, 0], [0] * 6, [0] * 6] and new.tolist() == [3, 2, 0, 0] and new.dtype == torch.int32
    assert q.tolist() == [[1, 2, 3, 0, 0, 0], [6, 7, 0, 0, 0, 0], [0] * 6, [0] * 6] and q.dtype == torch.uint8
    rows, new = W.trim_reads(labels, n, torch.tensor([[-3, 99], [1, 99], [6, 6], [0, 5]]))                # clamped into [0, length]
    assert rows.tolist() == [[1, 2, 3, 4, 4, 0], [1, 0, 0, 0, 0, 0], [0] * 6, [0] * 6] and new.tolist() == [5, 1, 0, 0]
    for bad in (dict(trim=torch.zeros(4, 3)), dict(lengths=[1, 2]), dict(qual=qual[:, :5]), dict(labels=labels.float())):
        with pytest.raises(ValueError, match="trim_reads"):
            W.trim_reads(**dict(dict(labels=labels, lengths=n, trim=torch.zeros(4, 2, dtype=torch.int32)), **bad))
    with pytest.raises(ValueError, match="reverse_complement"):
        W.reverse_complement(labels, [1, 2])


def test_names():
    import wavenet_speech_amd as W
    d = W.Demultiplexed(torch.tensor([1, -1, 0, 2]), None, None, None, None)
    d.group_names = ["a", "b"]
    assert d.names() == ["b", "unclassified", "a", "2"]


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    kit = W.BarcodeSet(["AAGC", "TTGA"])
    labels, n = torch.ones(2, 30, dtype=torch.int32), [30, 12]
    for fn in (W.demux_scores, W.demultiplex):
        name = fn.__name__
        for kw in (dict(window=0), dict(window=513), dict(window=1.5), dict(match=0.25), dict(gap_extend=-0.5), dict(gap_open=1, gap_extend=2),
                   dict(gap_open=512.5), dict(match=513), dict(mismatch=-512.5)):
            with pytest.raises(ValueError, match="wavenet_speech_amd.%s:" % name):
                fn(labels, n, kit, **kw)
        with pytest.raises(ValueError, match="wavenet_speech_amd.%s: patterns must be a BarcodeSet" % name):
            fn(labels, n, kit.patterns)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(labels, n, kit)
    for kw in (dict(min_fraction=-0.1), dict(min_fraction=1.5), dict(min_fraction="a"), dict(min_margin=-1), dict(min_margin=0.25)):
        with pytest.raises(ValueError, match="wavenet_speech_amd.demultiplex:"):
            W.demultiplex(labels, n, kit, **kw)
