"""CPU: the C ABI of the pileup and the consensus calls (csrc/wn_pileup.hip): the exported symbols, the ctypes rows against the
header argument by argument, and every host-side rejection on both sides of every limit and in its documented order (shape,
unsupported, NULL), with fake pointers: every call below returns before anything would be launched.  And the host side of the
Python surface: the refusals, "no CPU fallback", ReadMapping.window, variant_records and vcf_records on hand-made tensors."""
import pytest
import torch

from tests.abi_util import FAKE, READ_ACCEPTED, READ_BATCH, READ_REQUIRED, READ_SHAPE, READ_UNSUPPORTED, WN_ERR_BAD_SHAPE, WN_ERR_NULL, \
    WN_ERR_UNSUPPORTED, Entry, host_alignment
from tests.abi_util import lib  # noqa: F401

PILEUP = Entry("wn_pileup", dict(READ_BATCH, min_qual=0, max_ins=4, counts=FAKE, ins_lengths=FAKE, ins_bases=FAKE, used=FAKE, bad=None, stream=None))
CALL = Entry("wn_consensus_call", dict(counts=FAKE, ins_lengths=FAKE, ins_bases=FAKE, reference=FAKE, reference_len=5000, max_ins=4, min_depth=3,
                                       num=1, den=2, call=FAKE, ins_len=FAKE, ins_out=FAKE, flags=FAKE, alt_count=FAKE, tile_offsets=FAKE,
                                       total=FAKE, stream=None))
EMIT = Entry("wn_consensus_emit", dict(call=FAKE, ins_len=FAKE, ins_out=FAKE, tile_offsets=FAKE, reference_len=5000, max_ins=4, capacity=5000,
                                       offsets=FAKE, consensus=FAKE, stream=None))


def test_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for entry in (PILEUP, CALL, EMIT):
        entry.check_exported(lib)
    assert "wn_pileup_workspace_bytes" not in _lib.SIGNATURES        # no workspace is needed


def test_signature_rows_match_the_header():
    for entry in (PILEUP, CALL, EMIT):                               # 24, 17 and 10 arguments
        entry.check_declared()


def test_pileup_rejects_on_the_host_in_order(lib):
    PILEUP.rejects(lib, "ops", shape=READ_SHAPE + (dict(max_ins=-1),), unsupported=READ_UNSUPPORTED + (dict(max_ins=9),),
                   accepted=READ_ACCEPTED + (dict(reference_len=1), dict(max_ins=0), dict(max_ins=8)),
                   required=READ_REQUIRED + ("counts", "ins_lengths", "ins_bases", "used"))
    assert PILEUP(lib, max_ins=0, ins_bases=None, ops=None) == WN_ERR_NULL          # reached the NULL check: no table is needed there
    assert PILEUP(lib, batch=0, max_ins=9, ops=None) == WN_ERR_BAD_SHAPE            # the order: shape, then unsupported, then NULL
    assert PILEUP(lib, min_qual=-1, reference_len=2 ** 26 + 1) == WN_ERR_BAD_SHAPE
    assert PILEUP(lib, max_ins=9, ops=None) == WN_ERR_UNSUPPORTED


def test_consensus_call_rejects_on_the_host_in_order(lib):
    CALL.rejects(lib, "counts",
                 shape=(dict(reference_len=0), dict(reference_len=-1), dict(max_ins=-1), dict(min_depth=0), dict(num=-1), dict(den=0)),
                 unsupported=(dict(reference_len=2 ** 26 + 1), dict(max_ins=9), dict(den=2 ** 15 + 1), dict(num=3, den=2)),
                 accepted=(dict(reference_len=1), dict(reference_len=2 ** 26), dict(max_ins=0), dict(max_ins=8), dict(min_depth=1),
                           dict(min_depth=2 ** 31 - 1), dict(num=0), dict(num=2, den=2), dict(den=1, num=1), dict(den=2 ** 15)),
                 required=("counts", "ins_lengths", "ins_bases", "reference", "call", "ins_len", "ins_out", "flags", "alt_count", "tile_offsets",
                           "total"))
    assert CALL(lib, max_ins=0, ins_bases=None, ins_out=None, counts=None) == WN_ERR_NULL
    assert CALL(lib, min_depth=0, max_ins=9, counts=None) == WN_ERR_BAD_SHAPE
    assert CALL(lib, max_ins=9, counts=None) == WN_ERR_UNSUPPORTED


def test_consensus_emit_rejects_on_the_host_in_order(lib):
    EMIT.rejects(lib, "call", shape=(dict(reference_len=0), dict(max_ins=-1), dict(capacity=-1)),
                 unsupported=(dict(reference_len=2 ** 26 + 1), dict(max_ins=9)),
                 accepted=(dict(reference_len=1), dict(reference_len=2 ** 26), dict(max_ins=0), dict(max_ins=8), dict(capacity=0),
                           dict(capacity=2 ** 31 - 1)),
                 required=("call", "ins_len", "ins_out", "tile_offsets", "offsets", "consensus"))
    assert EMIT(lib, max_ins=0, ins_out=None, capacity=0, consensus=None, call=None) == WN_ERR_NULL
    assert EMIT(lib, capacity=-1, max_ins=9, call=None) == WN_ERR_BAD_SHAPE
    assert EMIT(lib, max_ins=9, call=None) == WN_ERR_UNSUPPORTED


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    query, n = torch.ones(2, 30, dtype=torch.int32), [30, 30]
    args = dict(alignment=host_alignment(), lo=[0, 0], ref_lengths=[30, 30], strand=[0, 1], query=query, query_lengths=n, R=100)
    with pytest.raises(ValueError, match="wavenet_speech_amd.pileup: alignment must be a PairwiseAlignment with ops"):
        W.pileup(**dict(args, alignment=W.PairwiseAlignment(None, None, None, None, None, None, None)))
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup: alignment.ops must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.pileup(**args)
    for kw in (dict(R=0), dict(R=2 ** 26 + 1), dict(R=5.0), dict(min_qual=-1), dict(min_qual=94), dict(max_ins=-1), dict(max_ins=9), dict(max_ins=True)):
        with pytest.raises(ValueError, match="wavenet_speech_amd.pileup: %s must be an integer in" % list(kw)[0]):
            W.pileup(**dict(args, **kw))
    pile = W.Pileup(torch.zeros(6, 2, 6, dtype=torch.int32), torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6, 2, 4, dtype=torch.int32), None)
    assert (pile.R, pile.max_ins) == (6, 2) and pile.depth.tolist() == [0] * 6
    with pytest.raises(ValueError, match="wavenet_speech_amd.call_consensus: pileup must be a Pileup"):
        W.call_consensus(pile.counts, [1] * 6)
    for kw in (dict(min_depth=0), dict(min_depth=2 ** 31), dict(min_fraction=0.5), dict(min_fraction=(1, 0)), dict(min_fraction=(-1, 2)),
               dict(min_fraction=(3, 2)), dict(min_fraction=(1, 2 ** 15 + 1)), dict(min_fraction=(1, 2, 3))):
        with pytest.raises(ValueError, match="wavenet_speech_amd.call_consensus: min_"):
            W.call_consensus(pile, [1] * 6, **kw)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.call_consensus: pileup.counts must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.call_consensus(pile, [1] * 6)


def test_window_of_a_hand_made_mapping():
    import wavenet_speech_amd as W
    INT_MIN = -2 ** 31
    index = W.ReadIndex(torch.zeros(1, dtype=torch.int64), 0, torch.ones(500, dtype=torch.int32), 15, 10)
    t = torch.tensor([[1600, 0, 100, 400, 0, 300, 20, 160], [1600, 1, 3, 495, 0, 310, 12, 1440], [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN]],
                     dtype=torch.int32)
    anchors = W.Anchors(None, None, None, None, torch.tensor([300, 310, 50], dtype=torch.int32), 15, 1000, index)
    m = W.ReadMapping(*(t[:, i] for i in range(8)), None, None, anchors=anchors)
    for flank, lo, length in ((0, [100, 3, 0], [300, 492, 0]), (8, [92, 0, 0], [316, 500, 0]), (200, [0, 0, 0], [500, 500, 0])):
        got = m.window(flank)
        assert got[0].dtype == got[1].dtype == torch.int32 and got[0].tolist() == lo and got[1].tolist() == length
        assert m.labels(flank)[1].tolist() == length                 # the numbers labels() computes
    with pytest.raises(ValueError, match="wavenet_speech_amd.ReadMapping.window: flank"):
        m.window(-1)
    bare = W.ReadMapping(*(t[:, i] for i in range(8)), None, None, anchors=W.Anchors(None, None, None, None, None, 15, 1000, None))
    with pytest.raises(ValueError, match="ReadMapping.window: these anchors were not seeded"):
        bare.window()


def test_variant_and_vcf_records_on_hand_made_tensors():
    import wavenet_speech_amd as W
    U = W.ConsensusCalls
    ref = [1, 2, 3, 4, 1, 2]                                          # the case of tests/test_pileup_ref.py::test_emit_and_records_by_hand
    counts = torch.zeros(6, 2, 6, dtype=torch.int32)
    for p, k in enumerate((4, 4, 2, 0, 4, 1)):
        counts[p, p & 1, k] = 4
    ins_lengths, ins_bases = torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6, 2, 4, dtype=torch.int32)
    ins_lengths[2, 1], ins_bases[2, 0, 3], ins_bases[2, 1, 0] = 3, 3, 3
    pile = W.Pileup(counts, ins_lengths, ins_bases, None)
    u8 = lambda v: torch.tensor(v, dtype=torch.uint8)                # noqa: E731
    calls = W.ConsensusCalls(u8([0, 0, 3, 1, 0, 2]), u8([0, 0, 2, 0, 0, 0]), u8([[0, 0], [0, 0], [4, 1], [0, 0], [0, 0], [0, 0]]),
                             u8([U.DELETION, U.DELETION, U.INSERTION, U.SUBSTITUTION, U.DELETION, 0]),
                             torch.tensor([[4, 0], [0, 4], [4, 0], [0, 4], [4, 0], [0, 4]], dtype=torch.int32),
                             torch.tensor([0, 0, 0, 3, 4, 4, 5], dtype=torch.int32), torch.tensor([3, 4, 1, 1, 2], dtype=torch.int32))
    assert [tuple(v) for v in W.variant_records(ref, calls, pile)] == [
        (0, "del", (1, 2, 3), (3,), 4, 4, 4, 0), (2, "ins", (3,), (3, 4, 1), 4, 3, None, None), (3, "sub", (4,), (1,), 4, 4, 0, 4),
        (3, "del", (4, 1), (4,), 4, 4, 4, 0)]
    assert W.vcf_records("chr1", torch.tensor(ref), calls, pile) == [
        "chr1\t1\t.\tAGC\tC\t.\tPASS\tDP=4;AC=4;SF=4,0\n", "chr1\t3\t.\tC\tCTA\t.\tPASS\tDP=4;AC=3;SF=.,.\n",
        "chr1\t4\t.\tT\tA\t.\tPASS\tDP=4;AC=4;SF=0,4\n", "chr1\t4\t.\tTA\tT\t.\tPASS\tDP=4;AC=4;SF=4,0\n"]
    quiet = calls._replace(flags=u8([0, U.LOW_DEPTH, U.AMBIGUOUS, 0, 0, 0]))
    assert W.variant_records(ref, quiet, pile) == [] and W.vcf_records("c", ref, quiet, pile) == []
    whole = calls._replace(flags=u8([U.DELETION] * 6), call=u8([0] * 6))
    assert W.vcf_records("c", [1, 2, 3, 4, 1, 7], whole, pile) == ["c\t1\t.\tAGCTAN\t<DEL>\t.\tPASS\tDP=4;AC=4;SF=4,0\n"]
    with pytest.raises(ValueError, match="wavenet_speech_amd.variant_records: reference must be a ReadIndex or integer labels of shape \\(6,\\)"):
        W.variant_records(ref[:5], calls, pile)
    with pytest.raises(ValueError, match="wavenet_speech_amd.variant_records: calls must be ConsensusCalls"):
        W.variant_records(ref, pile, pile)
