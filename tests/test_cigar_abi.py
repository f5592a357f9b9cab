"""CPU: the C ABI of the CIGAR encoder and decoder (csrc/wn_cigar.hip): the exported symbols, the ctypes rows against the header
argument by argument, the workspace query, and every host-side rejection on both sides of every limit and in its documented order
(shape, unsupported, NULL, workspace), with fake pointers: every call below returns before anything would be launched.  And the
refusals of the Python surface."""
import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry, host_alignment
from tests.abi_util import lib  # noqa: F401

MAX_OPS = 65535 + 8192
ENCODE = Entry("wn_cigar_encode", dict(ops=FAKE, ops_stride=900, ops_len=FAKE, lo=FAKE, ref_lengths=FAKE, strand=FAKE, query_lengths=FAKE, keep=None,
                                       batch=2, max_query_len=400, max_ops=900, reference_len=5000, eqx=1, max_cigar=803, cigar=FAKE,
                                       cigar_stride=803, n_cigar=FAKE, fields=FAKE, used=FAKE, bad=None, stream=None))
DECODE = Entry("wn_cigar_decode", dict(cigar=FAKE, cigar_stride=300, n_cigar=FAKE, pos=FAKE, strand=FAKE, reference=FAKE, reference_len=5000, query=FAKE,
                                       query_stride=400, query_lengths=FAKE, batch=2, max_cigar=300, max_query_len=400, max_ops=900, strict=0, ops=FAKE,
                                       ops_stride=900, ops_len=FAKE, ref_lengths=FAKE, stats=FAKE, used=FAKE, workspace=FAKE,
                                       workspace_bytes=lambda a: (a["batch"] * 3 * a["max_cigar"] * 4 + 15) // 16 * 16, bad=None, stream=None))
SHAPE = (dict(batch=0), dict(batch=-1), dict(max_query_len=0), dict(max_ops=0), dict(reference_len=0), dict(max_cigar=0), dict(max_cigar=-4),
         dict(ops_stride=-1), dict(cigar_stride=-1))
UNSUPPORTED = (dict(batch=65536), dict(max_query_len=8193), dict(max_ops=MAX_OPS + 1), dict(reference_len=2 ** 26 + 1), dict(max_cigar=65536))
ACCEPTED = (dict(batch=1), dict(batch=65535), dict(max_query_len=1), dict(max_query_len=8192), dict(max_ops=1), dict(max_ops=MAX_OPS),
            dict(reference_len=1), dict(reference_len=2 ** 26), dict(max_cigar=1), dict(max_cigar=65535), dict(ops_stride=0), dict(cigar_stride=0),
            dict(bad=FAKE))


def test_symbols_and_signature_rows(lib):
    ENCODE.check_exported(lib)
    DECODE.check_exported(lib)
    ENCODE.check_declared()                                          # 21 arguments
    DECODE.check_declared()                                          # 25 arguments
    Entry("wn_cigar_decode_workspace_bytes", dict(batch=2, max_cigar=300)).check_declared()


def test_workspace_query(lib):
    q = lib.wn_cigar_decode_workspace_bytes
    assert q(2, 300) == 2 * 3 * 300 * 4 and q(1, 1) == 16 and q(3, 5) == 192                      # three int32 per run, whole 16 bytes
    assert q(65535, 65535) == (65535 * 65535 * 12 + 15) // 16 * 16                                # no 32-bit product
    for bad in ((0, 300), (-1, 300), (2, 0), (2, -1), (65536, 300), (2, 65536)):
        assert q(*bad) == 0, bad


def test_encode_rejects_on_the_host_in_order(lib):
    ENCODE.rejects(lib, "ops", shape=SHAPE + (dict(eqx=2), dict(eqx=-1)), unsupported=UNSUPPORTED, accepted=ACCEPTED + (dict(eqx=0), dict(keep=FAKE)),
                   required=("ops", "ops_len", "lo", "ref_lengths", "strand", "query_lengths", "cigar", "n_cigar", "fields", "used"))
    assert ENCODE(lib, batch=0, max_cigar=65536, ops=None) == WN_ERR_BAD_SHAPE                  # the order: shape, unsupported, NULL
    assert ENCODE(lib, eqx=2, max_ops=MAX_OPS + 1) == WN_ERR_BAD_SHAPE
    assert ENCODE(lib, max_cigar=65536, cigar=None) == WN_ERR_UNSUPPORTED


def test_decode_rejects_on_the_host_in_order(lib):
    DECODE.rejects(lib, "cigar", shape=SHAPE + (dict(query_stride=-1), dict(strict=2), dict(strict=-1)), unsupported=UNSUPPORTED,
                   accepted=ACCEPTED + (dict(strict=1), dict(query_stride=0)),
                   required=("cigar", "n_cigar", "pos", "strand", "reference", "query", "query_lengths", "ops", "ops_len", "ref_lengths", "stats", "used",
                             "workspace"))
    assert DECODE(lib, batch=0, max_cigar=65536, cigar=None) == WN_ERR_BAD_SHAPE                # the order: shape, unsupported, NULL, workspace
    assert DECODE(lib, strict=2, reference_len=2 ** 26 + 1) == WN_ERR_BAD_SHAPE
    assert DECODE(lib, max_ops=MAX_OPS + 1, cigar=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert DECODE(lib, used=None, workspace_bytes=0) == WN_ERR_NULL
    assert DECODE(lib, workspace_bytes=2 * 3 * 300 * 4 - 1) == WN_ERR_WORKSPACE                # too small
    assert DECODE(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    import ctypes
    assert DECODE(lib, workspace=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE           # not 16-byte aligned


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    from wavenet_speech_amd import sam
    assert W.cigar_runs is sam.cigar_runs and W.cigar_ops is sam.cigar_ops and W.sam_records is sam.sam_records and W.parse_sam is sam.parse_sam
    assert W.CigarRows._fields == ("cigar", "n_cigar", "pos", "ref_span", "clip_front", "clip_back", "nm", "used", "eqx", "strand")
    assert W.CigarAlignment._fields == ("alignment", "lo", "ref_lengths", "used") and (sam.MAX_CIGAR, sam.CIGAR_CODES) == (65535, "MIDNSHP=X")
    args = dict(alignment=host_alignment(), lo=[0, 0], ref_lengths=[30, 30], strand=[0, 1], query_lengths=[30, 30], R=100)
    with pytest.raises(ValueError, match="wavenet_speech_amd.cigar_runs: alignment must be a PairwiseAlignment with ops"):
        W.cigar_runs(**dict(args, alignment=torch.ones(2, 30, dtype=torch.uint8)))
    for bad in (0, 2 ** 26 + 1, 2.0, None):
        with pytest.raises(ValueError, match="wavenet_speech_amd.cigar_runs: R must be an integer in"):
            W.cigar_runs(**dict(args, R=bad))
    with pytest.raises(ValueError, match="wavenet_speech_amd.cigar_runs: eqx must be True or False"):
        W.cigar_runs(**dict(args, eqx=1))
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.cigar_runs: alignment.ops must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.cigar_runs(**args)
    runs = dict(cigar=torch.zeros(2, 4, dtype=torch.int32), n_cigar=[1, 1], pos=[0, 0], strand=[0, 0], reference=[1, 2, 3, 4],
                query=torch.ones(2, 30, dtype=torch.int32), query_lengths=[30, 30])
    with pytest.raises(ValueError, match="wavenet_speech_amd.cigar_ops: strict must be True or False"):
        W.cigar_ops(**dict(runs, strict=0))
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.cigar_ops: query must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.cigar_ops(**runs)
