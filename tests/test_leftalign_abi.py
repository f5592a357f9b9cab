"""CPU: the C ABI of the indel left-alignment (csrc/wn_leftalign.hip): the exported symbol, the ctypes row against the header
argument by argument, and every host-side rejection on both sides of every limit and in its documented order (shape, unsupported,
NULL, aliasing), with fake pointers: every call below returns before anything would be launched.  And the refusals of the Python
surface."""
import ctypes

import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, Entry, host_alignment
from tests.abi_util import lib  # noqa: F401

OTHER = ctypes.c_void_p(2 << 20)         # a second fake pointer: ops_out must differ from ops_in
LEFT = Entry("wn_gap_left_align", dict(ops_in=FAKE, ops_stride=900, ops_len=FAKE, ref=FAKE, ref_stride=500, ref_lengths=FAKE, query=FAKE,
                                       query_stride=400, query_lengths=FAKE, strand=FAKE, batch=2, max_ref_len=500, max_query_len=400, max_ops=900,
                                       max_passes=8, ops_out=OTHER, out_stride=900, passes=FAKE, settled=FAKE, workspace=None, workspace_bytes=0,
                                       bad=None, stream=None))


def test_symbol_and_signature_row(lib):
    from wavenet_speech_amd import _lib
    LEFT.check_exported(lib)
    assert "wn_gap_left_align_workspace_bytes" not in _lib.SIGNATURES     # the passes run in place on ops_out: no workspace
    LEFT.check_declared()                                            # 23 arguments


def test_rejects_on_the_host_in_order(lib):
    LEFT.rejects(lib, "ops_in",
                 shape=(dict(batch=0), dict(batch=-1), dict(max_ref_len=0), dict(max_query_len=0), dict(max_ops=0), dict(max_passes=0),
                        dict(max_passes=-3), dict(ops_stride=-1), dict(ref_stride=-1), dict(query_stride=-1), dict(out_stride=-1)),
                 unsupported=(dict(batch=65536), dict(max_query_len=8193), dict(max_ref_len=65536), dict(max_ops=65535 + 8192 + 1), dict(max_passes=65)),
                 accepted=(dict(batch=1), dict(batch=65535), dict(max_query_len=1), dict(max_query_len=8192), dict(max_ref_len=1),
                           dict(max_ref_len=65535), dict(max_ops=1), dict(max_ops=65535 + 8192), dict(max_passes=1), dict(max_passes=64),
                           dict(ops_stride=0), dict(out_stride=0), dict(ref_stride=0), dict(query_stride=0), dict(bad=FAKE),
                           dict(workspace=FAKE, workspace_bytes=4096)),
                 required=("ops_in", "ops_len", "ref", "ref_lengths", "query", "query_lengths", "strand", "ops_out", "passes", "settled"))
    assert LEFT(lib, ops_out=FAKE) == WN_ERR_UNSUPPORTED             # ops_out == ops_in: the input stays as it is
    assert LEFT(lib, batch=0, max_passes=65, ops_in=None) == WN_ERR_BAD_SHAPE        # the order: shape, unsupported, NULL, aliasing
    assert LEFT(lib, out_stride=-1, max_ops=65535 + 8192 + 1) == WN_ERR_BAD_SHAPE
    assert LEFT(lib, max_passes=65, ops_in=None) == WN_ERR_UNSUPPORTED
    assert LEFT(lib, ops_out=FAKE, passes=None) == WN_ERR_NULL


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    from wavenet_speech_amd import leftalign
    assert W.left_align is leftalign.left_align and W.LeftAligned is leftalign.LeftAligned
    assert W.LeftAligned._fields == ("alignment", "passes", "settled") and (leftalign.MAX_OPS, leftalign.MAX_PASSES) == (65535 + 8192, 64)
    rows, n = torch.ones(2, 30, dtype=torch.int32), [30, 30]
    args = dict(alignment=host_alignment(), ref=rows, ref_lengths=n, query=rows, query_lengths=n, strand=[0, 1])
    with pytest.raises(ValueError, match="wavenet_speech_amd.left_align: alignment must be a PairwiseAlignment with ops"):
        W.left_align(**dict(args, alignment=W.PairwiseAlignment(None, None, None, None, None, None, None)))
    with pytest.raises(ValueError, match="wavenet_speech_amd.left_align: alignment must be a PairwiseAlignment with ops"):
        W.left_align(**dict(args, alignment=torch.ones(2, 30, dtype=torch.uint8)))
    for bad in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="wavenet_speech_amd.left_align: max_passes must be an integer in"):
            W.left_align(**dict(args, max_passes=bad))
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.left_align: alignment.ops must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.left_align(**args)
