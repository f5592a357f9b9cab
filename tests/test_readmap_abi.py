"""CPU: the C ABI of the read mapping (csrc/wn_readmap.hip): the exported symbols, the ctypes rows against the header argument by
argument, and every host-side rejection on both sides of every limit and in its documented order (shape, unsupported, NULL), with
fake pointers: every call below returns before anything would be launched.  And the host side of the Python surface: the refusals,
"no CPU fallback", the packing of Anchors.from_table, mapq() and paf_records on hand-made tensors."""
import math

import numpy as np
import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, Entry
from tests.abi_util import lib  # noqa: F401

MINIMIZERS = Entry("wn_minimizers", dict(labels=FAKE, labels_stride=400, lengths=FAKE, batch=2, max_len=400, k=15, w=10, chunk=0, code=FAKE,
                                         flag=FAKE, bad=None, stream=None))
SEEDS = Entry("wn_read_seeds", dict(code=FAKE, flag=FAKE, lengths=FAKE, index=FAKE, n_index=1000, batch=2, max_len=400, k=15, max_occ=8,
                                    anchors_per_read=4096, keys=FAKE, n_minimizers=FAKE, n_anchors=FAKE, truncated=FAKE, bad=None, stream=None))
CHAIN = Entry("wn_chain", dict(keys=FAKE, n_anchors=FAKE, lengths=FAKE, batch=2, max_len=400, anchors_per_read=4096, k=15, h=64, max_dist=5000,
                               bandwidth=500, gap_base=2, gap_log=8, result=FAKE, f=None, pred=None, bad=None, stream=None))
INT_MIN = -2 ** 31


def test_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for entry in (MINIMIZERS, SEEDS, CHAIN):
        entry.check_exported(lib)
    assert "wn_chain_workspace_bytes" not in _lib.SIGNATURES         # no workspace is needed: f and pred are outputs


def test_signature_rows_match_the_header():
    for entry in (MINIMIZERS, SEEDS, CHAIN):                         # 12, 16 and 17 arguments
        entry.check_declared()


def test_minimizers_rejects_on_the_host_in_order(lib):
    MINIMIZERS.rejects(lib, "labels", shape=(dict(batch=0), dict(batch=-1), dict(max_len=0), dict(labels_stride=-1), dict(chunk=-1)),
                       unsupported=(dict(batch=65536), dict(max_len=2 ** 26 + 1), dict(k=0), dict(k=17), dict(w=0), dict(w=65), dict(chunk=2049)),
                       accepted=(dict(batch=1), dict(batch=65535), dict(max_len=1), dict(max_len=2 ** 26), dict(k=1), dict(k=16), dict(w=1),
                                 dict(w=64), dict(chunk=0), dict(chunk=1), dict(chunk=2048), dict(labels_stride=0)),
                       required=("labels", "lengths", "code", "flag"))
    assert MINIMIZERS(lib, batch=0, k=17, labels=None) == WN_ERR_BAD_SHAPE          # the order: shape, then unsupported, then NULL
    assert MINIMIZERS(lib, chunk=-1, w=65, code=None) == WN_ERR_BAD_SHAPE
    assert MINIMIZERS(lib, k=17, labels=None) == WN_ERR_UNSUPPORTED


def test_read_seeds_rejects_on_the_host_in_order(lib):
    SEEDS.rejects(lib, "code", shape=(dict(batch=0), dict(batch=-1), dict(max_len=0), dict(n_index=-1)),
                  unsupported=(dict(batch=65536), dict(max_len=65536), dict(n_index=2 ** 26 + 1), dict(k=0), dict(k=17), dict(max_occ=0),
                               dict(max_occ=65), dict(anchors_per_read=0), dict(anchors_per_read=32769)),
                  accepted=(dict(batch=1), dict(batch=65535), dict(max_len=1), dict(max_len=65535), dict(n_index=0), dict(n_index=2 ** 26),
                            dict(k=1), dict(k=16), dict(max_occ=1), dict(max_occ=64), dict(anchors_per_read=1), dict(anchors_per_read=32768)),
                  required=("code", "flag", "lengths", "index", "keys", "n_minimizers", "n_anchors", "truncated"))
    assert SEEDS(lib, n_index=-1, max_occ=65, keys=None) == WN_ERR_BAD_SHAPE
    assert SEEDS(lib, max_occ=65, keys=None) == WN_ERR_UNSUPPORTED


def test_chain_rejects_on_the_host_in_order(lib):
    CHAIN.rejects(lib, "keys", shape=(dict(batch=0), dict(batch=-1), dict(max_len=0)),
                  unsupported=(dict(batch=65536), dict(max_len=65536), dict(anchors_per_read=0), dict(anchors_per_read=32769), dict(k=0), dict(k=17),
                               dict(h=0), dict(h=1025), dict(max_dist=0), dict(max_dist=2 ** 26 + 1), dict(bandwidth=0), dict(bandwidth=2 ** 26 + 1),
                               dict(gap_base=-1), dict(gap_base=1025), dict(gap_log=-1), dict(gap_log=1025)),
                  accepted=(dict(batch=1), dict(batch=65535), dict(max_len=1), dict(max_len=65535), dict(anchors_per_read=1),
                            dict(anchors_per_read=32768), dict(k=1), dict(k=16), dict(h=1), dict(h=1024), dict(max_dist=1), dict(max_dist=2 ** 26),
                            dict(bandwidth=1), dict(bandwidth=2 ** 26), dict(gap_base=0), dict(gap_base=1024), dict(gap_log=0), dict(gap_log=1024),
                            dict(f=FAKE, pred=FAKE)),
                  required=("keys", "n_anchors", "lengths", "result"))
    assert CHAIN(lib, f=FAKE) == WN_ERR_NULL and CHAIN(lib, pred=FAKE) == WN_ERR_NULL          # the table comes whole or not at all
    assert CHAIN(lib, batch=0, h=1025, keys=None) == WN_ERR_BAD_SHAPE
    assert CHAIN(lib, h=1025, keys=None) == WN_ERR_UNSUPPORTED


def test_anchors_from_table_packs_and_sorts():
    import wavenet_speech_amd as W
    rows = [[(1, 3, 0), (0, 9, 2), (0, 9, 1), (0, 0, 0)], [(0, 2 ** 26 - 1, 65535), (1, 0, 0), (0, 0, 0), (0, 0, 0)]]
    a = W.Anchors.from_table(rows, [3, 2], [40, 30], 4)
    pad = 2 ** 63 - 1
    assert a.keys.dtype == torch.int64 and a.keys.tolist() == [[(9 << 16) | 1, (9 << 16) | 2, (1 << 43) | (3 << 16), pad],
                                                               [(2 ** 26 - 1) * 65536 + 65535, 1 << 43, pad, pad]]
    assert a.strand.tolist() == [[0, 0, 1, -1], [0, 1, -1, -1]] and a.ref_pos.tolist() == [[9, 9, 3, -1], [2 ** 26 - 1, 0, -1, -1]]
    assert a.query_pos.tolist() == [[1, 2, 0, -1], [65535, 0, -1, -1]]
    assert a.n_anchors.tolist() == [3, 2] and a.lengths.tolist() == [40, 30] and (a.k, a.max_len, a.reference) == (4, 40, None)
    assert a.n_anchors.dtype == torch.int32 and a.truncated.tolist() == [0, 0]
    assert W.Anchors.from_table(np.zeros((1, 1, 3), dtype=np.int64), [0], [0], 1, max_len=7).max_len == 7
    for bad in (dict(rows=[[(2, 0, 0)]]), dict(rows=[[(0, 2 ** 26, 0)]]), dict(rows=[[(0, 0, 65536)]]), dict(rows=[[(0, -1, 0)]]),
                dict(rows=[[(0, 1, 1), (0, 1, 1)]], counts=[2]), dict(counts=[2]), dict(counts=[-1]), dict(k=0), dict(k=17), dict(rows=[[0, 0, 0]]),
                dict(lengths=[1, 2]), dict(max_len=65536), dict(rows=np.zeros((1, 1, 3)))):
        with pytest.raises(ValueError, match="wavenet_speech_amd.Anchors.from_table:"):
            W.Anchors.from_table(**dict(dict(rows=[[(0, 1, 1)]], counts=[1], lengths=[10], k=4), **bad))


def _mapping(rows, k=15, lengths=None, reference=None):
    import wavenet_speech_amd as W
    t = torch.tensor(rows, dtype=torch.int32)
    anchors = W.Anchors(None, None, None, None, torch.tensor(lengths or [1000] * len(rows), dtype=torch.int32), k, 1000, reference)
    return W.ReadMapping(*(t[:, i] for i in range(8)), None, None, anchors=anchors)


def test_mapq_and_views_on_hand_made_tensors():
    m = _mapping([[1600, 0, 100, 500, 0, 400, 20, 160], [1600, 1, 100, 500, 0, 400, 5, INT_MIN], [320, 0, 1, 40, 2, 30, 2, 320],
                  [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN], [1600, 0, 0, 9, 0, 9, 20, 1440]])
    want = [40 * 0.9 * 1.0 * math.log(100.0), 40 * 1.0 * 0.5 * math.log(100.0), 0.0, 0.0, 40 * 0.1 * math.log(100.0)]
    got = m.mapq()
    assert got.dtype == torch.float32 and [min(60.0, w) for w in want] == pytest.approx(got.tolist(), rel=1e-6)
    assert got.tolist()[0] == 60.0 and got.tolist()[2:4] == [0.0, 0.0] and 18.4 < got.tolist()[4] < 18.5
    assert m.mapped.tolist() == [True, True, True, False, True] and m.ref_span().tolist() == [[100, 500], [100, 500], [1, 40], [-1, -1], [0, 9]]
    with pytest.raises(ValueError, match="ReadMapping.labels: these anchors were not seeded"):
        m.labels()


def test_paf_records_on_hand_made_tensors():
    import wavenet_speech_amd as W
    m = _mapping([[1600, 0, 100, 500, 3, 400, 20, 160], [INT_MIN, -1, -1, -1, -1, -1, 0, INT_MIN], [1600, 1, 7, 300, 0, 310, 12, 1440]],
                 lengths=[420, 50, 333])
    lines = W.paf_records(["a", "b", "c"], [420, 50, 333], m, "chr1", ref_length=5000)
    # columns 10 and 11 without an alignment: min(n_anchors k, query span) and the longer span; the unmapped read has no line
    assert lines == ["a\t420\t3\t400\t+\tchr1\t5000\t100\t500\t300\t400\t60\n", "c\t333\t0\t310\t-\tchr1\t5000\t7\t300\t180\t310\t18\n"]
    aln = W.PairwiseAlignment(None, torch.tensor([380, 0, 290]), None, None, torch.tensor([410, 0, 320]), None, None)
    lines = W.paf_records(["a", "b", "c"], torch.tensor([420, 50, 333]), m, "chr1", alignment=aln, ref_length=5000)
    assert [l.split("\t")[9:11] for l in lines] == [["380", "410"], ["290", "320"]]
    m12 = _mapping([[1600, 0, 0, 50, 0, 40, 2, INT_MIN]], k=15)
    assert W.paf_records(["r"], [40], m12, "t", ref_length=60)[0].split("\t")[9:11] == ["30", "50"]
    for kw, msg in ((dict(ref_length=None), "ref_length is needed"), (dict(names=["a"]), "1 names"), (dict(mapping=None), "must be a ReadMapping"),
                    (dict(alignment=W.PairwiseAlignment(None, torch.zeros(2), None, None, torch.zeros(2), None, None)), "2 rows for 3 reads")):
        with pytest.raises(ValueError, match="wavenet_speech_amd.paf_records: .*" + msg):
            W.paf_records(**dict(dict(names=["a", "b", "c"], lengths=[420, 50, 333], mapping=m, ref_name="chr1", ref_length=5000), **kw))


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    labels, n = torch.ones(2, 30, dtype=torch.int32), [30, 12]
    for kw in (dict(k=0), dict(k=17), dict(w=0), dict(w=65), dict(k=1.5), dict(w=True), dict(chunk=0), dict(chunk=2049)):
        with pytest.raises(ValueError, match="wavenet_speech_amd.minimizers:"):
            W.minimizers(labels, n, **kw)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.minimizers: labels must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.minimizers(labels, n)
    for bases, kw in (([1.0, 2.0], {}), ([[1, 2]], {}), ([], {}), ([1, 2, 3], dict(k=17)), ([1, 2, 3], dict(w=0))):
        with pytest.raises(ValueError, match="wavenet_speech_amd.read_index:"):
            W.read_index(bases, **kw)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.read_index: the index must live on a GPU \\(there is no CPU fallback\\)"):
        W.read_index([1, 2, 3, 4], device="cpu")
    index = W.ReadIndex(torch.zeros(1, dtype=torch.int64), 0, torch.ones(50, dtype=torch.int32), 15, 10)
    assert (index.R, index.k, index.w, index.n_entries) == (50, 15, 10, 0)
    for fn in (W.seed_anchors, W.map_reads):
        name = fn.__name__
        for kw in (dict(max_occ=0), dict(max_occ=65), dict(anchors_per_read=0), dict(anchors_per_read=32769), dict(chunk=2049)):
            with pytest.raises(ValueError, match="wavenet_speech_amd.%s:" % name):
                fn(labels, n, index, **kw)
        with pytest.raises(ValueError, match="wavenet_speech_amd.%s: index must be a ReadIndex" % name):
            fn(labels, n, [1, 2, 3])
        with pytest.raises(RuntimeError, match="wavenet_speech_amd.%s: labels must be a GPU tensor \\(there is no CPU fallback\\)" % name):
            fn(labels, n, index)
    chain = (dict(h=0), dict(h=1025), dict(max_dist=0), dict(max_dist=2 ** 26 + 1), dict(bandwidth=0), dict(bandwidth=2 ** 26 + 1),
             dict(gap_base=-1), dict(gap_base=1025), dict(gap_log=-1), dict(gap_log=1025), dict(gap_log=0.5))
    anchors = W.Anchors.from_table([[(0, 1, 1)]], [1], [10], 4)
    for kw in chain:
        with pytest.raises(ValueError, match="wavenet_speech_amd.map_reads:"):
            W.map_reads(labels, n, index, **kw)
        with pytest.raises(ValueError, match="wavenet_speech_amd.chain_anchors:"):
            W.chain_anchors(anchors, **kw)
    with pytest.raises(ValueError, match="wavenet_speech_amd.chain_anchors: anchors must be Anchors"):
        W.chain_anchors(anchors.keys)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.chain_anchors: anchors.keys must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.chain_anchors(anchors)
