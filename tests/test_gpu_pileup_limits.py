"""GPU: pileup / call_consensus / variant_records (csrc/wn_pileup.hip) at their seam, size and count limits, on the cases of
tests/pileup_limits_cases.py against the reference of tests/pileup_ref.py.  Every value is an integer: exact equality only.
tests/test_pileup_limits_ref.py (CPU) proves what each case reaches -- every wave and tile seam of the walk on both strands, tiles
and waves of op 4 only, i = 65534 and j = 8191 over 288 tiles, 65535 reads, two and three tile totals per thread of the scan,
products beside 2^46 whose 32-bit forms order differently -- so nothing below can pass vacuously."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import pileup_limits_cases as L
from tests import pileup_ref as P
from tests.gpu_calls import U, alignment as _alignment, assert_consensus as _assert_calls, assert_pile as _assert_pile, pile_dev as _to_device
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu
TOP = 2 ** 31 - 1


def _run(reads, want, into=None):
    """the reads through the kernel; the tables and `used` must equal the reference's exactly -> Pileup"""
    got = W.pileup(_alignment(reads.ops, reads.ops_len), _i32(reads.lo), _i32(reads.n_ref), _i32(reads.strand), _dev(reads.query),
                   _i32(reads.query_len), reads.R, max_ins=reads.max_ins, keep=None if reads.keep is None else torch.from_numpy(reads.keep).to(DEV),
                   into=into)
    _assert_pile(got, want)
    return got


@pytest.mark.parametrize("strand", [0, 1])
def test_every_wave_and_tile_seam(strand):
    _run(L.on_strand(L.grid(), strand), L.grid_pile(strand))
    W.check_device_flags()


@pytest.mark.parametrize("strand", [0, 1])
def test_whole_tiles_and_waves_of_one_op(strand):
    _run(L.on_strand(L.whole(), strand), L.whole_pile(strand))
    W.check_device_flags()


def test_reads_at_the_size_limits():
    reads = L.size()
    assert reads.ops.shape[1] == U.MAX_OPS and reads.query.shape[1] == U.MAX_PAIR_QUERY
    _run(reads, L.size_pile())
    W.check_device_flags()


def test_a_batch_at_the_limit():
    W.check_device_flags()
    want = L.batch_pile()
    got = _run(L.batch(), want)
    assert int(got.counts.sum()) == L.MAX_BATCH - len(L.BATCH_BAD) - len(L.BATCH_SKIPPED)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup: %d pair\\(s\\) whose ops do not fit" % len(L.BATCH_BAD)):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once


def test_counts_up_to_the_last_value_of_an_int32():
    """cells preset to 2^31 - 1 - n take n reads and read exactly 2^31 - 1; depth is summed in 64 bits"""
    n = 5
    reads = L.pack([[1, 4, 1]] * n, [[2, 3, 1]] * n, [3] * n, [0] * n, 2, R=6)
    tables = P.empty_pile(6, 2)
    cells = ((tables[0], (3, 0, 1)), (tables[0], (4, 0, 0)), (tables[1], (3, 0)), (tables[2], (3, 0, 2)))
    for t, cell in cells:
        t[cell] = TOP - n
    tables[0][3, 1, 2] = tables[0][3, 1, P.DEL] = TOP                # beside them: the depth of position 3 is 3 (2^31 - 1)
    start = P.Pile(*tables, None, 0)
    want = L.reference_pile(reads, into=start)
    got = _run(reads, want, into=_to_device(start))
    for t, cell in cells:
        assert t[cell] == TOP - n                                    # the reference copies; the kernel adds in place
    assert all(int(getattr(got, name)[cell]) == TOP for name, cell in (("counts", (3, 0, 1)), ("counts", (4, 0, 0)), ("ins_lengths", (3, 0)),
                                                                       ("ins_bases", (3, 0, 2))))
    depth = got.depth
    assert depth.dtype == torch.int64 and depth.cpu().tolist() == want.counts[:, :, :5].sum((1, 2)).tolist() and int(depth[3]) == 3 * TOP
    W.check_device_flags()


# ---- call_consensus -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", L.SCAN_R)
def test_scan_of_more_tile_totals_than_threads(R):
    rows, want = L.scan(R), L.scan_calls(R)
    got = W.call_consensus(_to_device(rows.pile), _dev(rows.ref), min_depth=L.SCAN_RULES["min_depth"],
                           min_fraction=(L.SCAN_RULES["num"], L.SCAN_RULES["den"]))
    _assert_calls(got, want)
    assert int(got.offsets[R]) == got.consensus.shape[0] == len(want.consensus)
    W.check_device_flags()


def test_calling_rules_beside_two_to_the_31():
    rows = L.count_rows()
    pile, ref = _to_device(rows.pile), _dev(rows.ref)
    assert int(pile.counts.max()) == rows.pile.counts.max() and int(pile.ins_lengths.max()) == TOP       # nothing was lost on the way
    for min_depth, num, den in L.COUNT_RULES:
        want = P.call_consensus_ref(rows.pile, rows.ref, min_depth, num, den)
        got = W.call_consensus(pile, ref, min_depth=min_depth, min_fraction=(num, den))
        _assert_calls(got, want)
    want = P.call_consensus_ref(rows.pile, rows.ref, 3, L.NUM, L.DEN)
    at = L.COUNT_NAMES.index
    assert want.flags[:4].tolist() == [P.AMBIGUOUS, P.SUBSTITUTION, 0, P.INSERTION] and want.alt_count[at("strand_split")].tolist() == list(L.SPLIT)
    W.check_device_flags()


def _vcf_line(name, v, alphabet=" AGCT"):
    text = lambda labels: "".join(alphabet[x] if 0 < x < len(alphabet) else "N" for x in labels)         # noqa: E731
    sf = ".,." if v[6] is None else "%d,%d" % (v[6], v[7])
    return "%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AC=%d;SF=%s\n" % (name, v[0] + 1, text(v[2]), text(v[3]) or "<DEL>", v[4], v[5], sf)


def test_records_of_every_kind_on_device_and_host_tensors():
    rows, want = L.variants(), L.variant_calls()
    pile = _to_device(rows.pile)
    calls = W.call_consensus(pile, _dev(rows.ref), min_depth=L.VARIANT_RULES["min_depth"], min_fraction=(L.VARIANT_RULES["num"], L.VARIANT_RULES["den"]))
    _assert_calls(calls, want)
    records = P.variants_ref(rows.ref, want, rows.pile)
    host_calls = W.ConsensusCalls(*(t.cpu() for t in calls))
    host_pile = W.Pileup(pile.counts.cpu(), pile.ins_lengths.cpu(), pile.ins_bases.cpu(), None)
    for c, p, ref in ((calls, pile, _dev(rows.ref)), (host_calls, host_pile, torch.from_numpy(rows.ref)), (calls, pile, rows.ref.tolist())):
        assert [tuple(v) for v in W.variant_records(ref, c, p)] == records
        assert W.vcf_records("chr", ref, c, p) == [_vcf_line("chr", v) for v in records]
    W.check_device_flags()


def test_emit_stops_at_its_capacity():
    """through the C ABI: the labels before `capacity` are written, no word at or past it, and offsets is whole every time"""
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    rows, want = L.variants(), L.variant_calls()
    R, max_ins, SENTINEL = L.VARIANT_R, L.VARIANT_MAX_INS, -77
    pile, ref = _to_device(rows.pile), _i32(rows.ref)
    lib = _lib.load()
    call, ins_len, flags = (torch.empty(R, dtype=torch.uint8, device=DEV) for _ in range(3))
    ins_out = torch.empty(R, max_ins, dtype=torch.uint8, device=DEV)
    alt_count = torch.empty(R, 2, dtype=torch.int32, device=DEV)
    tile_offsets = torch.empty((R + 255) // 256, dtype=torch.int32, device=DEV)
    total = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.check(lib.wn_consensus_call(_p(pile.counts), _p(pile.ins_lengths), _p(pile.ins_bases), _p(ref), R, max_ins, L.VARIANT_RULES["min_depth"],
                                     L.VARIANT_RULES["num"], L.VARIANT_RULES["den"], _p(call), _p(ins_len), _p(ins_out), _p(flags), _p(alt_count),
                                     _p(tile_offsets), _p(total), _stream()), "wn_consensus_call")
    n = int(total[0])
    assert n == len(want.consensus) and n > R                        # more labels than positions: insertions are emitted
    assert tile_offsets.cpu().tolist() == [0, int(want.offsets[256])]
    for capacity in (0, 1, n - 1, n, n + 5):
        out = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=DEV)
        offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        _lib.check(lib.wn_consensus_emit(_p(call), _p(ins_len), _p(ins_out), _p(tile_offsets), R, max_ins, capacity, _p(offsets),
                                         _p(out) if capacity else None, _stream()), "wn_consensus_emit")
        torch.cuda.synchronize()
        written = min(capacity, n)
        got = out.cpu().numpy()
        assert np.array_equal(got[:written], want.consensus[:written]), capacity
        assert (got[written:] == SENTINEL).all(), capacity
        assert np.array_equal(offsets.cpu().numpy()[:R], want.offsets[:R]) and int(offsets[R]) == SENTINEL, capacity       # [R] is the call's to write
    W.check_device_flags()
