"""GPU: pileup_evidence / call_genotypes (csrc/wn_genotype.hip) at their seam, size and batch limits, on the cases of
tests/call_limits_cases.py against the reference of tests/genotype_ref.py.  Every value is an integer: exact equality only.
tests/test_call_limits_ref.py (CPU) proves what each case reaches -- every wave and tile seam of the walk on both strands, tiles and
waves of op 3 or op 4 only, i = 65534 and j = 8191 over 288 tiles, 65535 reads with 7 bad and 5 skipped among them, 257 tiles of the
call kernel, and that a table of ones turns the evidence into the pileup's counts -- so nothing below can pass vacuously."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import call_limits_cases as K
from tests import genotype_ref as G
from tests import pileup_limits_cases as L
from tests import pileup_ref as P
from tests.gpu_calls import U, assert_evidence as _assert_evidence, assert_genotypes as _assert_calls, assert_pile as _assert_pile
from tests.gpu_calls import capture as _capture, copy_reads as _copy_reads, pile_rules as _pile_rules, reads_dev as _reads_dev
from tests.gpu_calls import rules_dev as _rules_dev, weights as _weights
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu


def _run(name, strand=None):
    """a case through the kernel; the table and `used` must equal the reference's exactly -> Evidence"""
    reads = K.reads_of(name, strand)
    got = W.pileup_evidence(*_reads_dev(reads), reads.R, _weights(K.TABLE), **_rules_dev(K.rules(name)))
    _assert_evidence(got, K.evidence(name, strand))
    return got


@pytest.mark.parametrize("strand", [0, 1])
def test_every_wave_and_tile_seam(strand):
    assert K.reads_of("grid").lo[:7].tolist() == [0, 1, 2, 3, 4, 0, 1]
    _run("grid", strand)
    W.check_device_flags()


@pytest.mark.parametrize("strand", [0, 1])
def test_whole_tiles_and_waves_of_one_op(strand):
    _run("whole", strand)
    W.check_device_flags()


def test_reads_at_the_size_limits():
    reads = K.reads_of("size")
    assert reads.ops.shape[1] == U.MAX_OPS and reads.query.shape[1] == U.MAX_PAIR_QUERY == K.quals("size").shape[1]
    _run("size")
    W.check_device_flags()


def test_a_batch_at_the_limit():
    W.check_device_flags()
    want = K.evidence("batch")
    got = _run("batch")
    assert int(got.evidence.sum()) == sum(v for p in want.evidence for c in p for v in c) > 0 and want.bad == len(L.BATCH_BAD) == 7
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup_evidence: %d pair\\(s\\) whose ops do not fit" % len(L.BATCH_BAD)):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once


@pytest.mark.parametrize("strand", [0, 1])
def test_unit_weights_reproduce_the_pileup_counts(strand):
    """a table of ones: every cell is pileup's count of the same batch over both strands, under the same quals and min_qual"""
    reads = K.reads_of("grid", strand)
    args, rules = _reads_dev(reads), _rules_dev(K.rules("grid"))
    pile = W.pileup(*args, reads.R, max_ins=reads.max_ins, **_pile_rules(rules))
    ones = W.pileup_evidence(*args, reads.R, _weights(K.UNIT, 1), **rules)
    assert torch.equal(ones.evidence, pile.counts[:, :, :5].sum(1).long()[:, :, None].expand(reads.R, 5, 3)) and torch.equal(ones.used, pile.used)
    assert int(ones.evidence.sum()) > 3 * 500000 and int(pile.counts[:, :, 5].sum()) > 50000      # the cells are full, and `other` took its share
    W.check_device_flags()


def test_call_genotypes_on_the_size_limit_pile():
    reads = K.reads_of("size")
    args, rules = _reads_dev(reads), _rules_dev(K.rules("size"))
    pile = W.pileup(*args, reads.R, max_ins=reads.max_ins, **_pile_rules(rules))
    _assert_pile(pile, K.size_pile())
    ev = W.pileup_evidence(*args, reads.R, _weights(K.TABLE), **rules)
    got = W.call_genotypes(pile, ev, _dev(K.size_reference()), _weights(K.TABLE), return_costs=True, **K.SIZE_CALL)
    assert tuple(got.flags.shape) == (L.SIZE_R,) and -(-L.SIZE_R // 256) == 257
    _assert_calls(got, K.size_calls())
    W.check_device_flags()


# ---- captured into a graph ------------------------------------------------------------------------------------------------------

def test_evidence_and_calls_captured_into_a_graph():
    """pileup_evidence(into=) and call_genotypes in one capture: the weight table travels by value, nothing is read back.  The pile is
    made outside and refreshed in place"""
    R = K.SMALL_R
    reference = np.random.default_rng(5).integers(0, 6, size=R)
    want = {}
    for seed in (1, 2):
        reads, qual, cap = K.small(seed)
        rules = K.small_rules(seed)
        pile = P.pileup_ref(*K.read_args(reads), R, max_ins=reads.max_ins, **_pile_rules(rules))
        ev = G.evidence_ref(K.TABLE, *K.read_args(reads), R, **rules)
        want[seed] = (ev, G.call_genotypes_ref(pile, ev.evidence, reference, K.TABLE, **K.SIZE_CALL))
    assert want[1][0].evidence != want[2][0].evidence and not np.array_equal(want[1][1].flags, want[2][1].flags)
    reads, qual, cap = K.small(1)
    args, rules = _reads_dev(reads), _rules_dev(K.small_rules(1))
    w, ref = _weights(K.TABLE), _i32(reference)
    pile = W.pileup(*args, R, max_ins=reads.max_ins, **_pile_rules(rules))
    table = W.Evidence(torch.zeros(R, 5, 3, dtype=torch.int64, device=DEV), None)

    def step():
        ev = W.pileup_evidence(*args, R, w, into=table, **rules)
        return ev, W.call_genotypes(pile, ev, ref, w, return_costs=True, **K.SIZE_CALL)

    graph, (ev, calls) = _capture(step)
    assert ev.evidence is table.evidence
    for seed in (1, 2):
        if seed == 2:                                                # other reads in the same tensors, and their pile
            _copy_reads(args, rules, *K.small(2))
            fresh = W.pileup(*args, R, max_ins=reads.max_ins, **_pile_rules(rules))
            for t, f in zip(pile[:3], fresh[:3]):
                t.copy_(f)
        table.evidence.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_evidence(ev, want[seed][0])
        _assert_calls(calls, want[seed][1])
    W.check_device_flags()
