"""GPU: the four tools that walk an op row (pileup, pileup_evidence, left_align, quality_profile) judge one row alike, by the
definition of a valid op row in csrc/wn_opscan.h: the two pileups share its validating pass, left_align and
quality_profile keep a copy of it by hand.  One batch (tests/opwalk_cases.py: valid rows of 0 to 513 columns on
both strands, one row of every bad kind, the skipped kinds) goes through all four once; every expected value is a host
reference's, by exact equality, and tests/test_opwalk_ref.py holds the references to each other on the CPU."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import genotype_ref as G
from tests import opwalk_cases as K
from tests.gpu_util import dev as _dev

pytestmark = pytest.mark.gpu


def _report():
    """the message of the device-flag report that is due, raised once"""
    with pytest.raises(RuntimeError) as e:
        W.check_device_flags()
    W.check_device_flags()
    return str(e.value)


@pytest.fixture(scope="module")
def run():
    """every tool once on the batch -> {tool: (result, report)}"""
    t = K.batch()
    W.check_device_flags()
    aln = W.PairwiseAlignment(None, None, None, None, None, _dev(t.ops), _dev(t.ops_len))
    reads = (aln, _dev(t.lo), _dev(t.ref_len), _dev(t.strand), _dev(t.query), _dev(t.query_len), K.R)
    weights = W.genotype_weights()
    assert weights.table.tolist() == G.weights()
    out = {}
    out["pileup"] = (W.pileup(*reads, qual=_dev(t.qual), min_qual=K.MIN_QUAL, max_ins=K.MAX_INS), _report())
    out["pileup_evidence"] = (W.pileup_evidence(*reads, weights, qual=_dev(t.qual), min_qual=K.MIN_QUAL), _report())
    out["left_align"] = (W.left_align(aln, _dev(t.ref), _dev(t.ref_len), _dev(t.query), _dev(t.query_len), _dev(t.strand)), _report())
    out["quality_profile"] = (W.quality_profile(aln, _dev(t.ref), _dev(t.ref_len), _dev(t.query), _dev(t.query_len), qual=_dev(t.qual),
                                                classes=K.CLASSES), _report())
    return out


def test_the_two_pileups_and_left_align_mark_the_same_reads(run):
    pile, evidence, aligned = run["pileup"][0], run["pileup_evidence"][0], run["left_align"][0]
    want = K.references()
    used = pile.used.cpu()
    assert used.dtype == torch.int8 and torch.equal(used, evidence.used.cpu()) and used.tolist() == want[0].used.tolist() == want[1].used.tolist()
    settled, passes = aligned.settled.cpu(), aligned.passes.cpu()
    assert settled.tolist() == want[2].settled.tolist() and passes.tolist() == want[2].passes.tolist()
    assert torch.equal(settled == -1, used == -1) and (used == -1).nonzero().flatten().tolist() == K.rows_of(K.BAD, K.STRAND_ONLY)
    t = K.batch()
    skipped = torch.from_numpy((t.strand < 0) | (t.ref_len == 0))
    assert int(skipped.sum()) == 4 and bool(((used == 0) & (settled == 1) & (passes == 0))[skipped].all())


def test_quality_profile_refuses_the_same_rows_apart_from_the_strand(run):
    got, want, t = run["quality_profile"][0], K.references()[3], K.batch()
    counts = got.read_counts.cpu().numpy()
    assert np.array_equal(counts, want["read_counts"])
    on_strand_0 = np.flatnonzero(t.strand == 0)
    assert [int(b) for b in on_strand_0 if counts[b, 0] == -1] == K.rows_of(K.BAD)
    assert (counts[K.rows_of(K.STRAND_ONLY, K.SKIPPED)] >= 0).all()


def test_every_tool_counts_its_bad_rows_once(run):
    want = K.references()
    assert want[0].bad == want[1].bad == want[2].bad == 12 and want[3]["bad"] == 11
    for tool, n in (("pileup", 12), ("pileup_evidence", 12), ("left_align", 12)):
        assert run[tool][1].count("wavenet_speech_amd.%s: %d pair(s) whose ops do not fit: " % (tool, n)) == 1, run[tool][1]
    assert run["quality_profile"][1].count("wavenet_speech_amd.quality_profile: 11 pair(s) whose ops do not fit their labels") == 1


def test_a_refused_row_leaves_every_table_and_row_as_the_references_leave_them(run):
    pile, evidence, aligned, profile = (run[k][0] for k in ("pileup", "pileup_evidence", "left_align", "quality_profile"))
    want, t = K.references(), K.batch()
    for name in ("counts", "ins_lengths", "ins_bases"):
        assert np.array_equal(getattr(pile, name).cpu().numpy(), getattr(want[0], name)), name
    assert np.array_equal(evidence.evidence.cpu().numpy(), np.array(want[1].evidence, dtype=np.int64))
    out = aligned.alignment.ops.cpu().numpy()
    assert np.array_equal(out, want[2].ops)
    refused = K.rows_of(K.BAD, K.STRAND_ONLY, K.SKIPPED)
    assert np.array_equal(out[refused], t.ops[refused]) and not np.array_equal(out, t.ops)      # copied; and some valid row moved
    for name in ("q_counts", "confusion", "outcome", "ref_index"):
        assert np.array_equal(getattr(profile, name).cpu().numpy(), want[3][name]), name
    assert profile.dwell_counts is None
