"""CPU: the C ABI of the genotype evidence and the diploid calls (csrc/wn_genotype.hip): the exported symbols, the ctypes rows
against the header argument by argument, and every host-side rejection on both sides of every limit and in its documented order
(shape, unsupported, NULL, then the weights), with fake pointers: every call below returns before anything would be launched.  And
the host side of the Python surface: the refusals, "no CPU fallback", genotype_records and vcf_genotype_records on hand-made
tensors."""
import ctypes

import pytest
import torch

from tests.abi_util import FAKE, READ_ACCEPTED, READ_BATCH, READ_REQUIRED, READ_SHAPE, READ_UNSUPPORTED, WN_ERR_BAD_SHAPE, WN_ERR_NULL, \
    WN_ERR_UNSUPPORTED, Entry, header_names, host_alignment
from tests.abi_util import hand_made_genotypes as _hand_made, lib  # noqa: F401


def _table(fill=1, **at):
    t = (ctypes.c_int * (3 * 94))(*([fill] * (3 * 94)))
    for k, v in at.items():
        t[int(k[1:])] = v
    return t


GOOD = _table()
EVIDENCE = Entry("wn_pileup_evidence", dict(READ_BATCH, cap=None, weights_host=GOOD, flat_qual=20, gap_qual=20, min_qual=0, evidence=FAKE, used=FAKE,
                                            bad=None, stream=None))
CALL = Entry("wn_genotype_call", dict(evidence=FAKE, counts=FAKE, ins_lengths=FAKE, ins_bases=FAKE, reference=FAKE, reference_len=5000, max_ins=4,
                                      min_depth=3, alt_prior=3000, weights_host=GOOD, gap_qual=20, alleles=FAKE, gq=FAKE, qual=FAKE, flags=FAKE,
                                      ins_copies=FAKE, ins_len=FAKE, ins_out=FAKE, ins_gq=FAKE, ins_qual=FAKE, costs=None, stream=None))


def test_symbols_are_exported(lib):
    EVIDENCE.check_exported(lib)
    CALL.check_exported(lib)


def test_signature_rows_match_the_header():
    EVIDENCE.check_declared()                                        # 25 arguments
    CALL.check_declared()                                            # 22
    assert header_names("wn_pileup_evidence")[:16] == header_names("wn_pileup")[:16] == list(READ_BATCH)      # the same read arguments


def test_pileup_evidence_rejects_on_the_host_in_order(lib):
    EVIDENCE.rejects(lib, "ops", shape=READ_SHAPE + (dict(flat_qual=-1), dict(gap_qual=-1)),
                     unsupported=READ_UNSUPPORTED + (dict(flat_qual=94), dict(gap_qual=94)),
                     accepted=READ_ACCEPTED + (dict(reference_len=1), dict(flat_qual=0), dict(flat_qual=93), dict(gap_qual=0), dict(gap_qual=93),
                                               dict(cap=FAKE)),
                     required=READ_REQUIRED + ("weights_host", "evidence", "used"))
    # the weights are read last, once the table is known not to be NULL: both sides of [0, 2^20], first and last entry
    for kw in (dict(w0=-1), dict(w0=2 ** 20 + 1), dict(w281=-1), dict(w281=2 ** 20 + 1), dict(w94=2 ** 31 - 1)):
        assert EVIDENCE(lib, weights_host=_table(**kw)) == WN_ERR_UNSUPPORTED, kw
        assert EVIDENCE(lib, weights_host=_table(**kw), ops=None) == WN_ERR_NULL, kw
    for t in (_table(0), _table(2 ** 20), _table(w0=0, w281=2 ** 20)):
        assert EVIDENCE(lib, weights_host=t, ops=None) == WN_ERR_NULL                            # accepted: on to the NULL check
    assert EVIDENCE(lib, batch=0, gap_qual=94, ops=None) == WN_ERR_BAD_SHAPE                   # the order: shape, unsupported, NULL, weights
    assert EVIDENCE(lib, flat_qual=-1, reference_len=2 ** 26 + 1) == WN_ERR_BAD_SHAPE
    assert EVIDENCE(lib, flat_qual=94, ops=None, weights_host=_table(w0=-1)) == WN_ERR_UNSUPPORTED


def test_genotype_call_rejects_on_the_host_in_order(lib):
    CALL.rejects(lib, "evidence",
                 shape=(dict(reference_len=0), dict(reference_len=-1), dict(max_ins=-1), dict(min_depth=0), dict(gap_qual=-1)),
                 unsupported=(dict(reference_len=2 ** 26 + 1), dict(max_ins=9), dict(gap_qual=94), dict(alt_prior=-1), dict(alt_prior=2 ** 30 + 1)),
                 accepted=(dict(reference_len=1), dict(reference_len=2 ** 26), dict(max_ins=0), dict(max_ins=8), dict(min_depth=1),
                           dict(min_depth=2 ** 31 - 1), dict(gap_qual=0), dict(gap_qual=93), dict(alt_prior=0), dict(alt_prior=2 ** 30),
                           dict(costs=FAKE)),
                 required=("evidence", "counts", "ins_lengths", "ins_bases", "reference", "weights_host", "alleles", "gq", "qual", "flags",
                           "ins_copies", "ins_len", "ins_out", "ins_gq", "ins_qual"))
    assert CALL(lib, max_ins=0, ins_bases=None, ins_out=None, evidence=None) == WN_ERR_NULL
    for kw in (dict(w0=-1), dict(w0=2 ** 20 + 1), dict(w281=-1), dict(w281=2 ** 20 + 1)):
        assert CALL(lib, weights_host=_table(**kw)) == WN_ERR_UNSUPPORTED, kw
        assert CALL(lib, weights_host=_table(**kw), evidence=None) == WN_ERR_NULL, kw
    assert CALL(lib, weights_host=_table(2 ** 20), evidence=None) == WN_ERR_NULL
    assert CALL(lib, min_depth=0, max_ins=9, evidence=None) == WN_ERR_BAD_SHAPE
    assert CALL(lib, alt_prior=-1, evidence=None) == WN_ERR_UNSUPPORTED


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    w = W.genotype_weights()
    for scale in (0, 10700, 1.5, True):
        with pytest.raises(ValueError, match="wavenet_speech_amd.genotype_weights: scale must be an integer in"):
            W.genotype_weights(scale)
    query, n = torch.ones(2, 30, dtype=torch.int32), [30, 30]
    args = dict(alignment=host_alignment(), lo=[0, 0], ref_lengths=[30, 30], strand=[0, 1], query=query, query_lengths=n, R=100, weights=w)
    with pytest.raises(ValueError, match="wavenet_speech_amd.pileup_evidence: alignment must be a PairwiseAlignment with ops"):
        W.pileup_evidence(**dict(args, alignment=W.PairwiseAlignment(None, None, None, None, None, None, None)))
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup_evidence: alignment.ops must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.pileup_evidence(**args)
    for kw in (dict(R=0), dict(R=2 ** 26 + 1), dict(min_qual=-1), dict(min_qual=94), dict(flat_qual=-1), dict(flat_qual=94), dict(gap_qual=-1),
               dict(gap_qual=94), dict(gap_qual=True)):
        with pytest.raises(ValueError, match="wavenet_speech_amd.pileup_evidence: %s must be an integer in" % list(kw)[0]):
            W.pileup_evidence(**dict(args, **kw))
    bad_tables = (w._replace(table=w.table.long()), w._replace(table=w.table[:, :93]), w._replace(scale=0), w._replace(scale=2.0),
                  w._replace(table=w.table.clone().index_put_((torch.tensor(2), torch.tensor(93)), torch.tensor(2 ** 20 + 1, dtype=torch.int32))),
                  w._replace(table=-w.table))
    for t in bad_tables:
        with pytest.raises(ValueError, match="wavenet_speech_amd.pileup_evidence: (weights|every weight)"):
            W.pileup_evidence(**dict(args, weights=t))
    with pytest.raises(ValueError, match="wavenet_speech_amd.pileup_evidence: weights must be a GenotypeWeights"):
        W.pileup_evidence(**dict(args, weights=w.table))
    pile = W.Pileup(torch.zeros(6, 2, 6, dtype=torch.int32), torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6, 2, 4, dtype=torch.int32), None)
    ev = W.Evidence(torch.zeros(6, 5, 3, dtype=torch.int64), None)
    with pytest.raises(ValueError, match="wavenet_speech_amd.call_genotypes: pileup must be a Pileup and evidence an Evidence"):
        W.call_genotypes(pile, ev.evidence, [1] * 6, w)
    with pytest.raises(ValueError, match="wavenet_speech_amd.call_genotypes: weights must be a GenotypeWeights"):
        W.call_genotypes(pile, ev, [1] * 6, None)
    for kw in (dict(min_depth=0), dict(min_depth=2 ** 31), dict(gap_qual=-1), dict(gap_qual=94), dict(alt_prior=-1), dict(alt_prior=2 ** 30 + 1),
               dict(alt_prior=1.5)):
        with pytest.raises(ValueError, match="wavenet_speech_amd.call_genotypes: %s must be an integer in" % list(kw)[0]):
            W.call_genotypes(pile, ev, [1] * 6, w, **kw)
    with pytest.raises(ValueError, match="wavenet_speech_amd.call_genotypes: alt_prior must be an integer in"):
        W.call_genotypes(pile, ev, [1] * 6, w._replace(scale=2 ** 26))                          # 30 * scale is past 2^30
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.call_genotypes: pileup.counts must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.call_genotypes(pile, ev, [1] * 6, w)
    assert (W.Genotypes.HET, W.Genotypes.INS_HET, W.Genotypes.LOW_DEPTH, W.Genotypes.SUBSTITUTION, W.Genotypes.DELETION, W.Genotypes.INSERTION) == \
        (32, 64, 1, 4, 8, 16)


def test_genotype_and_vcf_records_on_hand_made_tensors():
    import wavenet_speech_amd as W
    ref, g, pile = _hand_made()
    assert [tuple(v) for v in W.genotype_records(ref, g, pile)] == [
        (0, "del", (1, 2), ((2,),), "1/1", 2, 1, 3),                 # a run at position 0: anchored on the next base
        (0, "del", (1, 2, 3, 4), ((1,),), "0/1", 1002, 101, 4),      # the run goes on, but its zygosity changed at 1
        (2, "sub", (3,), ((1,), ()), "1/2", 2002, 201, 5),           # A beside the deletion: the `*` allele
        (4, "sub", (1,), ((2,),), "1/1", 4002, 401, 7),
        (4, "del", (1, 2), ((1,),), "0/1", 5002, 501, 8),
        (4, "ins", (1,), ((1, 4, 1),), "0/1", 47, 45, 7),            # an insertion on a substituted site
        (5, "del", (2, 3), ((2,),), "1/1", 6002, 601, 9),
        (7, "sub", (4,), ((1,), (2,)), "1/2", 7002, 701, 10)]
    w = W.genotype_weights(100)
    assert W.vcf_genotype_records("chr1", torch.tensor(ref), g, pile, w) == [
        "chr1\t1\t.\tAG\tG\t0\tPASS\tDP=3\tGT:GQ\t1/1:0\n", "chr1\t1\t.\tAGCT\tA\t10\tPASS\tDP=4\tGT:GQ\t0/1:1\n",
        "chr1\t3\t.\tC\tA,*\t20\tPASS\tDP=5\tGT:GQ\t1/2:2\n", "chr1\t5\t.\tA\tG\t40\tPASS\tDP=7\tGT:GQ\t1/1:4\n",
        "chr1\t5\t.\tAG\tA\t50\tPASS\tDP=8\tGT:GQ\t0/1:5\n", "chr1\t5\t.\tA\tATA\t0\tPASS\tDP=7\tGT:GQ\t0/1:0\n",
        "chr1\t6\t.\tGC\tG\t60\tPASS\tDP=9\tGT:GQ\t1/1:6\n", "chr1\t8\t.\tT\tA,G\t70\tPASS\tDP=10\tGT:GQ\t1/2:7\n"]
    loud = g._replace(gq=torch.full((8,), 2 ** 31 - 1, dtype=torch.int32))
    assert all(line.endswith(":99\n") for line in W.vcf_genotype_records("c", ref, loud, pile, w) if "ATA" not in line)
    quiet = g._replace(flags=torch.tensor([0, W.Genotypes.LOW_DEPTH, W.Genotypes.HET, 0, 0, 0, 0, 0], dtype=torch.uint8))
    assert W.genotype_records(ref, quiet, pile) == [] and W.vcf_genotype_records("c", ref, quiet, pile, w) == []
    whole = g._replace(flags=torch.full((8,), W.Genotypes.DELETION, dtype=torch.uint8), alleles=torch.zeros(8, 2, dtype=torch.uint8))
    assert W.vcf_genotype_records("c", [1, 2, 3, 4, 1, 2, 3, 7], whole, pile, w) == ["c\t1\t.\tAGCTAGCN\t<DEL>\t0\tPASS\tDP=3\tGT:GQ\t1/1:0\n"]
    with pytest.raises(ValueError, match="wavenet_speech_amd.genotype_records: reference must be a ReadIndex or integer labels of shape \\(8,\\)"):
        W.genotype_records(ref[:5], g, pile)
    with pytest.raises(ValueError, match="wavenet_speech_amd.genotype_records: genotypes must be Genotypes"):
        W.genotype_records(ref, pile, pile)
    with pytest.raises(ValueError, match="wavenet_speech_amd.vcf_genotype_records: weights must be a GenotypeWeights"):
        W.vcf_genotype_records("c", ref, g, pile, 100)


def test_records_agree_with_the_reference_on_the_hand_made_case():
    import numpy as np
    import wavenet_speech_amd as W
    from tests import genotype_ref as G
    from tests import pileup_ref as P
    ref, g, pile = _hand_made()
    calls = G.Calls(*[None if t is None else t.numpy().astype(np.int64) for t in g])
    host = P.Pile(pile.counts.numpy().astype(np.int64), pile.ins_lengths.numpy(), pile.ins_bases.numpy(), None, 0)
    assert [tuple(v) for v in W.genotype_records(ref, g, pile)] == G.records_ref(ref, calls, host)
