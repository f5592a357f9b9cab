"""CPU: the C ABI of the phasing step (csrc/wn_phase.hip): the exported symbols, the ctypes rows against the header argument by
argument, and every host-side rejection on both sides of every limit and in its documented order (shape, unsupported, NULL), with
fake pointers: every call below returns before anything would be launched.  And the host side of the Python surface: the
refusals, "no CPU fallback", S == 0, phased_records and vcf_phased_records on hand-made tensors."""
import numpy as np
import pytest
import torch

from tests.abi_util import FAKE, READ_ACCEPTED, READ_BATCH, READ_REQUIRED, READ_SHAPE, READ_UNSUPPORTED, WN_ERR_BAD_SHAPE, WN_ERR_UNSUPPORTED, \
    Entry, header_names, host_alignment
from tests.abi_util import hand_made_genotypes, lib  # noqa: F401

READS = dict(READ_BATCH, cap=None, flat_qual=20, gap_qual=20, min_qual=0, site_of=FAKE, alleles=FAKE, n_sites=40)
LINKS = Entry("wn_phase_links", dict(READS, reach=4, links=FAKE, observed=FAKE, used=FAKE, bad=None, stream=None))
TAG = Entry("wn_haplotag", dict(READS, pos=FAKE, root=FAKE, parity=FAKE, set_size=FAKE, hp=FAKE, ps=FAKE, weight=FAKE, n_observed=FAKE, bad=None,
                                stream=None))
CHAIN = Entry("wn_phase_chain", dict(links=FAKE, pos=FAKE, n_sites=40, reach=4, min_margin=1, parent=FAKE, flip=FAKE, margin=FAKE, root=FAKE,
                                     parity=FAKE, ps=FAKE, set_size=FAKE, work=FAKE, stream=None))
# what the sites add to the read batch: the qualities of wn_pileup_evidence, and a reference that holds n_sites positions
SITES_SHAPE = READ_SHAPE + (dict(flat_qual=-1), dict(gap_qual=-1), dict(n_sites=0), dict(n_sites=-1))
SITES_UNSUPPORTED = READ_UNSUPPORTED + (dict(reference_len=2 ** 26 + 1, n_sites=1), dict(flat_qual=94), dict(gap_qual=94), dict(n_sites=5001),
                                        dict(reference_len=39))
SITES_ACCEPTED = READ_ACCEPTED + (dict(reference_len=40), dict(reference_len=2 ** 26, n_sites=2 ** 26), dict(flat_qual=0), dict(flat_qual=93),
                                  dict(gap_qual=0), dict(gap_qual=93), dict(n_sites=1), dict(n_sites=5000), dict(cap=FAKE))
SITES_REQUIRED = READ_REQUIRED + ("site_of", "alleles")


def test_symbols_are_exported(lib):
    for entry in (LINKS, CHAIN, TAG):
        entry.check_exported(lib)


def test_signature_rows_match_the_header():
    for entry in (LINKS, CHAIN, TAG):                                # 29, 14 and 33 arguments
        entry.check_declared()
    assert header_names("wn_phase_links")[:16] == header_names("wn_pileup")[:16] == list(READ_BATCH)          # the same read arguments
    evidence = header_names("wn_pileup_evidence")
    assert list(LINKS.defaults)[:20] == [n for n in evidence[:21] if n != "weights_host"]    # and pileup_evidence's qualities


def test_phase_links_rejects_on_the_host_in_order(lib):
    LINKS.rejects(lib, "ops", shape=SITES_SHAPE + (dict(reach=0), dict(reach=-1)), unsupported=SITES_UNSUPPORTED + (dict(reach=9),),
                  accepted=SITES_ACCEPTED + (dict(reach=1), dict(reach=8)), required=SITES_REQUIRED + ("links", "observed", "used"))
    assert LINKS(lib, batch=0, reach=9, ops=None) == WN_ERR_BAD_SHAPE                           # the order: shape, unsupported, NULL
    assert LINKS(lib, reach=0, reference_len=2 ** 26 + 1) == WN_ERR_BAD_SHAPE
    assert LINKS(lib, reach=9, ops=None) == WN_ERR_UNSUPPORTED


def test_haplotag_rejects_on_the_host_in_order(lib):
    TAG.rejects(lib, "ops", shape=SITES_SHAPE, unsupported=SITES_UNSUPPORTED, accepted=SITES_ACCEPTED,
                required=SITES_REQUIRED + ("pos", "root", "parity", "set_size", "hp", "ps", "weight", "n_observed"))
    assert TAG(lib, n_sites=0, gap_qual=94, ops=None) == WN_ERR_BAD_SHAPE
    assert TAG(lib, n_sites=5001, ops=None) == WN_ERR_UNSUPPORTED


def test_phase_chain_rejects_on_the_host_in_order(lib):
    CHAIN.rejects(lib, "links", shape=(dict(n_sites=0), dict(n_sites=-1), dict(reach=0), dict(min_margin=-1)),
                  unsupported=(dict(n_sites=2 ** 26 + 1), dict(reach=9)),
                  accepted=(dict(n_sites=1), dict(n_sites=2 ** 26), dict(reach=1), dict(reach=8), dict(min_margin=0), dict(min_margin=2 ** 31 - 1)),
                  required=("links", "pos", "parent", "flip", "margin", "root", "parity", "ps", "set_size", "work"))
    assert CHAIN(lib, n_sites=0, reach=9, links=None) == WN_ERR_BAD_SHAPE
    assert CHAIN(lib, reach=9, links=None) == WN_ERR_UNSUPPORTED


def _host_sites(S=3, R=100):
    import wavenet_speech_amd as W
    site_of = torch.full((R,), -1, dtype=torch.int32)
    site_of[:S] = torch.arange(S, dtype=torch.int32)
    return W.PhaseSites(torch.arange(S, dtype=torch.int32), torch.ones(S, 2, dtype=torch.uint8), site_of)


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    sites = _host_sites()
    query, n = torch.ones(2, 30, dtype=torch.int32), [30, 30]
    args = dict(alignment=host_alignment(), lo=[0, 0], ref_lengths=[30, 30], strand=[0, 1], query=query, query_lengths=n, sites=sites)
    phasing = W.Phasing(*[torch.zeros(3, dtype=d) for d in (torch.int32, torch.uint8, torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32)])
    for fn, extra, what in ((W.phase_links, {}, "phase_links"), (W.haplotag, dict(phasing=phasing), "haplotag")):
        args_fn = dict(args, **extra)
        # the reads are refused in pileup's words, through pileup's own checks
        with pytest.raises(ValueError, match="wavenet_speech_amd.%s: alignment must be a PairwiseAlignment with ops" % what):
            fn(**dict(args_fn, alignment=W.PairwiseAlignment(None, None, None, None, None, None, None)))
        with pytest.raises(RuntimeError, match="wavenet_speech_amd.%s: alignment.ops must be a GPU tensor \\(there is no CPU fallback\\)" % what):
            fn(**args_fn)
        for kw in (dict(min_qual=-1), dict(min_qual=94), dict(flat_qual=-1), dict(flat_qual=94), dict(gap_qual=-1), dict(gap_qual=94), dict(gap_qual=True)):
            with pytest.raises(ValueError, match="wavenet_speech_amd.%s: %s must be an integer in" % (what, list(kw)[0])):
                fn(**dict(args_fn, **kw))
        with pytest.raises(ValueError, match="wavenet_speech_amd.%s: sites must be PhaseSites" % what):
            fn(**dict(args_fn, sites=sites.site_of))
    for reach in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match="wavenet_speech_amd.phase_links: reach must be an integer in"):
            W.phase_links(**dict(args, reach=reach))
    with pytest.raises(ValueError, match="wavenet_speech_amd.phase_sites: genotypes must be Genotypes"):
        W.phase_sites(torch.zeros(4, dtype=torch.uint8))
    g = W.Genotypes(torch.zeros(4, 2, dtype=torch.uint8), None, None, torch.zeros(4, dtype=torch.uint8), None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.phase_sites: genotypes.flags must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.phase_sites(g)
    links = W.PhaseLinks(torch.zeros(3, 4, 2, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int32), None)
    with pytest.raises(ValueError, match="wavenet_speech_amd.phase_chain: links must be a PhaseLinks"):
        W.phase_chain(links.links, sites)
    for m in (-1, 2 ** 31, 0.5):
        with pytest.raises(ValueError, match="wavenet_speech_amd.phase_chain: min_margin must be an integer in"):
            W.phase_chain(links, sites, min_margin=m)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.phase_chain: links.links must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.phase_chain(links, sites)


def _hand_made():
    """the case of tests/test_phase_ref.py::test_phased_records_by_hand as tensors"""
    import wavenet_speech_amd as W
    from tests.phase_cases import HAND_CHAIN
    ref, g, pile = hand_made_genotypes()
    site_of = torch.tensor([-1, 0, 1, 2, -1, 3, -1, 4], dtype=torch.int32)
    sites = W.PhaseSites(torch.tensor([1, 2, 3, 5, 7], dtype=torch.int32), g.alleles[[1, 2, 3, 5, 7]], site_of)
    dtypes = (torch.int32, torch.uint8, torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32)
    return ref, g, pile, sites, W.Phasing(*[torch.tensor(v, dtype=d) for v, d in zip(HAND_CHAIN, dtypes)])


def test_phased_and_vcf_records_on_hand_made_tensors():
    import wavenet_speech_amd as W
    ref, g, pile, sites, phasing = _hand_made()
    records = W.phased_records(ref, g, pile, sites, phasing)
    assert [tuple(v) for v in records] == [
        (0, "del", (1, 2), ((2,),), "1/1", 2, 1, 3, None), (0, "del", (1, 2, 3, 4), ((1,),), "1|0", 1002, 101, 4, 1),
        (2, "sub", (3,), ((1,), ()), "2|1", 2002, 201, 5, 1), (4, "sub", (1,), ((2,),), "1/1", 4002, 401, 7, None),
        (4, "del", (1, 2), ((1,),), "0/1", 5002, 501, 8, None), (4, "ins", (1,), ((1, 4, 1),), "0/1", 47, 45, 7, None),
        (5, "del", (2, 3), ((2,),), "1/1", 6002, 601, 9, None), (7, "sub", (4,), ((1,), (2,)), "1|2", 7002, 701, 10, 1)]
    plain = W.genotype_records(ref, g, pile)                         # the same records; a phased gt keeps its alleles, in haplotype order
    assert [tuple(v)[:4] + tuple(v)[5:8] for v in records] == [tuple(v)[:4] + tuple(v)[5:] for v in plain]
    assert [sorted(v.gt.replace("|", "/").split("/")) for v in records] == [v.gt.split("/") for v in plain]
    w = W.genotype_weights(100)
    assert W.vcf_phased_records("chr1", torch.tensor(ref), g, pile, sites, phasing, w) == [
        "chr1\t1\t.\tAG\tG\t0\tPASS\tDP=3\tGT:GQ:PS\t1/1:0:.\n", "chr1\t1\t.\tAGCT\tA\t10\tPASS\tDP=4\tGT:GQ:PS\t1|0:1:2\n",
        "chr1\t3\t.\tC\tA,*\t20\tPASS\tDP=5\tGT:GQ:PS\t2|1:2:2\n", "chr1\t5\t.\tA\tG\t40\tPASS\tDP=7\tGT:GQ:PS\t1/1:4:.\n",
        "chr1\t5\t.\tAG\tA\t50\tPASS\tDP=8\tGT:GQ:PS\t0/1:5:.\n", "chr1\t5\t.\tA\tATA\t0\tPASS\tDP=7\tGT:GQ:PS\t0/1:0:.\n",
        "chr1\t6\t.\tGC\tG\t60\tPASS\tDP=9\tGT:GQ:PS\t1/1:6:.\n", "chr1\t8\t.\tT\tA,G\t70\tPASS\tDP=10\tGT:GQ:PS\t1|2:7:2\n"]
    flipped = phasing._replace(parity=torch.tensor([0, 0, 1, 1, 1], dtype=torch.uint8))
    assert [v.gt for v in W.phased_records(ref, g, pile, sites, flipped)] == ["1/1", "0|1", "1|2", "1/1", "0/1", "0/1", "1/1", "2|1"]      # 1|2 beside `*`
    with pytest.raises(ValueError, match="wavenet_speech_amd.phased_records: sites must be PhaseSites and phasing a Phasing"):
        W.phased_records(ref, g, pile, sites, None)
    with pytest.raises(ValueError, match="wavenet_speech_amd.phased_records: genotypes must be Genotypes"):
        W.phased_records(ref, pile, pile, sites, phasing)
    with pytest.raises(ValueError, match="wavenet_speech_amd.phased_records: sites of 8 positions and a phasing of 4 sites"):
        W.phased_records(ref, g, pile, sites, W.Phasing(*[t[:4] for t in phasing]))
    with pytest.raises(ValueError, match="wavenet_speech_amd.vcf_phased_records: weights must be a GenotypeWeights"):
        W.vcf_phased_records("c", ref, g, pile, sites, phasing, 100)


def test_records_agree_with_the_reference_and_with_no_site_at_all():
    import wavenet_speech_amd as W
    from tests import phase_ref as H
    from tests.phase_cases import HAND_CHAIN, hand_calls
    ref, g, pile, sites, phasing = _hand_made()
    host_ref, calls, host_pile = hand_calls()
    assert np.array_equal(calls.flags, g.flags.numpy()) and np.array_equal(calls.alleles, g.alleles.numpy())
    want = H.phased_records_ref(host_ref, calls, host_pile, H.sites_ref(calls.flags, calls.alleles), HAND_CHAIN)
    assert [tuple(v) for v in W.phased_records(ref, g, pile, sites, phasing)] == want
    # S == 0: the records of genotype_records, every one unphased
    none = W.PhaseSites(torch.zeros(0, dtype=torch.int32), torch.zeros(0, 2, dtype=torch.uint8), torch.full((8,), -1, dtype=torch.int32))
    empty = W.Phasing(*[torch.zeros(0, dtype=t.dtype) for t in phasing])
    got = W.phased_records(ref, g, pile, none, empty)
    assert [tuple(v) for v in got] == [tuple(v) + (None,) for v in W.genotype_records(ref, g, pile)]
    assert all(line.endswith(":.\n") for line in W.vcf_phased_records("c", ref, g, pile, none, empty, W.genotype_weights()))
