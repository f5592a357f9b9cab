"""GPU: phase_links / phase_chain / haplotag (csrc/wn_phase.hip) at their ring, seam, size and batch limits, on the cases of
tests/call_limits_cases.py against the reference of tests/phase_ref.py.  Every value is an integer: exact equality only.
tests/test_call_limits_ref.py (CPU) proves what each case reaches -- rows whose observations lap the 512-entry ring of
phase_links_kernel twice, look-backs of every length across the wrap into both cells of every distance, tiles of exactly 256
observations, runs of deletions and insertions on the wrap, every wave and tile seam of the walk, reads of 65535 observations (128
laps), 65535 reads that link -- and that the linear reference used for the long reads equals the quadratic definition wherever
that is affordable, so nothing below can pass vacuously."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import call_limits_cases as K
from tests import phase_ref as H
from tests import pileup_limits_cases as L
from tests.gpu_calls import U, assert_chain as _assert_chain, assert_counts as _assert_counts, assert_links as _assert_links, assert_tags as _assert_tags
from tests.gpu_calls import capture as _capture, chain_dev as _chain_dev, copy_reads as _copy_reads, pile_rules as _pile_rules
from tests.gpu_calls import reads_dev as _reads_dev, rules_dev as _rules_dev, sites_dev as _sites_dev, tags_both as _tags_both
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu


def _run(name, strand=None, kind="dense", reach=K.REACH, near=True, pile=False):
    """a case through the kernel; links, observed and `used` must equal the reference's exactly -> (PhaseLinks, reference Links)
    and, with pile=True, the Pileup of the same reads beside them"""
    reads = K.reads_of(name, strand)
    sites = K.pairs_sites() if name == "pairs" else K.sites_of(kind, reads.R)
    want = K.links(name, strand, kind, reach, near)
    args, rules = _reads_dev(reads), _rules_dev(K.rules(name))
    got = W.phase_links(*args, _sites_dev(sites), reach=reach, **rules)
    _assert_links(got, want)
    if pile:
        return got, want, W.pileup(*args, reads.R, max_ins=reads.max_ins, **_pile_rules(rules))
    return got, want


# ---- the ring ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("reach", [1, 8])
def test_observations_that_lap_the_ring(reach, strand):
    """against links_ref, the quadratic definition: dense sites, where the partner d sites back is d entries back, then every third
    position and a fifth of the positions, where the site distance is not the position distance"""
    got, want, pile = _run("ring", strand, "dense", reach, near=False, pile=True)
    assert torch.equal(got.used, pile.used)
    _assert_counts(want.observed, K.sites_of("dense", K.ring().R), pile)
    for kind in ("every3", "sparse"):
        got, want = _run("ring", strand, kind, reach, near=False)
        _assert_counts(want.observed, K.sites_of(kind, K.ring().R), pile)
        assert sum(v for s in want.links for c in s for v in c) > 0
    W.check_device_flags()


@pytest.mark.parametrize("strand", [0, 1])
def test_haplotags_of_reads_of_more_than_two_tiles_of_observations(strand):
    """the three walks of haplotag_kernel over the ring family, under the chain of the family's own links, with quals of three
    values only: the arg-max ties all the time"""
    reads = K.reads_of("ring", strand)
    want = _tags_both(K.sites_of("dense", reads.R), K.ring_chain(strand), K.read_args(reads), qual=K.few_quals("ring"), gap_qual=10)
    assert want.hp == K.ring_tags(strand).hp and want.weight == K.ring_tags(strand).weight       # the tags whose conditions the CPU file holds


# ---- seams, whole tiles, the size and batch limits --------------------------------------------------------------------------------

@pytest.mark.parametrize("strand", [0, 1])
def test_every_wave_and_tile_seam(strand):
    got, want, pile = _run("grid", strand, pile=True)
    assert torch.equal(got.used, pile.used) and want.used.tolist() == [1] * len(want.used)
    _assert_counts(want.observed, K.sites_of("dense", L.grid().R), pile)
    W.check_device_flags()


@pytest.mark.parametrize("strand", [0, 1])
def test_whole_tiles_and_waves_of_one_op(strand):
    for kind in ("dense", "every3"):
        _run("whole", strand, kind)
    W.check_device_flags()


def test_reads_at_the_size_limits():
    reads = K.reads_of("size")
    assert reads.ops.shape[1] == U.MAX_OPS and reads.query.shape[1] == U.MAX_PAIR_QUERY and reads.R == L.SIZE_R
    got, want = _run("size")
    assert max(sum(o) for o in want.observed) == 4
    W.check_device_flags()


def test_haplotags_of_reads_at_the_size_limits():
    reads = K.reads_of("size")
    want = _tags_both(K.sites_of("dense", reads.R), K.hand_chain("dense", reads.R), K.read_args(reads), **K.rules("size"))
    assert want.hp == K.size_tags().hp and want.n_sites == K.size_tags().n_sites


def test_a_batch_at_the_limit():
    W.check_device_flags()
    reads, sites = K.pairs(), K.pairs_sites()
    got, want = _run("pairs", reach=1)
    refused = "wavenet_speech_amd.%%s: %d pair\\(s\\) whose ops do not fit" % len(L.BATCH_BAD)
    with pytest.raises(RuntimeError, match=refused % "phase_links"):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once
    rules = _rules_dev(K.rules("pairs"))
    pile = W.pileup(*_reads_dev(reads), reads.R, max_ins=reads.max_ins, **_pile_rules(rules))
    with pytest.raises(RuntimeError, match=refused % "pileup"):
        W.check_device_flags()
    assert torch.equal(got.used, pile.used) and want.bad == 7 and (got.used == -1).sum().item() == 7 and (got.used == 0).sum().item() == 5
    _assert_counts(want.observed, sites, pile)
    assert min(v for s in want.links[1:] for c in s for v in c) > 10000
    chain = H.chain_ref(want.links, sites.pos)
    tags = _tags_both(sites, chain, K.read_args(reads), report=len(L.BATCH_BAD), **K.rules("pairs"))
    assert chain.set_size == [3, 3, 3] and set(tags.hp) == {0, 1, 2} and all(tags.hp[b] == 0 and tags.ps[b] == -1 for b in L.BATCH_BAD + L.BATCH_SKIPPED)


# ---- strided rows and int64 labels ------------------------------------------------------------------------------------------------

def test_strided_rows_and_int64_labels():
    """the wide() construction of tests/test_gpu_genotype.py::test_strided_rows_and_int64_labels on phase_links and haplotag: rows
    that are views into wider tensors, labels, lengths and strands as int64"""
    reads, qual, cap = K.small(1)
    sites = K.sites_of("dense", K.SMALL_R)
    rules = K.small_rules(1)
    want = H.links_ref(sites, *K.read_args(reads), reach=K.REACH, **rules)
    chain = H.chain_ref(want.links, sites.pos)
    want_tags = H.haplotag_ref(sites, chain, *K.read_args(reads), **rules)
    assert max(chain.set_size) > 8 and set(want_tags.hp) >= {1, 2}
    sites_dev, chain_dev, dev_rules = _sites_dev(sites), _chain_dev(chain), _rules_dev(rules)
    plain = _reads_dev(reads)
    wide = lambda a, fill: _dev(np.concatenate([a, np.full((a.shape[0], 37), fill, dtype=a.dtype)], axis=1))    # noqa: E731
    n = reads.ops.shape[1]
    ops_wide, q_wide, qual_wide = wide(reads.ops, 7), wide(reads.query.astype(np.int64), 2), wide(qual, 200)
    aln = W.PairwiseAlignment(None, None, None, None, None, ops_wide[:, :n], _i32(reads.ops_len))
    strided = (aln, _i32(reads.lo), _i32(reads.n_ref), torch.tensor(reads.strand.tolist(), device=DEV), q_wide[:, :n],
               torch.tensor(reads.query_len.tolist(), device=DEV))
    strided_rules = dict(dev_rules, qual=qual_wide[:, :n + 5])
    assert strided[3].dtype == strided[4].dtype == strided[5].dtype == torch.int64 and not strided[4].is_contiguous() and not aln.ops.is_contiguous()
    links = [W.phase_links(*a, sites_dev, reach=K.REACH, **r) for a, r in ((plain, dev_rules), (strided, strided_rules))]
    for got in links:
        _assert_links(got, want)
    assert torch.equal(links[0].links, links[1].links) and torch.equal(links[0].observed, links[1].observed) and torch.equal(links[0].used, links[1].used)
    tags = [W.haplotag(*a, sites_dev, chain_dev, **r) for a, r in ((plain, dev_rules), (strided, strided_rules))]
    for got in tags:
        _assert_tags(got, want_tags)
    assert all(torch.equal(a, b) for a, b in zip(*tags))
    W.check_device_flags()


# ---- captured into a graph ------------------------------------------------------------------------------------------------------

def test_links_chain_and_tags_captured_into_a_graph():
    """phase_links(into=), phase_chain and haplotag in one capture over S = 257 sites given by hand (phase_sites reads S back and
    stays outside): 1 + 3 + 9 + 1 launches, the chain's nine jump rounds ping-pong in graph memory"""
    sites = K.sites_of("dense", K.SMALL_R)
    S = len(sites.pos)
    assert S == 257 and (S - 1).bit_length() == 9
    want = {}
    for seed in (1, 2):
        reads, rules = K.small(seed)[0], K.small_rules(seed)
        links = H.links_ref(sites, *K.read_args(reads), reach=K.REACH, **rules)
        chain = H.chain_ref(links.links, sites.pos)
        want[seed] = (links, chain, H.haplotag_ref(sites, chain, *K.read_args(reads), **rules))
    assert want[1][0].links != want[2][0].links and want[1][1].root != want[2][1].root and want[1][2].hp != want[2][2].hp
    args, rules, sites_dev = _reads_dev(K.small(1)[0]), _rules_dev(K.small_rules(1)), _sites_dev(sites)
    tables = W.PhaseLinks(torch.zeros(S, K.REACH, 2, dtype=torch.int64, device=DEV), torch.zeros(S, 3, dtype=torch.int32, device=DEV), None)

    def step():
        links = W.phase_links(*args, sites_dev, reach=K.REACH, into=tables, **rules)
        phasing = W.phase_chain(links, sites_dev)
        return links, phasing, W.haplotag(*args, sites_dev, phasing, **rules)

    graph, (links, phasing, tags) = _capture(step)
    assert links.links is tables.links and links.observed is tables.observed
    for seed in (1, 2):
        if seed == 2:
            _copy_reads(args, rules, *K.small(2))                    # other reads in the same tensors
        tables.links.zero_()
        tables.observed.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_links(links, want[seed][0])
        _assert_chain(phasing, want[seed][1])
        _assert_tags(tags, want[seed][2], "seed %d " % seed)
    W.check_device_flags()
