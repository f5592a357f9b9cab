"""The drivers of the read-batch tools on the device (pileup, call_consensus, pileup_evidence, call_genotypes, phase_links,
phase_chain, haplotag): a batch of reads as device arguments, the same reads through the host reference and the
kernel, and the exact comparisons of every result class.  Used by tests/test_gpu_pileup.py, test_gpu_genotype.py,
test_gpu_phase.py, their *_limits files, test_gpu_leftalign.py and test_gpu_wave_steps.py; the host-side generators of reads are
in tests/pileup_cases.py.  Every value is an integer and every comparison exact equality; nothing here is rewritten by pytest, so
every assert carries its message."""
import sys

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import genotype_ref as G
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import pileup_ref as P
from tests.gpu_util import DEV, assert_equal_arrays, dev, i32, u8

TABLE = G.weights(100)
U = sys.modules["wavenet_speech_amd.pileup"]      # the module: the package exports the function under the same name


# ---- host tables and batches onto the device --------------------------------------------------------------------------------------

def alignment(ops_rows, ops_len):
    """a PairwiseAlignment that carries ops and ops_len only: all the read-batch tools look at"""
    return W.PairwiseAlignment(None, None, None, None, None, dev(ops_rows), i32(ops_len))


def host_rows(ops, query, qual, ops_len, query_len):
    """lists of op strings, labels and quals as zero-padded rows; a given ops_len / query_len replaces the true lengths
    -> (ops rows uint8, ops_len, query rows, query_len, qual rows uint8 or None)"""
    ops_rows, lens = C.rows(ops, dtype=np.uint8)
    q_rows, q_len = C.rows(query)
    qual_rows = None if qual is None else C.rows(qual, width=q_rows.shape[1], dtype=np.uint8)[0]
    return (ops_rows, lens if ops_len is None else np.asarray(ops_len, dtype=np.int32), q_rows,
            q_len if query_len is None else np.asarray(query_len, dtype=np.int32), qual_rows)


def reads_dev(reads):
    """a Reads as the leading arguments of pileup, pileup_evidence, phase_links and haplotag"""
    return (alignment(reads.ops, reads.ops_len), i32(reads.lo), i32(reads.n_ref), i32(reads.strand), dev(reads.query), i32(reads.query_len))


def rules_dev(rules):
    """the keyword arguments of call_limits_cases.rules() / small_rules() with their arrays on the device"""
    on = lambda v: None if v is None else dev(v)                     # noqa: E731
    return dict(rules, qual=on(rules["qual"]), cap=on(rules["cap"]), **({"keep": on(rules["keep"])} if "keep" in rules else {}))


def pile_rules(rules):
    """what pileup takes of them: it knows no cap and no gap_qual"""
    return {k: v for k, v in rules.items() if k in ("qual", "min_qual", "keep")}


def copy_reads(args, rules, reads, qual, cap):
    """another batch of the same shapes, written over the tensors the graph reads"""
    for t, a in zip((args[0].ops, args[0].ops_len) + args[1:], (reads.ops, reads.ops_len, reads.lo, reads.n_ref, reads.strand, reads.query, reads.query_len)):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    rules["qual"].copy_(torch.from_numpy(qual))
    rules["cap"].copy_(torch.from_numpy(cap))


def capture(step):
    """step() run once eagerly on a side stream (it warms the allocator there), then captured on it -> (graph, what the captured
    call returned)"""
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = step()
    return graph, captured


def pile_dev(pile):
    """a reference Pile as a Pileup on the device"""
    return W.Pileup(dev(pile.counts.astype(np.int32)), dev(pile.ins_lengths.astype(np.int32)), dev(pile.ins_bases.astype(np.int32)), None)


def weights(table=TABLE, scale=100):
    return W.GenotypeWeights(torch.tensor(table, dtype=torch.int32), scale)


def sites_dev(sites):
    return W.PhaseSites(i32(sites.pos), u8(np.asarray(sites.alleles, dtype=np.uint8).reshape(-1, 2)), i32(sites.site_of))


def chain_dev(chain):
    dtypes = (torch.int32, torch.uint8, torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32)
    return W.Phasing(*[torch.tensor(v, dtype=d, device=DEV) for v, d in zip(chain, dtypes)])


# ---- the exact comparisons ----------------------------------------------------------------------------------------------------------

def _dtypes(got, names, dtype):
    for name in names:
        assert getattr(got, name).dtype == dtype, "%s is %s, expected %s" % (name, getattr(got, name).dtype, dtype)


def assert_pile(got, want):
    _dtypes(got, ("counts", "ins_lengths", "ins_bases"), torch.int32)
    _dtypes(got, ("used",), torch.int8)
    assert_equal_arrays(got.used.cpu().numpy(), want.used, "used")
    for name in ("counts", "ins_lengths", "ins_bases"):
        assert_equal_arrays(getattr(got, name).cpu().numpy().astype(np.int64), getattr(want, name), name)


def assert_consensus(got, want):
    """a ConsensusCalls against the reference's calls"""
    _dtypes(got, ("call", "ins_len", "ins_bases", "flags"), torch.uint8)
    _dtypes(got, ("alt_count", "offsets", "consensus"), torch.int32)
    for name in ("call", "ins_len", "ins_bases", "flags", "alt_count", "offsets", "consensus"):
        assert_equal_arrays(getattr(got, name).cpu().numpy().astype(np.int64), getattr(want, name).astype(np.int64), name)


def assert_evidence(got, want):
    _dtypes(got, ("evidence",), torch.int64)
    _dtypes(got, ("used",), torch.int8)
    assert tuple(got.evidence.shape) == (len(want.evidence), 5, 3), "evidence has shape %s for %d positions" % (tuple(got.evidence.shape), len(want.evidence))
    assert_equal_arrays(got.used.cpu().numpy(), want.used, "used")
    assert_equal_arrays(got.evidence.cpu().numpy(), np.array(want.evidence, dtype=np.int64).reshape(-1, 5, 3), "evidence")


def assert_genotypes(got, want):
    """a Genotypes against the reference's Calls, the costs where they were asked for"""
    _dtypes(got, ("alleles", "flags", "ins_copies", "ins_len", "ins_bases"), torch.uint8)
    _dtypes(got, ("gq", "qual", "ins_gq", "ins_qual"), torch.int32)
    for name in ("alleles", "gq", "qual", "flags", "ins_copies", "ins_len", "ins_bases", "ins_gq", "ins_qual"):
        assert_equal_arrays(getattr(got, name).cpu().numpy().astype(np.int64), getattr(want, name).astype(np.int64), name)
    if got.costs is not None:
        _dtypes(got, ("costs",), torch.int64)
        assert got.costs.cpu().tolist() == want.costs, "costs: %s" % _first(got.costs.cpu().tolist(), want.costs)


def _first(got, want):
    """the first row at which two nested lists differ, with both rows"""
    if len(got) != len(want):
        return "%d rows, expected %d" % (len(got), len(want))
    at = next(n for n, (g, w) in enumerate(zip(got, want)) if g != w)
    return "first at row %d: %s, expected %s" % (at, got[at], want[at])


def _assert_lists(got, want, what):
    """exact equality of a tensor's nested list and the reference's"""
    assert got == want, "%s: %s" % (what, _first(got, want))


def assert_links(got, want):
    S = len(want.observed)
    _dtypes(got, ("links",), torch.int64)
    _dtypes(got, ("observed",), torch.int32)
    _dtypes(got, ("used",), torch.int8)
    shape = (S, len(want.links[0]) if S else got.links.shape[1], 2)
    assert tuple(got.links.shape) == shape and tuple(got.observed.shape) == (S, 3), \
        "links %s and observed %s, expected %s and %s" % (tuple(got.links.shape), tuple(got.observed.shape), shape, (S, 3))
    _assert_lists(got.used.cpu().tolist(), want.used.tolist(), "used")
    _assert_lists(got.observed.cpu().tolist(), want.observed, "observed")
    _assert_lists(got.links.cpu().tolist(), want.links, "links")


def assert_counts(observed, sites, pile):
    """observed[s] against the pileup's counts at pos[s] over both strands: label k is column k - 1, a deletion column 4"""
    counts = pile.counts.sum(1).cpu().tolist()
    for s, (p, (a0, a1)) in enumerate(zip(sites.pos, sites.alleles)):
        col = lambda label: 4 if label == 0 else label - 1           # noqa: E731
        assert observed[s][0] == counts[p][col(a0)] and observed[s][1] == counts[p][col(a1)], \
            "site %d at %d: observed %s, counts %s" % (s, p, observed[s], counts[p])
        assert sum(observed[s]) == sum(counts[p][:5]), "site %d at %d: observed %s, counts %s" % (s, p, observed[s], counts[p])


def assert_chain(got, want):
    for name in ("parent", "flip", "margin", "root", "parity", "ps", "set_size"):
        _dtypes(got, (name,), torch.uint8 if name in ("flip", "parity") else torch.int32)
        _assert_lists(getattr(got, name).cpu().tolist(), getattr(want, name), name)


def assert_tags(got, want, tag=""):
    """the four fields of a Haplotags against the reference's Tags"""
    for name in ("hp", "ps", "weight", "n_sites"):
        _assert_lists(getattr(got, name).cpu().tolist(), getattr(want, name), "%s%s" % (tag, name))


# ---- the same reads through the reference and the kernel ----------------------------------------------------------------------------

def pile_both(ops, lo, n_ref, strand, query, R, qual=None, keep=None, ops_len=None, query_len=None, into=None, **kw):
    """the tables and `used` must agree exactly -> (Pileup, Pile)"""
    ops_rows, ops_len, q_rows, q_len, qual_rows = host_rows(ops, query, qual, ops_len, query_len)
    want = P.pileup_ref(ops_rows, ops_len, lo, n_ref, strand, q_rows, q_len, R, qual=qual_rows, keep=keep, into=None if into is None else into[1], **kw)
    got = W.pileup(alignment(ops_rows, ops_len), i32(lo), i32(n_ref), i32(strand), dev(q_rows), i32(q_len), R,
                   qual=None if qual is None else dev(qual_rows), keep=None if keep is None else torch.tensor(keep, device=DEV),
                   into=None if into is None else into[0], **kw)
    assert_pile(got, want)
    return got, want


def evidence_both(ops, lo, n_ref, strand, query, R, table=TABLE, qual=None, keep=None, cap=None, ops_len=None, query_len=None, into=None, pile=False, **kw):
    """the table and `used` must agree exactly -> (Evidence, reference Evidence) and, with pile=True, the Pileup of the same batch
    beside them"""
    ops_rows, ops_len, q_rows, q_len, qual_rows = host_rows(ops, query, qual, ops_len, query_len)
    want = G.evidence_ref(table, ops_rows, ops_len, lo, n_ref, strand, q_rows, q_len, R, qual=qual_rows, keep=keep, cap=cap,
                          into=None if into is None else into[1].evidence, **kw)
    args = (alignment(ops_rows, ops_len), i32(lo), i32(n_ref), i32(strand), dev(q_rows), i32(q_len), R)
    common = dict(qual=None if qual is None else dev(qual_rows), keep=None if keep is None else torch.tensor(keep, device=DEV))
    got = W.pileup_evidence(*args, weights(table), cap=None if cap is None else dev(np.asarray(cap, dtype=np.uint8)),
                            into=None if into is None else into[0], **common, **kw)
    assert_evidence(got, want)
    if pile:
        return got, want, W.pileup(*args, min_qual=kw.get("min_qual", 0), **common)
    return got, want


def links_both(sites, ops, lo, n_ref, strand, query, qual=None, keep=None, cap=None, ops_len=None, query_len=None, into=None, reach=4, pile=False, **kw):
    """links, observed and `used` must agree exactly -> (PhaseLinks, reference Links) and, with pile=True, the Pileup of the same
    batch beside them"""
    ops_rows, ops_len, q_rows, q_len, qual_rows = host_rows(ops, query, qual, ops_len, query_len)
    want = H.links_ref(sites, ops_rows, ops_len, lo, n_ref, strand, q_rows, q_len, qual=qual_rows, keep=keep, cap=cap, reach=reach,
                       into=None if into is None else into[1], **kw)
    args = (alignment(ops_rows, ops_len), i32(lo), i32(n_ref), i32(strand), dev(q_rows), i32(q_len))
    common = dict(qual=None if qual is None else dev(qual_rows), keep=None if keep is None else torch.tensor(keep, device=DEV))
    got = W.phase_links(*args, sites_dev(sites), cap=None if cap is None else u8(cap), reach=reach, into=None if into is None else into[0],
                        **common, **kw)
    assert_links(got, want)
    if pile:
        return got, want, W.pileup(*args, len(sites.site_of), min_qual=kw.get("min_qual", 0), **common)
    return got, want


def tags_both(sites, chain, host, qual=None, keep=None, cap=None, report=0, **kw):
    """host: (ops rows, ops_len, lo, n_ref, strand, query rows, query_len) -> the reference Tags, equal to the kernel's exactly"""
    want = H.haplotag_ref(sites, chain, *host, qual=qual, keep=keep, cap=cap, **kw)
    got = W.haplotag(alignment(host[0], host[1]), i32(host[2]), i32(host[3]), i32(host[4]), dev(np.asarray(host[5])), i32(host[6]), sites_dev(sites),
                     chain_dev(chain), qual=None if qual is None else dev(qual), keep=None if keep is None else torch.tensor(keep, device=DEV),
                     cap=None if cap is None else u8(cap), **kw)
    if report:
        with pytest.raises(RuntimeError, match="wavenet_speech_amd.haplotag: %d pair\\(s\\) whose ops do not fit" % report):
            W.check_device_flags()
    W.check_device_flags()
    _dtypes(got, ("hp",), torch.uint8)
    _dtypes(got, ("ps", "weight", "n_sites"), torch.int32)
    assert_tags(got, want)
    return want
