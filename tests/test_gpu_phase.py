"""GPU: phase_sites / phase_links / phase_chain / haplotag / phased_records (csrc/wn_phase.hip through wavenet_speech_amd/phase.py)
against the reference of tests/phase_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality,
ties included; tests/test_phase_ref.py holds the reference itself on the CPU, and the planted run is built once in
tests/phase_cases.py.  Every shape is tiny: T = 256 op columns is the walk's tile and the chain kernels' workgroup."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import opwalk_cases as O
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import pileup_ref as P
from tests.gpu_calls import alignment as _alignment, assert_chain as _assert_chain, assert_counts as _assert_counts, assert_links as _assert_links
from tests.gpu_calls import assert_tags as _assert_tags, host_rows as _rows, links_both as _both, sites_dev as _sites_dev, tags_both as _tags_both
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu
T = 256


def _random_sites(rng, R, density=0.15, forced=()):
    """a Sites over R positions: every position a site with chance `density`, the forced ones always; random pairs of two different
    labels of 0..4 in allele order (0, the deletion, last)"""
    pos = sorted(set(int(p) for p in np.flatnonzero(rng.random(R) < density)) | set(forced))
    site_of = [-1] * R
    alleles = []
    for s, p in enumerate(pos):
        site_of[p] = s
        a, b = sorted((int(v) for v in rng.choice(5, size=2, replace=False)), key=lambda v: (v == 0, v))
        alleles.append((a, b))
    return H.Sites(pos, alleles, site_of)


# ---- phase_links ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reach", [1, 8])
def test_links_at_the_tile_edges_on_both_strands(reach):
    rng = np.random.default_rng(1)
    strings = [C.random_ops(rng, n) for n in (T - 1, T, T + 1, 2 * T + 1)]
    strings += [[1] * (2 * T + 1),                                   # column c is position lo + c: sites in the first and last column, on the tile edges
                [2] * (T - 6) + [3] * 12 + [2] * 9,                  # a deletion run of sites across the first tile edge
                [3] * T + [1] * 20 + [4] * 3,                        # the first aligned column on a tile edge, end columns before it
                [4] * 7 + [1] * (T - 8) + [1] + [3] * 30,            # the last aligned column at T - 1
                [1] * T + [4, 4] + [3] + [4] + [1] * (T - 3)]
    strings += [s[::-1] for s in strings[5:]]                        # a reverse-strand read walks its columns back to front
    reads = [C.read(s, rng) for s in strings]
    ops, n_ref, query, qual = C.cols(reads)
    n = len(reads)
    R = 2 * T + 1
    lo = [0 if b % 2 == 0 else R - n_ref[b] for b in range(n)]       # windows at 0 and windows that end at R
    sites = _random_sites(rng, R, 0.2, forced=(0, 1, T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T))
    cap = [int(v) for v in rng.integers(0, 120, size=n)]
    for strands in ([0] * n, [1] * n, [b & 1 for b in range(n)]):
        got, want, pile = _both(sites, ops, lo, n_ref, strands, query, qual=qual, min_qual=12, cap=cap, gap_qual=17, reach=reach, pile=True)
        assert want.used.tolist() == [1] * n and torch.equal(got.used, pile.used)
        _assert_counts(want.observed, sites, pile)
        assert sum(v for s in want.links for c in s for v in c) > 0 and sum(o[2] for o in want.observed) > 0 and sum(sum(o) for o in want.observed) > 100
    W.check_device_flags()


def test_quals_caps_flat_qual_a_deleted_allele_and_a_neither_base():
    sites = H.Sites([1, 3, 4, 6, 8], [(1, 2), (3, 0), (2, 4), (1, 4), (1, 3)], [-1, 0, -1, 1, 2, -1, 3, -1, 4, -1])
    ops = [1, 1, 1, 3, 1, 1, 1, 1, 1, 1]
    query, qual = [4, 2, 4, 3, 4, 1, 4, 0, 4], [9, 30, 9, 10, 9, 5, 9, 40, 9]
    rows = ([ops, ops[::-1]], [0, 0], [10, 10], [0, 1], [query, C.revcomp(query)])
    quals = [qual, qual[::-1]]
    for min_qual in (0, 5, 6, 10, 11, 93):                           # quals on both sides of min_qual
        got, want, pile = _both(sites, *rows, qual=quals, min_qual=min_qual, gap_qual=15, reach=8, pile=True)
        _assert_counts(want.observed, sites, pile)
    for cap in ([4, 4], [5, 5], [6, 6], [0, 0], [15, 16], [93, 255], [29, 30]):      # below, at and above q and gap_qual
        got, want = _both(sites, *rows, qual=quals, cap=cap, gap_qual=15, reach=8)
    assert want.links[1][0] == [30, 0] and want.links[3][1] == [0, 10] and want.observed[2] == [0, 0, 2]      # the values of tests/test_phase_ref.py
    for flat in (0, 20, 93):                                         # no qual: flat_qual on every base, min_qual asks nothing
        got, want = _both(sites, *rows, flat_qual=flat, min_qual=50, gap_qual=93 - flat, cap=[255, 20], reach=3)
    got, want = _both(sites, *rows, flat_qual=41)
    same, _ = _both(sites, *rows, qual=[[41] * 9] * 2)
    assert torch.equal(got.links, same.links) and int(got.links.sum()) > 0
    W.check_device_flags()


@pytest.mark.parametrize("reach", [1, 8])
def test_a_read_that_holds_reach_plus_3_sites(reach):
    n = reach + 3
    sites = H.Sites(list(range(0, 2 * n, 2)), [(1, 2)] * n, [p // 2 if p % 2 == 0 else -1 for p in range(2 * n)])
    query = [1 + (p // 2) % 2 if p % 2 == 0 else 3 for p in range(2 * n)]
    for strand in (0, 1):
        got, want = _both(sites, [[1] * 2 * n], [0], [2 * n], [strand], [C.revcomp(query) if strand else query], reach=reach, flat_qual=7)
        assert int(got.links.sum()) == 7 * sum(n - d for d in range(1, reach + 1))
    W.check_device_flags()


def test_skipped_reads_are_not_looked_at():
    rng = np.random.default_rng(5)
    good = C.read([3, 1, 2, 4, 1, 3, 1, 4], rng, odd=0.0)
    ops = [good[0], good[0], good[0], [3] * 6, [3, 3, 3, 4, 4], good[0], [9] * 8]
    query = [good[2], good[2], good[2], [], [1, 2], good[2], good[2]]
    sites = _random_sites(rng, 8, 1.0)
    # unmapped (strand -1, with a window that would be bad), ref_lengths 0, keep false, empty, end columns only, good, unmapped garbage
    got, want = _both(sites, ops, [0, 0, 0, 0, 0, 1, -7], [6, 0, 6, 6, 3, 6, 99], [-1, 0, 1, 0, 1, 1, -2], query,
                      keep=[True, True, False, True, True, True, True], ops_len=[8, 8, 8, 6, 5, 8, 200], query_len=[6, 6, 6, 0, 2, 6, -3])
    assert want.used.tolist() == [0, 0, 0, 0, 0, 1, 0] and want.bad == 0 and sum(sum(o) for o in want.observed) == 5
    W.check_device_flags()                                           # nothing is reported


def test_one_bad_read_of_every_kind_between_good_ones():
    """the rows of tests/opwalk_cases.py, reordered so that every refused row lies between valid ones: `used` and the bad count are
    the pileup's on the same batch"""
    t = O.batch()
    valid, refused = O.rows_of(O.VALID), O.rows_of(O.BAD, O.STRAND_ONLY, O.SKIPPED)
    order = [b for pair in zip(valid, refused) for b in pair] + refused[len(valid):] + valid[len(refused):] + valid[-1:]
    assert sorted(set(order)) == list(range(len(t.kind))) and valid[-1] == order[-1] and t.ops_len[order[-1]] == 513
    rng = np.random.default_rng(17)
    sites = _random_sites(rng, O.R, 0.3)
    host = (t.ops[order], t.ops_len[order], t.lo[order], t.ref_len[order], t.strand[order], t.query[order], t.query_len[order])
    want = H.links_ref(sites, *host, qual=t.qual[order], min_qual=O.MIN_QUAL, reach=8)
    want_pile = P.pileup_ref(*host, O.R, qual=t.qual[order], min_qual=O.MIN_QUAL, max_ins=O.MAX_INS)
    assert want.used.tolist() == want_pile.used.tolist() and want.bad == want_pile.bad == 12
    W.check_device_flags()
    reads = (_alignment(t.ops[order], t.ops_len[order]), _dev(t.lo[order]), _dev(t.ref_len[order]), _dev(t.strand[order]), _dev(t.query[order]),
             _dev(t.query_len[order]))
    got = W.phase_links(*reads, _sites_dev(sites), qual=_dev(t.qual[order]), min_qual=O.MIN_QUAL, reach=8)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.phase_links: 12 pair\\(s\\) whose ops do not fit"):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once
    _assert_links(got, want)
    pile = W.pileup(*reads, O.R, qual=_dev(t.qual[order]), min_qual=O.MIN_QUAL, max_ins=O.MAX_INS)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup: 12 pair"):
        W.check_device_flags()
    assert torch.equal(got.used, pile.used) and (got.used == -1).sum().item() == 12
    _assert_counts(want.observed, sites, pile)
    good = valid + valid[-1:]
    only_valid = H.links_ref(sites, *[a[good] for a in (t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query, t.query_len)], qual=t.qual[good],
                             min_qual=O.MIN_QUAL, reach=8)
    assert want.links == only_valid.links                            # the good reads' sums are intact
    # the tags of the same batch: a refused read is untagged, and counted once more
    chain = H.chain_ref(want.links, sites.pos)
    tags = _tags_both(sites, chain, host, qual=t.qual[order], min_qual=O.MIN_QUAL, report=12)
    assert all(tags.hp[b] == 0 and tags.ps[b] == -1 for b in range(len(order)) if want.used[b] != 1) and max(tags.hp) > 0


def test_the_carry_of_a_true_64_bit_add():
    """cells preset to 2^32 - 1 that take an add of 1, and one preset to 2^51"""
    sites = H.Sites([1, 2, 3], [(1, 2), (1, 2), (1, 2)], [-1, 0, 1, 2])
    preset = [[[0, 0], [0, 0]], [[2 ** 32 - 1, 2 ** 32 - 1], [5, 5]], [[2 ** 51, 7], [2 ** 32 - 1, 2 ** 32 - 1]]]
    observed = [[0, 0, 0], [2 ** 31 - 2, 0, 0], [0, 0, 0]]
    into = (W.PhaseLinks(torch.tensor(preset, dtype=torch.int64, device=DEV), torch.tensor(observed, dtype=torch.int32, device=DEV), None),
            H.Links(preset, observed, None, 0))
    # both reads show A, A, A (all cis) and A, G, A (1 trans to 0 and to 2; 0 and 2 cis) with weight 1
    got, want = _both(sites, [[1, 1, 1]] * 2, [1, 1], [3, 3], [0, 1], [[1, 1, 1], [4, 3, 4]], reach=2, flat_qual=1, into=into)
    assert want.links == [[[0, 0], [0, 0]], [[2 ** 32, 2 ** 32], [5, 5]], [[2 ** 51 + 1, 8], [2 ** 32 + 1, 2 ** 32 - 1]]]
    assert want.observed[1] == [2 ** 31 - 1, 1, 0]
    assert got.links is into[0].links and got.observed is into[0].observed
    W.check_device_flags()


def test_contention_on_one_locus():
    rng = np.random.default_rng(8)
    ops, n_ref, query, qual = C.read([1] * 12 + [4, 4] + [1] * 10 + [3] + [2] * 17, rng, odd=0.05)
    assert n_ref == 40
    sites = _random_sites(rng, 40, 0.0, forced=(2, 9, 17, 22, 30, 39))      # 6 sites; position 22 is the deletion column
    sites = sites._replace(alleles=[(1, 0) if p == 22 else a for p, a in zip(sites.pos, sites.alleles)])
    got, want = _both(sites, [ops] * 300, [0] * 300, [40] * 300, [0] * 300, [query] * 300, qual=[qual] * 300, gap_qual=2, reach=8)
    assert want.observed[3] == [0, 300, 0] and sum(sum(c) for c in want.links[5]) % 300 == 0 and sum(sum(c) for c in want.links[3]) > 0
    reads = [r for r in (C.read(C.random_ops(rng, 42), rng) for _ in range(300)) if r[1] <= 40]
    ops, n_ref, query, qual = C.cols(reads)
    n = len(reads)
    got, want = _both(sites, ops, [40 - r[1] if b % 3 else 0 for b, r in enumerate(reads)], n_ref, [int(v) for v in rng.integers(0, 2, size=n)], query,
                      qual=qual, cap=[int(v) for v in rng.integers(0, 94, size=n)], reach=5)
    assert n > 200 and min(sum(o) for o in want.observed) > 100
    W.check_device_flags()


def test_accumulation_over_batches_and_reproducibility():
    rng = np.random.default_rng(9)
    reads = [C.read(C.random_ops(rng, int(rng.integers(40, 300))), rng) for _ in range(24)]
    sites = _random_sites(rng, 400, 0.1)
    args = lambda part, first=0: (C.cols(part)[0], [2 * b for b in range(first, first + len(part))], C.cols(part)[1],      # noqa: E731
                                  [b & 1 for b in range(first, first + len(part))], C.cols(part)[2])
    kw = lambda part: dict(qual=C.cols(part)[3], min_qual=9)          # noqa: E731
    whole, _, pile = _both(sites, *args(reads), pile=True, **kw(reads))
    again, _ = _both(sites, *args(reads), **kw(reads))
    assert torch.equal(whole.links, again.links) and torch.equal(whole.observed, again.observed)    # bitwise: integer addition commutes
    _assert_counts(whole.observed.cpu().tolist(), sites, pile)
    first = _both(sites, *args(reads[:12]), **kw(reads[:12]))
    second = _both(sites, *args(reads[12:], 12), into=first, **kw(reads[12:]))
    assert second[0].links is first[0].links and torch.equal(second[0].links, whole.links) and torch.equal(second[0].observed, whole.observed)
    one = (_alignment(*C.rows([reads[0][0]], dtype=np.uint8)), _i32([0]), _i32([reads[0][1]]), _i32([0]), _i32([reads[0][2]]), _i32([len(reads[0][2])]))
    S = len(sites.pos)
    with pytest.raises(ValueError, match="wavenet_speech_amd.phase_links: into.links must be a contiguous int64 tensor of shape \\(%d, 3, 2\\)" % S):
        W.phase_links(*one, _sites_dev(sites), reach=3, into=whole)                               # another reach
    fewer = _random_sites(rng, 400, 0.05)
    with pytest.raises(ValueError, match="wavenet_speech_amd.phase_links: into.links must be a contiguous int64 tensor of shape \\(%d, 4, 2\\)" % len(fewer.pos)):
        W.phase_links(*one, _sites_dev(fewer), into=whole)                                        # another S
    W.check_device_flags()


def test_no_site_at_all():
    g = W.Genotypes(torch.ones(50, 2, dtype=torch.uint8, device=DEV), None, None, torch.full((50,), W.Genotypes.SUBSTITUTION, dtype=torch.uint8, device=DEV),
                    None, None, None, None, None, None)
    sites = W.phase_sites(g)
    assert tuple(sites.pos.shape) == (0,) and tuple(sites.alleles.shape) == (0, 2) and sites.site_of.tolist() == [-1] * 50
    reads = (_alignment(*C.rows([[1] * 9], dtype=np.uint8)), _i32([0]), _i32([9]), _i32([0]), _i32([[1] * 9]), _i32([9]))
    links = W.phase_links(*reads, sites, reach=2)
    assert tuple(links.links.shape) == (0, 2, 2) and tuple(links.observed.shape) == (0, 3) and links.used is None
    phasing = W.phase_chain(links, sites)
    assert all(tuple(t.shape) == (0,) for t in phasing)
    tags = W.haplotag(*reads, sites, phasing)
    assert tags.hp.tolist() == [0] and tags.ps.tolist() == [-1] and tags.weight.tolist() == [[0, 0]] and tags.n_sites.tolist() == [[0, 0]]
    W.check_device_flags()


# ---- phase_chain, on hand-given links ---------------------------------------------------------------------------------------------

def _chain_both(links, pos, **kw):
    want = H.chain_ref(links, pos, **kw)
    S = len(pos)
    sites = W.PhaseSites(_i32(pos), torch.ones(S, 2, dtype=torch.uint8, device=DEV), torch.full((max(pos) + 1,), -1, dtype=torch.int32, device=DEV))
    got = W.phase_chain(W.PhaseLinks(torch.tensor(links, dtype=torch.int64, device=DEV).reshape(S, -1, 2), None, None), sites, **kw)
    _assert_chain(got, want)
    return got, want


def _positions(rng, S):
    return np.cumsum(rng.integers(1, 5, size=S)).tolist()


@pytest.mark.parametrize("S", [1, 2, 255, 256, 257, 1025])
def test_the_chain_at_the_tile_edges(S):
    rng = np.random.default_rng(S)
    pos = _positions(rng, S)
    # one path through all S sites, the deepest tree, with random flips: only d = 1 holds a margin
    path = [[[int(c), int(t)]] + [[3, 3]] * 7 for c, t in zip(rng.integers(0, 9, size=S), rng.integers(10, 19, size=S))]
    for s in range(0, S, 3):
        path[s][0].reverse()
    got, want = _chain_both(path, pos)
    assert want.root == [0] * S and want.set_size == [S] * S and want.parent == [0] + list(range(S - 1)) and (S < 3 or 0 < sum(want.parity) < S)
    # all sites roots: no margin anywhere, and margins below min_margin
    got, want = _chain_both([[[5, 5]] * 4] * S, pos)
    assert want.root == list(range(S)) and want.set_size == [1] * S and want.ps == pos
    got, want = _chain_both(path, pos, min_margin=19)
    assert want.root == list(range(S))
    # random forests at reach 8 with random flips; small values: ties in d and cis == trans are common
    for top, min_margin in ((4, 1), (4, 2), (50, 1), (3, 0)):
        links = rng.integers(0, top, size=(S, 8, 2)).tolist()
        got, want = _chain_both(links, pos, min_margin=min_margin)
        assert (top, min_margin) != (4, 2) or S < 255 or (1 < len(set(want.root)) < S and max(want.set_size) > 8)


def test_the_chain_at_every_tie_and_at_the_clamp():
    from tests.phase_cases import CHAIN_LINKS, CHAIN_POS
    for min_margin in (0, 1, 2, 5):
        _chain_both(CHAIN_LINKS, CHAIN_POS, min_margin=min_margin)
    top = 2 ** 31 - 1
    links = [[[0, 0]], [[top - 1, 0]], [[0, top]], [[top + 1, 0]], [[2 ** 31 * 93, 1]], [[1, 2 ** 62]], [[top, 2 * top]]]
    got, want = _chain_both(links, list(range(7)), min_margin=top)
    assert want.margin == [0, 0, top, top, top, top, top] and want.parent == [0, 1, 1, 2, 3, 4, 5] and want.flip == [0, 0, 1, 0, 0, 1, 1]
    got, want = _chain_both(links, list(range(7)))
    assert want.margin[1] == top - 1 and want.root == [0] * 7 and want.set_size == [7] * 7


# ---- haplotag ---------------------------------------------------------------------------------------------------------------------

def test_haplotags_by_hand():
    """the rows of tests/test_phase_ref.py::test_haplotags_by_hand, and a bad read beside them"""
    from tests.phase_cases import CHAIN_LINKS, SITES
    chain = H.chain_ref(CHAIN_LINKS[:5], SITES.pos)
    rows = [([1] * 10, 10, 0, [4, 1, 4, 3, 4, 4, 1, 4, 3, 4], [9, 20, 9, 20, 30, 9, 30, 9, 5, 9]),      # the arg-max ties at 30: the least site
            ([1] * 10, 10, 0, [4, 1, 4, 3, 2, 4, 4, 4, 4, 4], [9, 20, 9, 5, 25, 9, 9, 9, 9, 9]),       # weight[0] == weight[1]; one site elsewhere
            ([1] * 10, 10, 0, [4, 4, 4, 4, 3, 4, 2, 4, 2, 4], [9] * 10),                               # only `neither`
            ([1] * 6, 6, -1, [4, 1, 4, 4, 4, 4], [9] * 6),                                             # skipped
            ([1, 7, 1], 3, 0, [1, 1, 1], [9] * 3),                                                     # bad
            ([1] * 5, 5, 1, [1] * 5, [9] * 5)]                                                         # reverse: T at 6 and 8, its window [5, 10)
    ops, ops_len = C.rows([r[0] for r in rows], dtype=np.uint8)
    query, q_len = C.rows([r[3] for r in rows])
    qual = C.rows([r[4] for r in rows], width=query.shape[1], dtype=np.uint8)[0]
    host = (ops, ops_len, [0, 0, 0, 0, 0, 5], [r[1] for r in rows], [r[2] for r in rows], query, q_len)
    want = _tags_both(SITES, chain, host, qual=qual, report=1)
    assert want.hp == [1, 0, 0, 0, 0, 2] and want.ps == [1, 1, -1, -1, -1, 6] and want.weight[:2] == [[70, 0], [25, 25]]
    assert want.n_sites == [[3, 2], [3, 1], [0, 0], [0, 0], [0, 0], [1, 0]]
    # a site that stands alone does not count: with min_margin 5 only sites 3 and 5 of six are linked
    for min_qual, cap in ((0, None), (10, None), (0, [10, 25, 93, 0, 0, 8])):
        for min_margin in (1, 2, 5):
            _tags_both(SITES, H.chain_ref(CHAIN_LINKS[:5], SITES.pos, min_margin=min_margin), host, qual=qual, min_qual=min_qual, cap=cap, report=1)


def test_haplotags_of_random_reads_across_sets():
    rng = np.random.default_rng(21)
    R = 2 * T + 40
    sites = _random_sites(rng, R, 0.25, forced=(0, R - 1))
    S = len(sites.pos)
    chain = H.chain_ref(rng.integers(0, 3, size=(S, 2, 2)).tolist(), sites.pos)          # many small sets: every read spans several
    assert 10 < len(set(chain.root)) < S and 1 in chain.set_size
    reads = [C.read(C.random_ops(rng, n), rng) for n in (T - 1, T, T + 1, 2 * T + 1, 60, 300, 17, 2 * T + 1)]
    reads = [r for r in reads if r[1] <= R]
    ops, n_ref, query, qual = C.cols(reads)
    n = len(reads)
    ops_rows, ops_len, q_rows, q_len, qual_rows = _rows(ops, query, qual, None, None)
    few = (rng.integers(0, 3, size=qual_rows.shape) * 10).astype(np.uint8)               # three weights only: the arg-max ties all the time
    for strands in ([0] * n, [1] * n, [b & 1 for b in range(n)]):
        host = (ops_rows, ops_len, [0 if b % 2 else R - n_ref[b] for b in range(n)], n_ref, strands, q_rows, q_len)
        want = _tags_both(sites, chain, host, qual=qual_rows, min_qual=12, cap=[int(v) for v in rng.integers(0, 120, size=n)], gap_qual=33)
        assert max(w[1] for w in want.n_sites) > 0 and set(want.hp) >= {1, 2}
        _tags_both(sites, chain, host, qual=few, gap_qual=10)
        _tags_both(sites, chain, host, flat_qual=7, gap_qual=7)


# ---- the closed loop on the planted runs ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noisy", [False, True])
def test_closed_loop_on_the_planted_phased_runs(noisy):
    run = PC.planted(noisy)
    labels, lengths, qual = _dev(run["labels"]), _dev(run["lengths"]), _dev(run["qual"])
    index = W.read_index(_i32(run["ref"]), k=11, w=5)
    m = W.map_reads(labels, lengths, index)
    lo, length = m.window(C.PLANT_FLANK)
    ref_rows, ref_len = m.labels(C.PLANT_FLANK)
    assert torch.equal(length, ref_len) and m.strand.cpu().tolist() == run["strand"]
    aln = W.pairwise_align(ref_rows, ref_len, labels, lengths)
    aln = W.left_align(aln, ref_rows, ref_len, labels, lengths, m.strand).alignment
    w = W.genotype_weights(K.SCALE)
    reads = (aln, lo, ref_len, m.strand, labels, lengths)
    pile = W.pileup(*reads, index.R, qual=qual, min_qual=PC.MIN_QUAL)
    ev = W.pileup_evidence(*reads, index.R, w, qual=qual, min_qual=PC.MIN_QUAL)
    calls = W.call_genotypes(pile, ev, index, w)
    sites = W.phase_sites(calls)
    links = W.phase_links(*reads, sites, qual=qual, min_qual=PC.MIN_QUAL, reach=PC.REACH)
    phasing = W.phase_chain(links, sites)
    tags = W.haplotag(*reads, sites, phasing, qual=qual, min_qual=PC.MIN_QUAL)
    records = W.phased_records(index, calls, pile, sites, phasing)
    # the reference fed with the GPU's own windows and ops
    host = (aln.ops.cpu().numpy(), aln.ops_len.cpu().numpy(), lo.cpu().tolist(), ref_len.cpu().tolist())
    args = host + (run["strand"], run["labels"], run["lengths"], index.R)
    want_pile = P.pileup_ref(*args, qual=run["qual"], min_qual=PC.MIN_QUAL)
    want_ev = G.evidence_ref(K.weights(), *args, qual=run["qual"], min_qual=PC.MIN_QUAL)
    want_calls = G.call_genotypes_ref(want_pile, want_ev.evidence, run["ref"], K.weights(), alt_prior=K.ALT_PRIOR)
    assert np.array_equal(calls.flags.cpu().numpy(), want_calls.flags) and np.array_equal(calls.alleles.cpu().numpy(), want_calls.alleles)
    want = PC.phase_all(run, *host, want_pile, want_calls)
    assert sites.pos.dtype == sites.site_of.dtype == torch.int32 and sites.alleles.dtype == torch.uint8
    assert sites.pos.cpu().tolist() == want["sites"].pos and sites.site_of.cpu().tolist() == want["sites"].site_of
    assert [tuple(a) for a in sites.alleles.cpu().tolist()] == want["sites"].alleles
    _assert_links(links, want["links"])
    _assert_counts(links.observed.cpu().tolist(), want["sites"], pile)
    assert torch.equal(links.used, pile.used)
    _assert_chain(phasing, want["chain"])
    _assert_tags(tags, want["tags"])
    assert [tuple(v) for v in records] == want["records"]
    # the five conditions, on the device's tables
    got = dict(sites=want["sites"]._replace(pos=sites.pos.cpu().tolist()), chain=H.Chain(*[t.cpu().tolist() for t in phasing]),
               tags=H.Tags(tags.hp.cpu().tolist(), tags.ps.cpu().tolist(), None, None, None, 0), per_read=want["per_read"])
    assert PC.check_conditions(run, got) > PC.READS // 2
    lines = W.vcf_phased_records("chr", index, calls, pile, sites, phasing, w)
    phased = [l for l in lines if "|" in l]
    assert len(lines) == len(records) and len(phased) == len(lines) - 6 and all(l.split("\t")[8] == "GT:GQ:PS" for l in lines)
    assert {l.rstrip("\n").split(":")[-1] for l in phased} == {str(p + 1) for p in set(want["chain"].ps)}
    W.check_device_flags()
