"""GPU: global pairwise alignment with affine gaps (csrc/wn_pairalign.hip through wavenet_speech_amd.pairwise_align and
edit_distance) against the numpy int64 reference of tests/pairwise_align_ref.py.

The arithmetic is integer and the tie rule is part of the contract, so EVERYTHING is compared for exact equality: the score,
the four counts, ops_len and every op -- no tolerance and no excluded case.  Next to that, checks that do not depend on the
reference: the ops spell both input rows exactly once, rescore to the score, and the counts are the op counts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import pairwise_align_ref as R
from tests.gpu_labels import check_pair as _check_pair, check_pair_batch as _check_batch, package as _W, pad_rows as _pad, pair_align as _align
from tests.gpu_util import DEV, peaked_logits as _peaked_logits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emboss_pairs.json")
BASES = {"A": 1, "G": 2, "C": 3, "T": 4}
COST_SETS = {"emboss": R.EMBOSS, "unit": R.UNIT, "open_eq_extend": (2, -3, 2, 2)}      # integers: half units
INT_MIN = -2 ** 31


def _mutate(rng, ref, rate, alphabet):
    """a query made from the reference by substitutions, insertions and deletions, `rate` of the positions each way"""
    out = []
    for v in ref:
        u = rng.random()
        if u < rate / 3:
            continue                                                 # deletion
        if u < 2 * rate / 3:
            out.append(int(rng.integers(1, alphabet + 1)))           # insertion before
        if u > 1 - rate / 3:
            v = int(rng.integers(1, alphabet + 1))                   # substitution (may draw the same label)
        out.append(int(v))
    return out


def _golden_pairs():
    pairs = json.load(open(GOLDEN))["pairs"]
    return [[BASES[c] for c in p["true"]] for p in pairs], [[BASES[c] for c in p["pred"]] for p in pairs], pairs


# ------------------------------------------------------------------------------------------------------- 1. the notebook's pairs

def test_the_notebook_pairs_with_the_emboss_costs():
    refs, queries, recorded = _golden_pairs()
    got = _align(refs, queries, R.EMBOSS, True)
    want = _check_batch(refs, queries, R.EMBOSS, True, got, "notebook")
    for n, (w, p) in enumerate(zip(want, recorded)):                 # and needle itself: never above our optimum
        assert w.score / 2 >= p["score"], n
    # the default arguments ARE needle's costs
    a, an = _pad(refs)
    b, bn = _pad(queries)
    out = _W().pairwise_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV))
    assert np.array_equal((out.score.double() * 2).cpu().numpy().astype(np.int64), got[0])
    assert torch.equal(out.identity.cpu(), out.matches.cpu().float() / out.length.cpu().float())
    assert torch.equal(out.matches.cpu(), torch.tensor([w.matches for w in want], dtype=torch.int32))


# -------------------------------------------------------------------------------------- 2. random pairs, every mode and cost set

@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", sorted(COST_SETS))
@pytest.mark.parametrize("kind", ["mutated4", "unrelated4", "mutated2", "unrelated2"])
def test_random_pairs(kind, costs, free):
    alphabet = int(kind[-1])                                         # 2 letters: ties everywhere, the tie rule decides
    rng = np.random.default_rng(sorted(COST_SETS).index(costs) * 10 + alphabet + (100 if free else 0))
    lens = [300, 257, 120, 64, 33, 8, 1, 200]
    refs = [rng.integers(1, alphabet + 1, size=n).tolist() for n in lens]
    if kind.startswith("mutated"):
        queries = [_mutate(rng, r, rng.uniform(0.10, 0.25), alphabet) for r in refs]
    else:
        queries = [rng.integers(1, alphabet + 1, size=int(rng.integers(1, 320))).tolist() for _ in lens]
    got = _align(refs, queries, COST_SETS[costs], free)
    _check_batch(refs, queries, COST_SETS[costs], free, got, kind)


def test_ties_are_really_met():
    """the 2-letter pairs must contain cells where two candidates tie, or the tie rule is not exercised: count them on the host"""
    rng = np.random.default_rng(5)
    a, b = rng.integers(1, 3, size=60).tolist(), rng.integers(1, 3, size=60).tolist()
    go, ge = R.UNIT[2], R.UNIT[3]
    H, _ = R.fill(a, b, *R.UNIT, False)
    ties = 0
    for i in range(1, 61):
        for j in range(1, 61):
            d = H[i - 1, j - 1] + (R.UNIT[0] if a[i - 1] == b[j - 1] else R.UNIT[1])
            ties += int(d == H[i, j - 1] - go) + int(d == H[i - 1, j] - ge)
    assert ties > 100, ties
    got = _align([a], [b], R.UNIT, False)
    _check_batch([a], [b], R.UNIT, False, got, "ties")


# ------------------------------------------------------------------------------------------------------ 3. thread-count edges

@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("M", [1, 7, 8, 9, 511, 512, 513, 1023, 1025])
def test_query_lengths_at_the_thread_count_edges(M, free):
    """8 columns per thread, one wave up to 512 columns, one more wave per 512 after that; N in {1, M/3, M, 2M}, ragged"""
    rng = np.random.default_rng(1000 + M)
    ref_lens = [1, max(M // 3, 1), M, 2 * M, M]
    query_lens = [M, M, M, M, max(M // 2, 1)]
    refs = [rng.integers(1, 5, size=n).tolist() for n in ref_lens]
    queries = [_mutate(rng, refs[2], 0.2, 4)[:n] if k == 2 else rng.integers(1, 5, size=n).tolist() for k, n in enumerate(query_lens)]
    queries[2] = (queries[2] + rng.integers(1, 5, size=M).tolist())[:M]
    costs = R.EMBOSS if M % 2 else COST_SETS["open_eq_extend"]
    got = _align(refs, queries, costs, free)
    _check_batch(refs, queries, costs, free, got, "M%d" % M)


@pytest.mark.parametrize("N,M", [(64, 8192), (4096, 64)])
def test_the_widest_workgroup_and_the_longest_stream(N, M):
    rng = np.random.default_rng(N + M)
    refs = [rng.integers(1, 5, size=N).tolist()]
    if M > N:                                                        # the reference is a mutated stretch of the long query
        q = rng.integers(1, 5, size=M).tolist()
        refs = [_mutate(rng, q[5000:5000 + N], 0.15, 4)[:N]]
        queries = [q]
    else:
        queries = [_mutate(rng, refs[0][1000:1000 + M], 0.15, 4)[:M]]
    for free in (True, False):
        got = _align(refs, queries, R.EMBOSS, free)
        want = _check_batch(refs, queries, R.EMBOSS, free, got, "%dx%d" % (N, M))
        if free:
            assert want[0].matches > 40                              # the stretch was found


# -------------------------------------------------------------------------------------------- 4. score-only form, edit distance

def test_score_only_and_stats_only_equal_the_full_form():
    from wavenet_speech_amd import decoding as D
    rng = np.random.default_rng(11)
    refs = [rng.integers(1, 5, size=n).tolist() for n in (600, 90, 0, 513, 17)]
    queries = [_mutate(rng, r, 0.2, 4) for r in refs]
    queries[1] = []
    for name, costs in sorted(COST_SETS.items()):
        for free in (True, False):
            full = _align(refs, queries, costs, free)
            a, an = _pad(refs)
            b, bn = _pad(queries)
            score, stats, ops, ops_len = D._pair_align("test", a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV), costs, free, False, False)
            assert stats is None and ops is None and ops_len is None
            assert np.array_equal(score.cpu().numpy(), full[0]), (name, free)
            counts = _align(refs, queries, costs, free, return_ops=False)
            assert np.array_equal(counts[0], full[0]) and np.array_equal(counts[1], full[1]), (name, free)
    _W().check_device_flags()


def test_edit_distance_equals_levenshtein():
    W = _W()
    rng = np.random.default_rng(12)
    a_lens = [0, 1, 50, 300, 520, 7, 64, 100]
    refs = [rng.integers(1, 5, size=n).tolist() for n in a_lens]
    queries = [_mutate(rng, r, 0.25, 4) for r in refs]
    queries[5] = []
    queries[6] = rng.integers(1, 3, size=90).tolist()
    a, an = _pad(refs, dtype=torch.int64)
    b, bn = _pad(queries)
    d = W.edit_distance(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV))
    assert d.dtype == torch.int32 and d.is_cuda and d.shape == (8,)
    want = [R.levenshtein(x, y) for x, y in zip(refs, queries)]
    assert d.cpu().tolist() == want
    assert want == [-R.align(x, y, *R.UNIT, False).score for x, y in zip(refs, queries)]
    W.check_device_flags()


# ------------------------------------------------------------------------------------------------------------- 5. edge cases

@pytest.mark.parametrize("free", [True, False])
def test_zero_length_rows(free):
    refs = [[], [1, 2, 3], [], [4], [1, 2, 3, 4, 1, 2, 3, 4, 1], []]
    queries = [[1, 2], [], [], [4], [], [3] * 20]
    for costs in (R.EMBOSS, R.UNIT):
        got = _align(refs, queries, costs, free, ref_width=12, query_width=21, fill=3)
        _check_batch(refs, queries, costs, free, got, "zero")
        score, stats, ops, ops_len = got
        assert ops_len.tolist() == [2, 3, 0, 1, 9, 20]
        assert ops[0, :2].tolist() == [4, 4] and ops[1, :3].tolist() == [3, 3, 3] and ops[3, 0] == 1
        assert stats[2].tolist() == [0, 0, 0, 0] and score[2] == 0
    # tensors without any column
    W = _W()
    none = torch.zeros(2, 0, dtype=torch.int32, device=DEV)
    some, n_some = _pad([[1, 2, 3], [4]])
    out = W.pairwise_align(none, torch.zeros(2, dtype=torch.int32), some.to(DEV), n_some, end_gaps_free=free)
    assert out.ops.shape == (2, 3) and out.ops_len.tolist() == [3, 1] and out.gaps.tolist() == [3, 1]
    assert out.ops.cpu().tolist() == [[4, 4, 4], [4, 0, 0]]
    W.check_device_flags()


def test_values_past_the_lengths_are_never_read():
    rng = np.random.default_rng(13)
    refs = [rng.integers(1, 5, size=n).tolist() for n in (100, 37, 0, 520, 64)]
    queries = [_mutate(rng, r, 0.2, 4) for r in refs]
    for free in (True, False):
        one = _align(refs, queries, R.EMBOSS, free, ref_width=700, query_width=777, fill=3)
        two = _align(refs, queries, R.EMBOSS, free, ref_width=700, query_width=777, fill=-123456789)
        for u, v in zip(one, two):
            assert np.array_equal(u, v)
        _check_batch(refs, queries, R.EMBOSS, free, one, "padding")


def test_bad_lengths_poison_only_their_own_row():
    W = _W()
    W.check_device_flags()
    rng = np.random.default_rng(14)
    refs = [rng.integers(1, 5, size=n).tolist() for n in (40, 40, 40, 40, 40, 40)]
    queries = [_mutate(rng, r, 0.2, 4)[:44] for r in refs]
    a, an = _pad(refs, 40)
    b, bn = _pad(queries, 44)
    an[1], bn[3], an[4] = -1, 45, 41                                 # negative, above its maximum (twice)
    out = W.pairwise_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV))
    with pytest.raises(RuntimeError, match="3 pair"):
        W.check_device_flags()
    for n in (1, 3, 4):
        assert float(out.score[n]) == INT_MIN / 2
        assert (out.matches[n], out.mismatches[n], out.gaps[n], out.length[n]) == (-1, -1, -1, -1)
        assert int(out.ops_len[n]) == 0 and (out.ops[n] == 0).all()
    good = [0, 2, 5]
    stats = torch.stack([out.matches, out.mismatches, out.gaps, out.length], dim=1).cpu().numpy()
    for n in good:
        _check_pair(refs[n], queries[n], R.EMBOSS, True, int(float(out.score[n]) * 2), stats[n], out.ops[n].cpu().numpy(),
                    int(out.ops_len[n]), "good[%d]" % n)
    d = W.edit_distance(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV))
    with pytest.raises(RuntimeError, match="3 pair"):
        W.check_device_flags()
    assert [d[n].item() for n in (1, 3, 4)] == [-1, -1, -1]
    assert [d[n].item() for n in good] == [R.levenshtein(refs[n], queries[n]) for n in good]


def test_int64_and_int32_inputs_and_strided_rows():
    W = _W()
    rng = np.random.default_rng(15)
    refs = [rng.integers(1, 5, size=n).tolist() for n in (90, 33, 70)]
    queries = [_mutate(rng, r, 0.2, 4) for r in refs]
    a, an = _pad(refs)
    b, bn = _pad(queries)
    base = W.pairwise_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV))
    wide = W.pairwise_align(a.long().to(DEV), an.long().to(DEV), b.long().to(DEV), bn.long())    # host lengths are taken too
    beams = torch.zeros(3, 4, b.shape[1], dtype=torch.int32, device=DEV)                         # [B][W][T] as ctc_beam_decode's
    beams[:, 2] = b.to(DEV)
    view = W.pairwise_align(a.to(DEV), an.to(DEV), beams[:, 2], bn.to(DEV))                      # a row-strided view, in place
    torch.cuda.synchronize()
    for other in (wide, view):
        for u, v in zip(base, other):
            assert torch.equal(u, v)
    stats = torch.stack([base.matches, base.mismatches, base.gaps, base.length], dim=1).cpu().numpy()
    _check_batch(refs, queries, R.EMBOSS, True, ((base.score.double() * 2).cpu().numpy().astype(np.int64), stats, base.ops.cpu().numpy(),
                                                 base.ops_len.cpu().numpy()), "dtype")
    W.check_device_flags()


def test_two_runs_are_bitwise_identical_and_the_inputs_are_untouched():
    W = _W()
    rng = np.random.default_rng(16)
    refs = [rng.integers(1, 3, size=n).tolist() for n in (400, 380, 10, 0, 700, 390, 410, 64)]
    queries = [_mutate(rng, r, 0.2, 2) for r in refs]
    a, an = _pad(refs)
    b, bn = _pad(queries)
    a, an, b, bn = a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV)
    keep_a, keep_b = a.clone(), b.clone()
    r1 = W.pairwise_align(a, an, b, bn)
    r2 = W.pairwise_align(a, an, b, bn)
    torch.cuda.synchronize()
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert torch.equal(a, keep_a) and torch.equal(b, keep_b)
    W.check_device_flags()


def test_cpu_tensors_and_bad_arguments_raise():
    W = _W()
    a, an = _pad([[1, 2, 3], [2, 2]])
    b, bn = _pad([[1, 3], [2]])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        W.pairwise_align(a, an, b, bn)
    ad, bd = a.to(DEV), b.to(DEV)
    for bad in ({"gap_extend": 0.25}, {"match": 1.3}, {"gap_open": 0.5, "gap_extend": 1.0}, {"gap_open": 513}, {"mismatch": -600},
                {"gap_extend": -0.5}):
        with pytest.raises(ValueError, match="multiple of 0.5|need 0 <="):
            W.pairwise_align(ad, an, bd, bn, **bad)
    with pytest.raises(ValueError, match="int32 or int64"):
        W.pairwise_align(ad.float(), an, bd, bn)
    with pytest.raises(ValueError, match="same number of rows"):
        W.pairwise_align(ad, an, bd[:1], bn[:1])
    with pytest.raises(ValueError, match="query_lengths"):
        W.pairwise_align(ad, an, bd, bn[:1])
    with pytest.raises(ValueError, match="at most"):
        W.pairwise_align(ad, an, torch.ones(2, 8193, dtype=torch.int32, device=DEV), bn)
    W.check_device_flags()


# --------------------------------------------------------------------------------------------------------------- 6. end to end

def _collapse(path):
    out, prev = [], 0
    for v in path:
        if v != prev and v != 0:
            out.append(int(v))
        prev = v
    return out


def test_end_to_end_greedy_decode_then_align_on_the_device():
    W = _W()
    B, C, T = 4, 5, 1200
    x, path = _peaked_logits(60, B, C, T, margin=3.5)                # a weak margin: the noise wins some frames, reads have errors
    planted = [_collapse(path[b]) for b in range(B)]
    targets, target_lengths = _pad(planted, dtype=torch.int64)       # as given to ctc_forced_align
    targets, target_lengths = targets.to(DEV), target_lengths.to(DEV)
    labels, lengths, _ = W.ctc_greedy_decode(x.to(DEV))
    out = W.pairwise_align(targets, target_lengths, labels, lengths)         # labels [B][T] int32 as decoded, in place
    torch.cuda.synchronize()
    reads = [labels[b, :int(lengths[b])].cpu().tolist() for b in range(B)]
    assert any(r != p for r, p in zip(reads, planted)), "the reads have no errors: nothing to align"
    stats = torch.stack([out.matches, out.mismatches, out.gaps, out.length], dim=1).cpu().numpy()
    _check_batch(planted, reads, R.EMBOSS, True, ((out.score.double() * 2).cpu().numpy().astype(np.int64), stats, out.ops.cpu().numpy(),
                                                  out.ops_len.cpu().numpy()), "e2e")
    ident = out.identity.cpu()
    print("identity per read:", ["%.3f" % v for v in ident.tolist()])
    for b in range(B):
        top, mid, bottom = W.format_alignment(targets[b], labels[b], out.ops[b])
        n = int(out.length[b])
        assert len(top) == len(mid) == len(bottom) == n
        assert mid.count("|") == int(out.matches[b]) and mid.count(".") == int(out.mismatches[b])
        assert top.count("-") + bottom.count("-") == int(out.gaps[b])
        assert top.replace("-", "") == W.labels_to_strings(targets[b:b + 1], target_lengths[b:b + 1])[0]
        assert bottom.replace("-", "") == W.labels_to_strings(labels[b:b + 1], lengths[b:b + 1])[0]
    d = W.edit_distance(targets, target_lengths, labels, lengths)
    assert d.cpu().tolist() == [R.levenshtein(p, r) for p, r in zip(planted, reads)]
    W.check_device_flags()
