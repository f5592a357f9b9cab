"""CPU: the numpy reference of pairwise alignment (tests/pairwise_align_ref.py), which the GPU tests compare against bit for
bit, held to three things it does not share code with: exhaustive enumeration of every global alignment of short sequences,
the textbook Levenshtein recurrence, and the EMBOSS needle results recorded in the reference's evaluation notebook
(tests/golden/emboss_pairs.json, written by tests/golden/make_emboss_pairs.py)."""
import itertools
import json
import os
import time

import numpy as np
import pytest

from tests import pairwise_align_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emboss_pairs.json")
BASES = {"A": 1, "G": 2, "C": 3, "T": 4}            # decoding.DEFAULT_ALPHABET

# needle's costs in half units, and a set with cheap gaps and gap_open == gap_extend where other alignments win
COST_SETS = [R.EMBOSS, (2, -3, 2, 2)]


def _sequences(max_len):
    for n in range(max_len + 1):
        for s in itertools.product((1, 2), repeat=n):
            yield list(s)


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", COST_SETS)
def test_against_exhaustive_enumeration(costs, free):
    """every pair with N, M <= 4 over a 2-letter alphabet: the DP score is the best over ALL alignments, and the reference's
    own ops spell both sequences and rescore to it"""
    seqs = list(_sequences(4))
    assert len(seqs) == 31
    for a in seqs:
        for b in seqs:
            want = R.best_score_by_enumeration(a, b, *costs, free)
            got = R.align(a, b, *costs, free)
            assert got.score == want, (a, b, got.score, want)
            ra, rb = R.replay(a, b, got.ops)
            assert ra == a and rb == b, (a, b, got.ops)
            assert R.rescore(got.ops, *costs, free) == want, (a, b, got.ops)
            assert got.length == len(got.ops) == got.matches + got.mismatches + got.gaps
            assert R.score_only(a, b, *costs, free) == want


def test_unit_costs_give_the_levenshtein_distance():
    rng = np.random.default_rng(0)
    for n in range(200):
        alphabet = 2 if n % 2 else 4
        a = rng.integers(1, alphabet + 1, size=int(rng.integers(0, 40))).tolist()
        b = rng.integers(1, alphabet + 1, size=int(rng.integers(0, 40))).tolist()
        want = R.levenshtein(a, b)
        got = R.align(a, b, *R.UNIT, False)
        assert -got.score == want, (a, b)
        assert got.mismatches + got.gaps == want                      # every edit is one column of the alignment
        assert R.replay(a, b, got.ops) == (a, b)


def _golden():
    doc = json.load(open(GOLDEN))
    assert len(doc["pairs"]) == 12
    return doc["pairs"]


def _labels(s):
    return [BASES[c] for c in s]


# what was found when the recorded results were first compared with this rule (indices into the 12 pairs)
SCORE_EQUAL = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]       # pair 0: needle shows 222.5 where the optimum is 223.5
SHAPE_EQUAL = [1, 2, 3, 4, 5, 6, 7, 8, 10, 11]          # pair 9: an equally scoring alignment of another shape (59/112 for 58/115)


def test_recorded_emboss_needle_results():
    pairs = _golden()
    for n, p in enumerate(pairs):
        a, b = _labels(p["true"]), _labels(p["pred"])
        got = R.align(a, b, *R.EMBOSS, True)
        print("pair %2d: needle score %.1f identity %d/%d gaps %d; reference score %.1f identity %d/%d gaps %d"
              % (n, p["score"], p["identity"], p["length"], p["gaps"], got.score / 2, got.matches, got.length, got.gaps))
        assert R.replay(a, b, got.ops) == (a, b)
        assert R.rescore(got.ops, *R.EMBOSS, True) == got.score
        # an optimum cannot be below the score of any alignment that was shown
        assert got.score / 2 >= p["score"], n
        if n in SCORE_EQUAL:
            assert got.score / 2 == p["score"], n
        if n in SHAPE_EQUAL:
            assert (got.matches, got.length, got.gaps) == (p["identity"], p["length"], p["gaps"]), n
    first = R.align(_labels(pairs[0]["true"]), _labels(pairs[0]["pred"]), *R.EMBOSS, True)
    assert first.score / 2 == 223.5 and pairs[0]["score"] == 222.5
    tenth = R.align(_labels(pairs[9]["true"]), _labels(pairs[9]["pred"]), *R.EMBOSS, True)
    assert (tenth.matches, tenth.length) == (59, 112) and (pairs[9]["identity"], pairs[9]["length"]) == (58, 115)


def test_the_reference_is_quick_enough_for_the_gpu_tests():
    """8 pairs of 512 x 512 in a couple of seconds: the anti-diagonal fill, not a cell loop"""
    rng = np.random.default_rng(1)
    seqs = [(rng.integers(1, 5, size=512).tolist(), rng.integers(1, 5, size=512).tolist()) for _ in range(8)]
    t = time.perf_counter()
    for a, b in seqs:
        r = R.align(a, b)
        assert R.replay(a, b, r.ops) == (a, b)
    took = time.perf_counter() - t
    print("8 pairs of 512 x 512: %.2f s" % took)
    assert took < 10.0                                                # a cell loop takes minutes
