"""CPU: the four host references (tests/pileup_ref.py, genotype_ref.py, leftalign_ref.py, quality_profile_ref.py) judge the rows of
tests/opwalk_cases.py alike.  That makes "one op row, one verdict" a property of the definitions; tests/test_gpu_opwalk.py holds
the four kernels, which follow the definition of a valid op row in csrc/wn_opscan.h, to these references."""
import numpy as np

from tests import opwalk_cases as K


def test_the_batch_holds_every_kind():
    t = K.batch()
    valid = K.rows_of(K.VALID)
    assert sorted((int(t.ops_len[b]), int(t.strand[b])) for b in valid) == sorted((n, s) for n in K.LENGTHS for s in (0, 1))
    assert len(K.rows_of(K.BAD)) == 11 and len(K.rows_of(K.STRAND_ONLY)) == 1 and len(K.rows_of(K.SKIPPED)) == 2
    poked = t.ops[K.rows_of(K.BAD)[:6]]                                # op 0, then op 5, at column 0, 256 and the last
    assert [int(poked[r, at]) for r, at in enumerate((0, 256, K.WIDTH - 1) * 2)] == [0, 0, 0, 5, 5, 5]
    assert int(((poked < 1) | (poked > 4)).sum()) == 6 and (t.ops_len[K.rows_of(K.BAD)[:6]] == K.WIDTH).all()
    assert int(t.ops_len.max()) == K.WIDTH + 1 and sorted(int(v) for v in t.strand[K.rows_of(K.STRAND_ONLY, K.SKIPPED)]) == [-1, 0, 2]


def test_the_four_references_judge_a_row_alike():
    t = K.batch()
    pile, evidence, aligned, profile = K.references()
    refused = K.rows_of(K.BAD, K.STRAND_ONLY)
    assert pile.used.tolist() == evidence.used.tolist()
    assert [b for b, u in enumerate(pile.used.tolist()) if u == -1] == refused
    assert [b for b, s in enumerate(aligned.settled.tolist()) if s == -1] == refused
    skipped = [b for b in range(len(t.kind)) if t.strand[b] < 0 or t.ref_len[b] == 0]
    assert set(K.rows_of(K.SKIPPED)) < set(skipped) and len(skipped) == 4                        # and the two rows without columns
    assert all(pile.used[b] == 0 and aligned.settled[b] == 1 and aligned.passes[b] == 0 for b in skipped)
    assert all(pile.used[b] == 1 for b in K.rows_of(K.VALID) if b not in skipped)
    on_strand_0 = [b for b in range(len(t.kind)) if t.strand[b] == 0]
    assert [b for b in on_strand_0 if profile["read_counts"][b, 0] == -1] == K.rows_of(K.BAD)
    assert all((profile["read_counts"][b] >= 0).all() for b in K.rows_of(K.STRAND_ONLY, K.SKIPPED))  # no strand there: valid rows
    assert pile.bad == evidence.bad == aligned.bad == len(refused) == 12 and profile["bad"] == len(K.rows_of(K.BAD)) == 11


def test_a_refused_row_adds_nothing_and_is_copied():
    t = K.batch()
    pile, evidence, aligned, profile = K.references()
    walked = [b for b, u in enumerate(pile.used.tolist()) if u == 1]
    aligned_columns = sum(int(((t.ops[b, :t.ops_len[b]] == 1) | (t.ops[b, :t.ops_len[b]] == 2)).sum()) for b in walked)
    assert int(pile.counts[:, :, :4].sum() + pile.counts[:, :, 5].sum()) == aligned_columns > 1000
    assert int(profile["read_counts"][[b for b in range(len(t.kind)) if b not in K.rows_of(K.BAD)], :2].sum()) > aligned_columns
    for b in K.rows_of(K.BAD, K.STRAND_ONLY, K.SKIPPED):
        assert np.array_equal(aligned.ops[b], t.ops[b]), b
    assert any(int(aligned.passes[b]) > 0 for b in walked)
    for b in K.rows_of(K.BAD):
        assert not profile["outcome"][b].any() and (profile["ref_index"][b] == -1).all(), b
