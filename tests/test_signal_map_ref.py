"""CPU: the host reference of the signal mapping (tests/signal_map_ref.py) held to things it shares no code with: the minimum over
every start and segmentation by brute force, a case worked by hand, the two tie cases, the cost of the path that signal_align's
reference recovers on the mapped span, the strand arithmetic against a string search, the runner-up rule on block tables written
down here, and the 24-read fixture, on which the reference itself must find every read."""
import itertools
import random

import numpy as np

from tests import signal_align_ref as AR
from tests import signal_map_cases as C
from tests import signal_map_ref as R


def _brute(q, ref, model, S, max_cost):
    """per end state: (cost, origin) of the best path over every start and every stay / step sequence, or None.  Among paths of
    equal cost the one whose moves, read from the last sample backwards, stay longest wins: the tie rule of the definition"""
    T, M = len(q), len(ref)
    out = []
    for e in range(M):
        best = None
        for moves in itertools.product((0, 1), repeat=T - 1):
            s = e - sum(moves)
            if s < 0:
                continue
            states = [s + sum(moves[:t]) for t in range(T)]
            if any(ref[j] == 0 for j in states):
                continue
            cost = sum(AR.sample_cost(q[t], *model[ref[j] - 1], S, max_cost) for t, j in enumerate(states))
            key = (cost, tuple(reversed(moves)))
            if best is None or key < best[0]:
                best = (key, s)
        out.append(None if best is None else (best[0][0], best[1]))
    return out


def test_against_brute_force():
    """T <= 7, M <= 9, k = 1 (a state is a base, a 0 is a wall), 102 random integer tables; every third is built to tie (two levels,
    samples on a level or half way between)"""
    rng = random.Random(3)
    ties = 0
    for n in range(102):
        T, M = rng.randint(1, 7), rng.randint(1, 9)
        tie = n % 3 == 0
        if tie:
            model = [[64 * (1 + (i & 1)), 1 << 16, 0] for i in range(4)]
            q = [rng.choice((64, 96, 128)) for _ in range(T)]
        else:
            model = [[rng.randint(-200, 200), rng.randint(1, 1 << 18), rng.randint(-50, 50)] for _ in range(4)]
            q = [rng.randint(-250, 250) for _ in range(T)]
        ref = [rng.choice((0, 1, 2, 3, 4, 1, 2, 3, 4)) for _ in range(M)]
        max_cost = rng.choice((2 ** 31 - 1, 3000))
        want = _brute(q, ref, model, 16, max_cost)
        got = R.signal_map_ref(np.array([q + [7]], dtype=np.float32), [T], ref, model, 1, frac_bits=0, weight_shift=16, max_cost=max_cost)
        codes, _ = R.prepare(ref, model, 1)
        D, O = R.last_row(q, codes, model, 16, max_cost)
        finite = [w for w in want if w is not None]
        for e, w in enumerate(want):
            assert (int(D[e]) >= R.INF) == (w is None)
            if w is not None:
                assert (int(D[e]), int(O[e])) == w, (n, e)
                assert got["end_cost"][0, e] == w[0]
            else:
                assert got["end_cost"][0, e] == R.NO_MAPPING
        if not finite:
            assert got["score"][0] == R.NO_MAPPING and got["end"][0] == -1 and got["start"][0] == -1
            continue
        low = min(c for c, _ in finite)
        end = next(e for e, w in enumerate(want) if w is not None and w[0] == low)
        ties += sum(1 for c, _ in finite if c == low) > 1
        assert (got["score"][0], got["end"][0], got["start"][0]) == (low, end, want[end][1])
        assert got["runner_up"][0] == R.NO_MAPPING                  # one block: nothing lies T states away
    assert ties >= 10


def test_case_worked_by_hand():
    """levels 10 20 30 40 10, cost d^2, samples 20 21 30 29.  Rows by hand:
        t0  100   0 100 400 100
        t1  221   1  81 461 221     (state 2 steps from state 1: 81 + 0)
        t2  621 101   1 181 621     (state 2 steps again: 0 + 1)
        t3  982 182   2 122 542     origins 0 1 1 1 1"""
    got = C.reference("hand")
    assert got["end_cost"][0].tolist() == [982, 182, 2, 122, 542]
    assert (got["score"][0], got["end"][0], got["start"][0], got["runner_up"][0]) == (2, 2, 1, R.NO_MAPPING)
    assert got["block_cost"][0].tolist() == [2] and got["block_end"][0].tolist() == [2] and got["bad"] == 0
    case = C.CASES["hand"]
    codes, _ = R.prepare(case.ref, case.model, 1)
    assert R.last_row([20, 21, 30, 29], codes, case.model, 16, 2 ** 31 - 1)[1].tolist() == [0, 1, 1, 1, 1]


def test_ties():
    got = C.reference("homopolymer")                                 # every cell of the last row is equal: the smallest end, no step
    for b in range(2):
        assert len(set(got["end_cost"][b].tolist())) == 1 and (got["end"][b], got["start"][b]) == (0, 0)
    assert got["runner_up"][0] == got["score"][0] and got["runner_up"][1] == got["score"][1]
    got, case = C.reference("two_copies"), C.CASES["two_copies"]     # two identical copies of a locus: the left one wins
    for b in range(2):
        e = int(got["end"][b])
        assert 200 <= got["start"][b] <= e < 350 and abs(int(got["start"][b]) - int(case.truth[b])) <= 2
        assert got["end_cost"][b, e + 2300] == got["score"][b]
    assert got["runner_up"][0] == got["score"][0]                    # the other copy is the runner-up, at the same cost


def test_score_is_the_cost_of_the_path_signal_align_recovers():
    """labels() of a mapping, aligned end to end by tests/signal_align_ref with no band: the same score, and the segmentation it
    returns costs that much when it is summed state by state"""
    for name in ("sweep_4100", "seam_walls", "form_k5", "form_k1", "cost_clamp"):
        case, got = C.CASES[name], C.reference(name)
        k, kw = case.kw["k"], case.kw
        for b in range(len(case.signal_lengths)):
            s, e, T = int(got["start"][b]), int(got["end"][b]), int(case.signal_lengths[b])
            assert 0 <= e - s <= T - 1
            labels = case.ref[s:e + k][None, :]
            al = AR.signal_align_ref(case.signal[b:b + 1], [T], labels, [e + k - s], case.model, k=k, first=0, frac_bits=kw["frac_bits"],
                                     weight_shift=kw["weight_shift"], max_cost=kw["max_cost"], band=None)
            assert al["score"][0] == got["score"][b], (name, b)
            q = AR.read_samples(case.signal[b], T, None, kw["frac_bits"])
            codes = AR.read_states(labels[0], e + k - s, k, 0)
            max_cost = 2 ** 31 - 1 if kw["max_cost"] is None else kw["max_cost"]
            assert AR.rescore(q, codes, case.model, kw["weight_shift"], max_cost, al["starts"][0]) == got["score"][b]


def test_strands_against_a_string_search():
    rng = random.Random(9)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    text = "".join(rng.choice("ACGT") for _ in range(500))
    bases = ["ACGT".index(c) + 1 for c in text]
    joined = R.join_strands(bases)
    assert len(joined) == 1001 and joined[500] == 0
    assert "".join("NACGT"[v] for v in joined[501:]) == "".join(comp[c] for c in reversed(text))
    assert R.join_strands([1, 0, 7, 4]) == [1, 0, 7, 4, 0, 1, 7, 0, 4]
    R_, k = 500, 5
    for _ in range(200):
        start = rng.randrange(0, 1001 - 40)
        end = start + rng.randrange(0, 30)
        if start <= 500 <= end + k - 1:
            continue                                                 # a path never crosses the joint
        read = "".join("NACGT"[v] for v in joined[start:end + k])
        lo, hi = R.ref_span_of(start, end, R_, k)
        if R.strand_of(end, R_) == 0:
            assert end + k - 1 < 500 and text[lo:hi] == read
        else:
            assert start > 500 and "".join(comp[c] for c in reversed(text[lo:hi])) == read
        assert hi - lo == end + k - start
    assert R.ref_span_of(-1, -1, R_, k) == (-1, -1) and R.strand_of(-1, R_) == -1
    assert R.ref_span_of(501, 996, R_, k) == (0, 500) and R.ref_span_of(0, 495, R_, k) == (0, 500)


def test_runner_up_block_rule():
    """blocks of 64 end states; a block counts when all of it lies T or more states from `end`"""
    costs = [50, 40, 30, 20, 10]                                     # M = 320
    assert R.runner_up_of(costs, 0, 64) == 10                        # end at 0: blocks 1.. (64 g >= 64)
    assert R.runner_up_of(costs, 0, 65) == 10 and R.runner_up_of(costs[:2], 0, 65) == R.NO_MAPPING      # block 1 starts at 64 < 65
    assert R.runner_up_of(costs, 5, 60) == 10 and R.runner_up_of(costs[:2], 5, 60) == R.NO_MAPPING      # 64 < 65
    assert R.runner_up_of(costs, 319, 64) == 20                      # end at M - 1: blocks 0..3 (64 g + 63 <= 255)
    assert R.runner_up_of(costs, 319, 65) == 30                      # block 3 ends at 255 > 254
    assert R.runner_up_of(costs, 160, 33) == 10 and R.runner_up_of(costs[:4], 160, 33) == 40            # 127 <= 127, 256 >= 193: 0, 1, 4
    assert R.runner_up_of(costs, 160, 34) == 10 and R.runner_up_of(costs[:4], 160, 34) == 50            # block 1 ends at 127 > 126: 0, 4
    assert R.runner_up_of(costs[:3], 160, 97) == 50                  # block 0 alone (63 <= 63)
    assert R.runner_up_of(costs, 160, 400) == R.NO_MAPPING           # T above M: nothing is that far away
    got, case = C.reference("t_above_m"), C.CASES["t_above_m"]
    assert got["runner_up"].tolist() == [R.NO_MAPPING] * 4 and (got["score"] < R.INF).all()
    assert (got["end"] - got["start"] <= case.signal_lengths - 1).all() and (got["end"] < 40).all()
    got = C.reference("few_open_states")                            # 20 open states: 10 samples fit, 30 do too (stays)
    assert (got["start"] >= 100).all() and (got["end"] <= 119).all()
    got = C.reference("all_walls")
    assert got["score"].tolist() == [R.NO_MAPPING] * 2 and got["end"].tolist() == [-1, -1] and got["bad"] == 0
    assert (got["block_end"] == -1).all() and (got["block_cost"] == R.NO_MAPPING).all()


def test_faults():
    got = C.bad_reference()
    bad = np.array([name not in C.BAD_GOOD for name in C.BAD_READS])
    assert got["bad"] == int(bad.sum()) == 5
    assert (got["score"][bad] == AR.BAD_READ).all() and (got["runner_up"][bad] == AR.BAD_READ).all()
    assert (got["block_cost"][bad] == AR.BAD_READ).all() and (got["end_cost"][bad] == AR.BAD_READ).all()
    assert (got["end"][bad] == -1).all() and (got["block_end"][bad] == -1).all()
    empty = C.BAD_READS.index("good_empty")
    assert got["score"][empty] == R.NO_MAPPING and (got["end_cost"][empty] == R.NO_MAPPING).all()
    faulty = C.faulty_reference_case()
    codes, ref_bad = R.prepare(faulty.ref, faulty.model, 3)
    clean, none = R.prepare(np.where(faulty.ref == 7, 0, faulty.ref), C.A.table(3)[2], 3)
    zeroed = int(np.flatnonzero(faulty.model[:, 1] == 0)[0])
    assert none == 0 and ref_bad == 1 + int((clean == zeroed).sum()) and codes[40] == -1
    assert (codes[248:251] == -1).all() and ((codes == -1) == ((clean == -1) | (clean == zeroed))).all()


def test_fixture_is_found_by_the_reference():
    """the 24 reads of 120 bases cut from both strands of a 3000-base reference, their first 400 samples: the reference puts every
    start within 2 states of the stretch the read was generated from, on the right strand.  A condition on the fixture."""
    fx, got = C.fixture(), C.fixture_reference()
    assert got["bad"] == 0 and got["ref_bad"] == 0 and set(fx["strand"].tolist()) == {0, 1}
    off = got["start"].astype(np.int64) - fx["start_state"]
    ratio = [float(r) / float(s) for r, s in zip(got["runner_up"], got["score"])]
    print("start - truth:", off.tolist(), "runner-up / score: %.3f .. %.3f" % (min(ratio), max(ratio)))
    assert (np.abs(off) <= 2).all()
    assert [R.strand_of(int(e), 3000) for e in got["end"]] == fx["strand"].tolist()
    assert min(ratio) > 1.0
