"""CPU: the inputs of tests/test_gpu_align_limits.py (tests/align_limits_cases.py) hold what they are there for -- asserted from
the references alone, before any device sees them -- and the closed forms used beyond the references' reach equal the references
at small sizes.

The coverage proof.  Both kernels trace their path back in chunks of 64 through a window of backpointers staged in LDS, and the
windows' sizes rest on "the path moves at most ..." arguments that are tight only on the steepest path.  forced_trace_windows and
pair_trace_windows below are plain models of the two trace loops with the kernels' index arithmetic written out; they take a
REFERENCE path and return which window offsets each chunk reads (and assert that none lies outside the window).  The first lookup
of a chunk sits at the window's high corner whatever the path is, so "a corner is reached" means here: ONE chunk reads both the
lowest and the highest offset.  The new cases do; the older random cases, one of each recomputed here, do not."""
import numpy as np
import pytest

from tests import align_limits_cases as C
from tests import ctc_align_ref as A
from tests import pairwise_align_ref as R

CHUNK = 64


# ================================================================================================================ the models
def forced_trace_windows(states):
    """csrc/wn_align.hip's trace over a path: per chunk (s_end, lowest word offset read, highest word offset read)"""
    states = [int(s) for s in states]
    nT, out = len(states), []
    s_end = states[-1]
    for t0 in range((nT - 1) // CHUNK * CHUNK, -1, -CHUNK):
        nf = min(CHUNK, nT - t0)
        w0 = max(s_end - (2 * CHUNK - 1), 0) >> 4
        s, offsets = s_end, []
        for f in range(nf - 1, -1, -1):
            assert s == states[t0 + f]
            offsets.append((s >> 4) - w0)                            # win[f * 9 + ((s >> 4) - w0)]
            s = states[t0 + f - 1] if t0 + f > 0 else s
        assert 0 <= min(offsets) and max(offsets) <= 8, (t0, s_end, offsets)
        out.append((s_end, min(offsets), max(offsets)))
        s_end = s
    return out


def pair_trace_windows(a, b, costs, free):
    """csrc/wn_pairalign.hip's trace over the reference's backpointers: per chunk (lowest step offset, highest, lowest thread
    offset, highest) of the 72 x 9 window, and the ops it walks back to front"""
    H, bp = R.fill(a, b, *costs, free)
    _, i0, j0 = R.end_cell(H, free)
    st, out, back = 0, [], []
    while i0 > 0 and j0 > 0:
        tj = (j0 - 1) // 8
        kbase, tbase = (i0 - 1) + tj - 71, tj - 8
        i, j, steps, threads = i0, j0, [], []
        for _ in range(CHUNK):
            if not (i > 0 and j > 0):
                break
            t = (j - 1) // 8
            steps.append(i - 1 + t - kbase)                          # win[(i - 1 + t - kbase) * 9 + (t - tbase)]
            threads.append(t - tbase)
            v = int(bp[i, j])
            if st == 0:
                st = v & 3
                if st != 0:
                    continue
                back.append(1 if a[i - 1] == b[j - 1] else 2)
                i, j = i - 1, j - 1
            elif st == 1:
                back.append(4)
                j -= 1
                if not v & 4:
                    st = 0
            else:
                back.append(3)
                i -= 1
                if not v & 8:
                    st = 0
        assert 0 <= min(steps) and max(steps) <= 71 and 0 <= min(threads) and max(threads) <= 8, (i0, j0)
        out.append((min(steps), max(steps), min(threads), max(threads)))
        i0, j0 = i, j
    return out, back[::-1]


def count_alignments(labels, T, blank=0):
    """how many paths align `labels` to T frames (float64, capped at 1e300: exact where it matters, at 0 and 1)"""
    ext = A.extended(labels, blank)
    skip = A._skip_mask(ext, blank)
    n = np.zeros(len(ext))
    n[:2] = 1.0
    for _ in range(1, T):
        m = n.copy()
        m[1:] += n[:-1]
        m[2:] += np.where(skip[2:], n[:-2], 0.0)
        n = np.minimum(m, 1e300)
    return n[-1] + (n[-2] if len(ext) > 1 else 0.0)


def longest_run_of_skips(states):
    best = run = 0
    for d in np.diff(states):
        run = run + 1 if d == 2 else 0
        best = max(best, run)
    return best


# ========================================================================================================= the forced aligner
STEEP = ["steep_one_wave"] + ["steep_L%d" % L for L in C.STEEP_WAVES]


@pytest.mark.parametrize("name", STEEP)
def test_steep_paths_are_the_only_alignment_and_every_step_is_the_predicted_one(name):
    case = C.forced(name)
    for b, (labels, Tb) in enumerate(zip(case.labels, case.input_lengths)):
        states, score, _ = C.forced_reference(name)[b]
        want = C.forced_states(labels)
        assert len(want) == Tb and count_alignments(labels, Tb) == 1.0, (name, b)
        assert np.array_equal(states, want) and np.isfinite(score), (name, b)
        repeats = sum(u == v for u, v in zip(labels, labels[1:]))
        assert Tb == len(labels) + repeats and (repeats > 0) == (b >= len(case.labels) // 2)
        steps = np.diff(states)
        assert (steps == 2).sum() == len(labels) - 1 - repeats and (steps == 1).sum() == 2 * repeats
    if name == "steep_one_wave":                                     # the last state takes all eight odd phases
        assert {int(C.forced_reference(name)[b][0][-1]) & 15 for b in range(8)} == {1, 3, 5, 7, 9, 11, 13, 15}


@pytest.mark.parametrize("name", ["lead_one_wave", "lead_waves"])
def test_planted_paths_wait_in_the_first_blank_and_then_skip_on_every_frame(name):
    case = C.forced(name)
    L, leads = C.LEAD_ONE_WAVE if name == "lead_one_wave" else C.LEAD_WAVES
    for b, d in enumerate(leads):
        states, score, _ = C.forced_reference(name)[b]
        assert states.tolist() == [0] * d + list(range(1, 2 * L, 2)) and score == 0.0
        assert count_alignments(case.labels[b], L + d) > 1.0         # a choice, decided by the values


@pytest.mark.parametrize("L", C.NEAR_STEEP)
def test_near_steepest_paths_have_a_choice_and_long_runs_of_skips(L):
    case = C.forced("near_L%d" % L)
    for b, slack in enumerate((1, 3)):
        states = C.forced_reference("near_L%d" % L)[b][0]
        assert count_alignments(case.labels[b], L + slack) > 1.0
        assert longest_run_of_skips(states) >= (L - 1) // (slack + 1)


def _old_exact_case():
    """utterance 0 of tests/test_gpu_align.py::test_exact_on_a_quarter_grid_ties_included, the same draws"""
    rng = np.random.default_rng(7)
    x = rng.integers(-24, 1, size=(6, 5, 512)) / 4.0
    labels = [rng.integers(1, 5, size=n).tolist() for n in [90, 90, 37, 1, 0, 60]][0]
    return x[0], labels


def test_the_forced_trace_window_is_walked_from_corner_to_corner():
    full, phases = [], set()
    for name in STEEP + ["lead_one_wave", "lead_waves"] + ["near_L%d" % L for L in C.NEAR_STEEP]:
        for b, (states, _, _) in enumerate(C.forced_reference(name)):
            for s_end, lo, hi in forced_trace_windows(states):
                if s_end >= 2 * CHUNK - 1:                           # the window is not clamped at state 0
                    if lo == 0:
                        assert hi >= 7
                        full.append((name, b, s_end & 15, hi))
                        phases.add(s_end & 15)
    # word offsets 0 and 8 in ONE chunk: 126 states down from a last state whose phase is not 15 (phase 15 starts in word 7)
    assert any(hi == 8 for _, _, _, hi in full) and any(hi == 7 for _, _, _, hi in full)
    assert phases == {1, 3, 5, 7, 9, 11, 13, 15}                     # every phase a label state can have
    assert {n for n, _, _, hi in full if hi == 8} >= {"lead_one_wave", "lead_waves"}       # one wave and several
    print("forced aligner: %d chunks walk their whole window, %d of them words 0..8" % (len(full), sum(hi == 8 for _, _, _, hi in full)))
    # the older exact case: recomputed, its chunks never leave the three highest words
    lp, labels = _old_exact_case()
    states, _, _ = A.viterbi_align(lp, labels)
    assert longest_run_of_skips(states) < 16
    old = [(lo, hi) for s_end, lo, hi in forced_trace_windows(states) if s_end >= 2 * CHUNK - 1]
    assert old and all(lo >= 5 for lo, _ in old), old
    # and neither do the random multi-wave cases (ties_L*, below; the same kind as the older tolerant tests): none reads word 0
    for L in sorted(C.TIE_SHAPES):
        w = [(lo, hi) for s_end, lo, hi in forced_trace_windows(C.forced_reference("ties_L%d" % L)[0][0]) if s_end >= 2 * CHUNK - 1]
        assert all(lo >= 1 for lo, _ in w), (L, min(w))


@pytest.mark.parametrize("L", sorted(C.TIE_SHAPES))
def test_multi_wave_cases_meet_exact_ties_in_a_state_that_reads_across_waves(L):
    name = "ties_L%d" % L
    case = C.forced(name)
    assert case.x.shape == (2, 5, C.TIE_SHAPES[L]) and [len(l) for l in case.labels] == [L, L // 3] and L >= 256   # more than one wave
    assert case.input_lengths[1] < case.input_lengths[0] == C.TIE_SHAPES[L]
    states = C.forced_reference(name)[0][0]
    margins = A.frame_margins(C.forced_lp(case, 0), case.labels[0], states)
    tied = margins == 0
    across = tied & (states % 512 < 8) & (states >= 512)             # owned by lane 0 of a wave other than wave 0
    print("L %d: %d tied frames, %d of them in a state owned by lane 0 of a later wave" % (L, tied.sum(), across.sum()))
    assert tied.sum() >= 1 and across.sum() >= 1


def test_every_forced_case_is_exact_in_float32():
    for name in C.FORCED:
        case = C.forced(name)
        assert case.x.dtype == np.float32 and 24 * case.x.shape[2] < 2 ** 24           # every sum of quarters is a float32
        finite = case.x[np.isfinite(case.x)]
        assert (finite * 4 == np.round(finite * 4)).all() and finite.min() >= -6 and finite.max() <= 0
        lengths = case.input_lengths or [case.x.shape[2]] * len(case.labels)
        assert len(lengths) == len(case.labels) == case.x.shape[0]
        for _, score, _ in C.forced_reference(name):
            assert np.isneginf(score) or np.float64(np.float32(score)) == score == round(score * 4) / 4


def test_time_edges_cover_the_chunk_boundaries_with_every_label_count():
    assert C.TIME_EDGES == (1, 63, 64, 65, 127, 128, 129, 4096)
    for T in C.TIME_EDGES:
        case = C.forced("time_T%d" % T)
        assert case.x.shape == (3, 5, T) and case.input_lengths is None
        assert [len(l) for l in case.labels] == [0, 1, min(T // 2, 300)]
        assert all(np.isfinite(score) for _, score, _ in C.forced_reference("time_T%d" % T)) or T == 1
    inside = C.forced("time_inside")
    assert inside.x.shape[2] == C.TIME_TENSOR > max(C.TIME_EDGES)
    assert sorted(set(inside.input_lengths)) == sorted(C.TIME_EDGES)
    assert [(len(l), T) for l, T in zip(inside.labels, inside.input_lengths)] == \
        [(n, T) for T in C.TIME_EDGES for n in (0, 1, min(T // 2, 300))]


def test_class_limits():
    for blank in (0, 1):
        case = C.forced("two_classes_blank%d" % blank)
        assert case.x.shape[1] == 2 and case.blank == blank and all(set(l) == {1 - blank} for l in case.labels)
        assert count_alignments(case.labels[0], 699, blank) == 1.0 and count_alignments(case.labels[1], 700, blank) > 1.0
        states = C.forced_reference("two_classes_blank%d" % blank)[0][0]
        assert states.tolist() == list(range(1, 700))                # label, blank, label, ...: every gap a forced blank
    for blank in (0, 63, 31):
        case = C.forced("classes64_blank%d" % blank)
        assert case.x.shape == (1, 64, 700) and len(case.labels[0]) == 300 and blank not in case.labels[0]
        assert len(set(case.labels[0])) > 50 and np.isfinite(C.forced_reference("classes64_blank%d" % blank)[0][1])


def test_neg_inf_cases():
    case = C.forced("neg_inf")
    ref = C.forced_reference("neg_inf")
    # 0: confined to the band, and an alignment still fits
    holes = np.isneginf(case.x[0])
    assert not holes[0].any() and holes[1:].mean() > 0.05
    states, score, _ = ref[0]
    assert np.isfinite(score)
    on = A.frame_labels_of(states, case.labels[0])
    assert not holes[on, np.arange(700)].any()
    # 1: no alignment at all
    assert np.isneginf(case.x[1, case.labels[1][17]]).all()
    assert np.isneginf(ref[1][1]) and (ref[1][0] == -1).all() and (ref[1][2] == -1).all()
    # 2: the holes lie beside the path, which is the path of the finite values
    holes = np.isneginf(case.x[2])
    assert holes.sum() > 2000
    rng = np.random.default_rng(500)
    finite = C.grid(rng, (3, 16, 700))[2].astype(np.float64)
    assert np.array_equal(finite[~holes], case.x[2][~holes])
    want = A.viterbi_align(finite, case.labels[2])
    assert np.array_equal(ref[2][0], want[0]) and ref[2][1] == want[1]


# ======================================================================================================= the pairwise aligner
SELF = ["self_%s/%s" % (g, c) for g in sorted(C.SELF_GROUPS) for c in ("emboss", "largest")]


def test_self_sizes_are_the_ones_the_window_argument_needs():
    sizes = C.SELF_ONE_WAVE + C.SELF_WAVES + C.SELF_LONG
    assert set(sizes) == {1, 8, 63, 64, 65, 71, 72, 73, 128, 512, 513, 1100} | set(range(520, 528))
    assert {(n - 1) % 8 for n in range(520, 528)} == set(range(8))   # every column phase of the end cell
    assert max(C.SELF_ONE_WAVE) <= 512 < min(C.SELF_WAVES)           # one wave / several


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("name", SELF)
def test_a_row_against_itself_is_all_matches(name, free):
    case = C.pairs(name)
    for n, row in enumerate(case.refs):
        want = C.pair_reference(name, n, free)
        assert case.queries[n] == row and (want.ops == 1).all() and want.length == len(row)
        assert want == C.identical_result(len(row), case.costs)[:5] + (want.ops,)


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("name", ["variants_200/emboss", "variants_200/largest", "variants_600/emboss"])
def test_variants_are_a_diagonal_with_one_mismatch_or_one_head_gap(name, free):
    case = C.pairs(name)
    n = int(name.split("/")[0].split("_")[1])
    for k, d in enumerate(C.PLANTED):
        ops = C.pair_reference(name, k, free).ops
        assert len(ops) == n and ops[n - d] == 2 and (np.delete(ops, n - d) == 1).all()
    for k, s in enumerate(C.SHIFTS):
        for m, gap in ((0, 3), (1, 4)):                              # the reference is the longer row, then the query
            ops = C.pair_reference(name, len(C.PLANTED) + 2 * k + m, free).ops
            assert len(ops) == n and (ops == 1).sum() == n - s and (ops == gap).sum() == s
            assert (ops[-(n - s - 20):] == 1).all()                  # the gap lies in the head: a long diagonal from the end cell


def _old_random_case():
    """pair 0 of tests/test_gpu_pairalign.py::test_random_pairs[mutated4-emboss-True], the same draws"""
    rng = np.random.default_rng(1 * 10 + 4 + 100)                    # "emboss" is the second of the sorted cost sets
    refs = [rng.integers(1, 5, size=n).tolist() for n in [300, 257, 120, 64, 33, 8, 1, 200]]
    return refs[0], C.mutate(rng, refs[0], rng.uniform(0.10, 0.25), 4)


def test_the_pairwise_trace_window_is_walked_from_corner_to_corner():
    corners = set()
    for name in ("self_one_wave/emboss", "self_waves/largest", "variants_200/emboss"):
        case = C.pairs(name)
        for n, (a, b) in enumerate(zip(case.refs, case.queries)):
            for free in (True, False):
                windows, _ = pair_trace_windows(a, b, case.costs, free)
                for lo_k, hi_k, lo_t, hi_t in windows:
                    if (lo_k, hi_k, lo_t, hi_t) == (0, 71, 0, 8):
                        corners.add((name, (len(b) - 1) % 8))                        # the column phase of the end cell
    # step offsets 0 and 71 and thread offsets 0 and 8 in ONE chunk: 63 diagonal moves from a column whose phase is not 7
    assert {n for n, _ in corners} == {"self_one_wave/emboss", "self_waves/largest", "variants_200/emboss"}
    assert {p for n, p in corners if n == "self_waves/largest"} >= set(range(7))
    # the model walks what the reference walks
    case = C.pairs("variants_200/emboss")
    for n in (0, 5, 6):
        _, ops = pair_trace_windows(case.refs[n], case.queries[n], case.costs, False)
        want = C.pair_reference("variants_200/emboss", n, False).ops.tolist()
        assert ops == want[len(want) - len(ops):] and set(want[:len(want) - len(ops)]) <= {3, 4}
    # the older random case, recomputed: no chunk comes near step 0 of its window
    a, b = _old_random_case()
    windows, _ = pair_trace_windows(a, b, R.EMBOSS, True)
    assert len(windows) >= 4 and min(lo_k for lo_k, _, _, _ in windows) >= 3, windows
    assert all((lo_k, lo_t) != (0, 0) for lo_k, _, lo_t, _ in windows)


def test_cost_sets_sit_on_the_limits_the_wrapper_accepts():
    sets = [C.COSTS[k] for k in C.COST_LIMIT_SETS]
    assert sets == [(1024, -1024, 1024, 1024), (1024, -1024, 1024, 0), (0, 0, 0, 0), (-1024, 1024, 1024, 0), (5, 5, 3, 1)]
    assert all(0 <= ge <= go <= 1024 and abs(ma) <= 1024 and abs(mi) <= 1024 for ma, mi, go, ge in sets)
    row, same = C.identical_rows(1100)
    assert R.score_only(row, same, *sets[0], True) == 1126400 and R.score_only(row, same, *sets[2], True) == 0
    for size in (300, 1100):
        for k in C.COST_LIMIT_SETS:
            case = C.pairs("costs_%d/%s" % (size, k))
            assert [len(r) for r in case.refs] == [size] * 4 and all(abs(len(q) - size) <= size // 8 for q in case.queries)
            assert [max(r) for r in case.refs] == [2, 2, 4, 4]
    for free in (True, False):                                       # far inside int32, and inside the kernel's own bound of 2^27
        scores = [C.pair_reference("costs_300/%s" % k, n, free).score for k in C.COST_LIMIT_SETS for n in range(4)]
        assert max(abs(s) for s in scores) < 2 ** 27 and len(set(scores)) > 10


def test_ring_cases_reload_the_reference_ring_in_one_wave_and_in_several():
    reloads = {}
    for N in C.RING_N:
        case = C.pairs("ring_N%d" % N)
        assert [len(r) for r in case.refs] == [N] * 3 and [len(q) for q in case.queries] == list(C.RING_M)
        for M in C.RING_M:
            nsteps = N + (M + 7) // 8 - 1
            reloads[(N, M)] = (nsteps - 1) // 1024                   # reloads after the first: at k = 1024, 2048, ...
    assert reloads[(1023, 8)] == 0 and reloads[(1024, 8)] == 0 and reloads[(1025, 8)] == 1        # the edge, in one wave
    assert reloads[(1023, 1100)] == 1 and reloads[(2048, 8)] == 1 and reloads[(2049, 8)] == 2 and reloads[(4100, 1100)] == 4
    assert sorted(set(reloads.values())) == [0, 1, 2, 3, 4]
    wide, waves = C.pairs("threads_1100x8192"), C.pairs("waves_2100x4104")
    assert (len(wide.refs[0]), len(wide.queries[0])) == (1100, 8192) and 1100 + 1024 - 1 > 2048   # 1024 threads, two reloads
    assert (len(waves.refs[0]), len(waves.queries[0])) == (2100, 4104) and (4104 + 7) // 8 == 513
    assert C.pair_reference("threads_1100x8192", 0, True).matches > 800                          # the stretch is found


@pytest.mark.parametrize("free", [True, False])
def test_closed_forms_equal_the_reference_at_small_sizes(free):
    for costs in (R.EMBOSS, C.COSTS["largest"]):
        for n in (1, 2, 64, 65, 300, 600):
            row, same = C.identical_rows(n)
            want, got = R.align(row, same, *costs, free), C.identical_result(n, costs)
            assert want[:5] == got[:5] and np.array_equal(want.ops, got.ops)
    for N, M in ((1, 1), (5, 5), (9, 4), (40, 8), (70, 33), (300, 64), (600, 75)):
        a, b = C.unequal_rows(N, M)
        assert R.score_only(a, b, *C.UNEQUAL_COSTS, free) == C.unequal_score(N, M, free), (N, M)
        if free:
            assert np.array_equal(R.align(a, b, *C.UNEQUAL_COSTS, True).ops, C.unequal_free_ops(N, M))
        a, b = C.equal_rows(N, M)
        assert R.score_only(a, b, *C.EQUAL_COSTS, free) == C.equal_score(N, M, free), (N, M)
    N, M = C.LONGEST
    assert (N, M) == (65535, 8192) and abs(C.unequal_score(N, M, False)) < 2 ** 27 and C.equal_score(N, M, False) == 1024 * (2 * M - N)


# ========================================================================================================= the quality profile
def test_synthetic_op_strings_sit_on_both_length_limits():
    N, M = C.LONGEST
    for kind, columns, aligned in (("longest", N + M, 0), ("mixed", N + M - 8000, 8000)):
        ops, ref, query = C.synthetic_ops(kind)
        assert len(ops) == columns and len(ref) == N and len(query) == M and int(np.isin(ops, (1, 2)).sum()) == aligned
        assert R.replay(ref, query, ops) == (ref, query)
    ops, ref, query = C.synthetic_ops("mixed")
    qual, dwell = C.profile_inputs(660, M)
    want = C.profile_reference(ops, ref, query, qual, dwell, False)
    assert want["bad"] == 0 and want["read_counts"][0, :2].tolist() == [7000, 1000] and int(want["q_counts"].sum()) > 8000
