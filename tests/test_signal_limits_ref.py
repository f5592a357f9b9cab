"""CPU: the inputs of tests/test_gpu_signal_limits.py (tests/signal_limits_cases.py) hold what they are there for -- asserted from
the references alone, before any device sees them -- and the numpy-vectorised reference of the event tables equals the plain loop
of tests/kmer_events_ref.py."""
import numpy as np
import pytest

from tests import kmer_events_cases as EC
from tests import kmer_events_ref as ER
from tests import signal_align_ref as AR
from tests import signal_limits_cases as C
from tests import signal_map_ref as MR


# ---- 1. the sample cost
def test_the_grid_holds_every_value_and_the_reference_every_kmer_once():
    model = C.grid_model()
    assert model.shape == (64, 3)
    assert set(model[:, 0].tolist()) == set(C.GRID_LEVELS) and set(model[:, 1].tolist()) == set(C.GRID_WEIGHTS)
    assert set(model[:, 2].tolist()) == set(C.GRID_OFFSETS)
    assert len({(l, w) for l, w, _ in model.tolist()}) == 36         # every (level, weight) pair
    for level in (C.Q_MAX, -C.Q_MAX):                                # the rows that decide the 79-bit product, under every offset
        assert {o for l, w, o in model.tolist() if l == level and w == C.WEIGHT_MAX} and len({o for l, w, o in model.tolist() if l == level}) == 3
    ref = C.grid_reference()
    codes, faults = MR.prepare(ref, model, C.GRID_K)
    assert len(ref) == 77 and faults == 0 and sorted(codes[:64].tolist()) == list(range(64))
    assert codes[64:67].tolist() == [-1] * 3 and (codes[67:] >= 0).all() and codes[67:].tolist() == codes[:8].tolist()
    q = C.grid_q()
    assert len(q) == 40 and {0, 1, -1, 1 << 16, -(1 << 16), 1 << 22, -(1 << 22), C.Q_MAX, -C.Q_MAX} <= set(q)
    for F in C.GRID_FRAC:                                            # both F quantise to the same q
        assert AR.read_samples(C.grid_signal(F)[:, 0], 40, None, F) == q
    sig, labels = C.grid_align_inputs(0)
    assert sig.shape == (2560, 2) and labels.shape == (2560, 3) and labels[64 + 27].tolist() == [2, 3, 4] and sig[64 + 27, 0] == q[1]
    assert [ER.kmer_index(row) for row in labels[:64].tolist()] == list(range(64))


def test_the_grid_reaches_the_high_half_of_the_product():
    products = C.grid_products()
    flat = [p for row in products for p in row]
    assert max(flat) == (2 ** 24 - 2) ** 2 * C.WEIGHT_MAX >= 2 ** 78            # d = 2^24 - 2, the largest there is
    assert sum(p >= 2 ** 64 for p in flat) > 200
    model = C.grid_model().tolist()
    reached = set()
    for S in C.GRID_SHIFTS:
        clamped = free = high_free = high_decides = negative = 0
        for mc in C.GRID_MAX_COSTS:
            costs = C.grid_costs(S, mc)
            for s in range(40):
                for c in range(64):
                    p, sh = products[s][c], products[s][c] >> S
                    assert costs[s][c] == min(sh, mc) + model[c][2]
                    clamped += sh >= mc
                    free += 0 < sh < mc
                    high_free += p >= 2 ** 64 and sh < mc                       # un-clamped, and hi != 0
                    high_decides += p >= 2 ** 64 and sh >= mc and ((p % 2 ** 64) >> S) < mc      # without hi it would not clamp
                    negative += costs[s][c] < 0
        assert clamped > 0 and free > 0 and negative > 0, S
        assert high_decides > 0, S
        if high_free:
            reached.add(S)
    assert reached == {47, 48, 62, 63}                               # p < 2^(31 + S) when un-clamped: 2^64 needs S >= 34
    assert C.grid_costs(63, C.COST_MAX)[7][1] == ((2 ** 24 - 2) ** 2 * 2 >> 63) + model[1][2]
    # the half-word seam: at S = 32 the result is the high word of lo joined to hi
    assert any(2 ** 64 <= p < 2 ** 64 + 2 ** 62 for p in flat)


def test_the_grid_references_agree_with_the_cost_matrix():
    codes, _ = MR.prepare(C.grid_reference(), C.grid_model(), C.GRID_K)
    for S, mc, F in ((16, C.COST_MAX, 0), (32, 12345, 20), (63, 1, 0), (48, C.COST_MAX, 20)):
        ref, costs = C.grid_map_reference(F, S, mc), C.grid_costs(S, mc)
        assert ref["bad"] == 0 and ref["ref_bad"] == 0
        for s in range(40):
            assert ref["end_cost"][s].tolist() == [costs[s][c] if c >= 0 else MR.NO_MAPPING for c in codes.tolist()]
            assert ref["score"][s] == min(costs[s]) and ref["start"][s] == ref["end"][s]


# ---- 2. quantisation
def test_quantisation_cases_hold_their_edges():
    want = [0, 2, 2, 0, -2, -2, 4194304, 4194306, -4194304, 8388606, -8388606, 1, 0, -1, 3, 0, C.Q_MAX, -C.Q_MAX, 8388606, 1000002, 0]
    for F in C.QUANT_FRAC:
        case = C.quant_f32_case(F)
        q = C.quant_expected_q(case)
        assert q[0] == want and q[2] == want[::-1] and q[5] == want
        assert [b for b, row in enumerate(q) if None in row] == list(C.QUANT_BAD_READS)
        assert [row.count(None) for row in q] == [0, 1, 0, 1, 1, 0]                  # one sample each, among good ones
        assert np.signbit(case.signal[0, 15]) and case.signal[0, 15] == 0 and 0 < case.signal[0, 20] < np.finfo(np.float32).tiny
        ref = C.quant_events_reference(case)
        assert ref["bad"] == 3 and ref["sum"][0].tolist() == want and (ref["length"][0] == 1).all()
    case = C.quant_i16_case()
    q = C.quant_expected_q(case)
    assert [b for b, row in enumerate(q) if None in row] == list(C.QUANT_I16_BAD_READS) and [row.count(None) for row in q] == [0, 0, 0, 0, 1, 1, 1, 0]
    assert q[2][4] == C.Q_MAX and q[3][0] == -C.Q_MAX and q[4][4] is None and q[5][0] is None and q[6][4] is None
    assert {-32768, -1, 1, 3, 32767} == set(case.signal[2].tolist())
    for b in (0, 1):                                                 # float32 arithmetic would land elsewhere, fused or not
        raw, scale, shift = C.QUANT_I16_READS[b]
        other = [C.quantise_in_float32(x, scale, shift, C.QUANT_I16_FRAC) for x in raw]
        assert any(q[b][i] != o[0] for i, o in enumerate(other)) and any(q[b][i] != o[1] for i, o in enumerate(other)), b
    assert C.quant_events_reference(case)["bad"] == 3
    cases = [C.quant_f32_case(F) for F in C.QUANT_FRAC] + [case]
    model = C.quant_model(cases)
    levels = model[:, 0].tolist()
    assert model.shape == (64, 3) and levels[0] == 0 and (model[:, 1] == 1 << 16).all() and not model[:, 2].any()
    for c in cases:                                                  # every sample has its own row, and a row one above it
        for row in C.quant_expected_q(c):
            assert all(v is None or v in levels for v in row)
    assert C.Q_MAX in levels and -C.Q_MAX in levels and -C.Q_MAX + 1 in levels and 4194305 in levels and 3 in levels
    costs = C.quant_costs(C.quant_f32_case(12), model)
    assert costs[21 + 7] is None and costs[16][levels.index(C.Q_MAX)] == 0 and costs[16][0] == C.COST_MAX and costs[14][0] == 9


# ---- 3. the largest event sums
def test_the_big_events_reach_the_limits_of_their_sums():
    case, ref = C.big_case(), C.big_reference()
    assert case.signal.shape == (2, 131138) and ref["bad"] == 0 and ref["length"].tolist() == [list(C.BIG_EVENTS)] * 2
    n = np.array(C.BIG_EVENTS, dtype=object)
    assert ref["sum"][0].tolist() == (-C.Q_MAX * n).tolist() and ref["sum"][1].tolist() == (C.Q_MAX * n).tolist()
    assert ref["sumsq"][0].tolist() == ref["sumsq"][1].tolist() == (C.Q_MAX ** 2 * n).tolist()
    assert 2 ** 62 - 2 ** 41 < int(ref["sumsq"][0, 0]) < 2 ** 62 and -2 ** 39 < int(ref["sum"][0, 0]) < -2 ** 39 + 2 ** 17
    row = ref["kmer_stats"][C.BIG_BASE - 1].tolist()
    squares = [int(v) for v in ref["sumsq"].ravel()]
    assert row == [10, 2 * 131138, 0, sum(v & 0xffffffff for v in squares), sum(v >> 32 for v in squares)]       # the sums cancel
    assert row[4] > 2 ** 32 and row[3] > 2 ** 32                     # several such events: each limb sum is past 32 bits
    assert ref["dwell_hist"][C.BIG_BASE - 1, 255] == 4 and ref["dwell_hist"][C.BIG_BASE - 1, [1, 32, 33]].tolist() == [2, 2, 2]
    twice = C.big_reference(twice=True)
    assert twice["kmer_stats"][C.BIG_BASE - 1].tolist() == [2 * v for v in row]
    import wavenet_speech_amd as W
    for read, sign in ((0, -1), (1, 1)):
        alone = C.big_reference(reads=(read,), max_dwell=65536)
        events, samples, s1, lo, hi = alone["kmer_stats"][C.BIG_BASE - 1].tolist()
        assert (events, samples, s1) == (5, 131138, sign * C.Q_MAX * 131138) and (hi << 32) + lo == C.Q_MAX ** 2 * 131138
        assert alone["dwell_hist"][C.BIG_BASE - 1, 65536] == 2 and alone["dwell_hist"].shape == (4, 65537)
        means, stdvs, counts = W.fit_kmer_model(alone["kmer_stats"], frac_bits=0, min_count=1)
        assert float(means[C.BIG_BASE - 1]) == s1 / samples == sign * C.Q_MAX and float(stdvs[C.BIG_BASE - 1]) == 0.0
        assert float(counts[C.BIG_BASE - 1]) == samples and bool(np.isnan(means.numpy()[[0, 1, 3]]).all())


# ---- 4. the table kernel across workgroups
def test_the_table_cases_fall_on_the_seams_they_are_for():
    assert C.table_grid(1) == (1, 256) and C.table_grid(4096) == (1, 4096) and C.table_grid(4097) == (2, 2304)
    blocks, chunk = C.table_grid(37 * 300)
    assert (blocks, chunk) == (3, 3840) and chunk // 300 == 12 and 2 * chunk // 300 == 25 and chunk % 300 and 2 * chunk % 300
    three = C.table_case("three")
    assert three.starts.shape == (37, 301) and three.bad_reads == (12, 30) and three.signal_lengths[30] == -1
    assert np.isnan(three.signal[12]).sum() == 1
    rows = 2050 * 513
    blocks, chunk = C.table_grid(rows)
    assert rows > 2 ** 20 and (blocks, chunk) == (256, 4352) and chunk > C.TABLE_CHUNK
    assert [w for w in range(256) if w * chunk >= rows] == list(range(242, 256))          # the workgroups with nothing to do
    cap = C.table_case("cap")
    assert cap.starts.shape == (2050, 514) and (np.diff(cap.starts, axis=1) == 1).all() and cap.signal.nbytes < 5 * 2 ** 20
    assert cap.bad_reads == (8, 848, 2044, 2049)
    for w, b in ((1, 8), (100, 848), (241, 2044)):                   # each seam falls inside its bad read
        assert b * 513 < w * chunk < (b + 1) * 513
    for name, kk in (("three", (2, 6)), ("cap", (1, 6))):
        for k in kk:
            ref = C.table_reference(name, k)
            case = C.table_case(name)
            assert ref["bad"] == len(case.bad_reads) and (ref["read_counts"][list(case.bad_reads)] == -1).all()
            assert (ref["kmer"][list(case.bad_reads)] == -4).all() and (np.delete(ref["read_counts"][:, 0], case.bad_reads) > 0).all()
            assert int(ref["kmer_stats"][:, 0].sum()) == int((ref["kmer"] >= 0).sum()) == int(ref["dwell_hist"].sum())
            assert (ref["kmer_stats"][:, 0] > 0).mean() > (0.9 if name == "cap" or k < 6 else 0.5)      # contention on every row
            assert 0 < ref["kmer_stats"][:, 2:].max() < 2 ** 62 and ref["kmer_stats"][:, 4].max() > 0
    assert (C.table_reference("cap", 6)["kmer"] == -1).sum() == 2 * (2050 - 4)             # windows that run off the labels


@pytest.mark.parametrize("k", sorted(C.TABLE_WINDOWS))
@pytest.mark.parametrize("name", ["three", "cap_small"])
def test_the_vectorised_table_reference_is_the_plain_loop(name, k):
    fast, plain = C.table_reference(name, k), C.table_plain_reference(name, k)
    assert plain["bad"] == len(C.table_case(name).bad_reads) > 1
    for key in fast:
        assert fast[key].dtype == plain[key].dtype if key != "bad" else True, key
        assert np.array_equal(fast[key], plain[key]), key


def test_the_vectorised_table_reference_on_the_event_cases():
    """the cases of tests/kmer_events_cases.py with frame_stride 1, both layouts and signal kinds: events of every length and code,
    gaps, reads cut by their length, and every kind of bad read"""
    for name, case in sorted(EC.CASES.items()):
        if "frame_stride" in case.kw:
            continue
        for layout in EC.LAYOUTS:
            begin, end, events = EC.segments(case, layout)
            for kind, F in (("f32", 12), ("i16", 0)):
                signal, ss = (case.signal, None) if kind == "f32" else EC.int16_form(name)
                kw = dict(dict(max_dwell=255), **case.kw)
                fast = C.fast_events_ref(signal, case.signal_lengths, case.labels, case.label_lengths, begin, end, events, scale_shift=ss,
                                         frac_bits=F, **kw)
                plain = EC.reference(name, layout, kind, F)
                assert all(np.array_equal(fast[key], plain[key]) for key in fast), (name, layout, kind)
    bad = EC.bad_batch()
    for layout in EC.LAYOUTS:
        _, begin, end, events = EC.bad_segments(layout)
        fast = C.fast_events_ref(bad.signal, bad.signal_lengths, bad.labels, bad.label_lengths, begin, end, events, frac_bits=12, **EC.BAD_KW)
        plain = EC.bad_reference(layout)
        assert all(np.array_equal(fast[key], plain[key]) for key in fast) and fast["bad"] == 12, layout


# ---- 5. long paths
@pytest.mark.parametrize("which", ["costly", "cheap"])
def test_the_long_mapping_is_as_long_and_as_costly_as_it_can_be(which):
    case, ref = C.map_long_case(which), C.map_long_reference(which)
    assert case.signal.shape == (4, C.MAP_T) and C.MAP_T == 4096 and case.signal_lengths.tolist() == [4096, 4095, 1, 1]
    codes, faults = MR.prepare(case.ref, case.model, C.PATH_K)
    assert len(codes) == C.MAP_M == 5200 and faults == 0 and (codes < 0).sum() == 2 * C.PATH_K
    assert ref["bad"] == 0 and (ref["end"] >= 0).all() and MR.BAD_READ not in ref["score"].tolist()
    score = [int(v) for v in ref["score"]]
    if which == "costly":                                            # the largest a cell can cost is 2^31 - 1 + 2^30 - 1
        assert 0.9 * 4096 * (2 ** 31 + 2 ** 30) < score[0] < 4096 * (2 ** 31 + 2 ** 30) and score[0] > 2 ** 43.5
        assert C.COST_MAX < score[3] <= C.COST_MAX + C.OFFSET_MAX
    else:
        assert -4096 * 2 ** 30 < score[0] < -4096 * 2 ** 30 + 2 ** 20 and -2 ** 30 < score[2] < -2 ** 30 + 100
    assert ref["end"][0] - ref["start"][0] > 1500 and ref["end"][1] - ref["start"][1] > 1500       # a walk, not a stay
    assert ref["end"][0] - ref["start"][0] < 4096 - 1024             # and it stays as well: both moves in every tile
    tiles_after_the_halo = -(-C.MAP_M // 1024) - (4096 + 64) // 1024
    assert tiles_after_the_halo > 1
    finite = [int(v) for v in ref["end_cost"][0] if v != MR.NO_MAPPING]
    assert len(finite) == C.MAP_M - 2 * C.PATH_K and len(set(finite)) > 1000


@pytest.mark.parametrize("band", sorted(C.DIAGONAL))
@pytest.mark.parametrize("which", ["costly", "cheap"])
def test_the_diagonal_is_forced_and_its_cost_is_the_plain_sum(which, band):
    case, ref = C.diagonal_case(which, band), C.diagonal_reference(which, band)
    assert ref["bad"] == 0
    for b, (T, N) in enumerate(C.DIAGONAL[band]):
        assert N > band and T - N in (0, 1) and int(case.signal_lengths[b]) == T
        lo = [AR.band_lo(t, N, T, band) for t in range(T)]
        assert lo[-1] == N - band and sum(np.diff(lo) == 1) == N - band
        if T == N:
            assert lo == [min(max(t - band // 2, 0), N - band) for t in range(T)]       # it rises on every step until it is at the top
            assert ref["states"][b, :T].tolist() == list(range(N)) and ref["starts"][b, :N + 1].tolist() == list(range(N + 1))
            assert ref["score"][b] == C.diagonal_sum(case, b)
        else:
            assert sorted(set(ref["states"][b, :T].tolist())) == list(range(N))
        per_sample = ref["score"][b] / T
        assert per_sample > 0.9 * (2 ** 31 + 2 ** 30) if which == "costly" else per_sample < -2 ** 30 + 100
