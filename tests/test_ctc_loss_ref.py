"""CPU: tests/ctc_loss_ref.py, the vectorised float64 reference that tests/test_gpu_ctc_edges.py holds the CTC loss kernels to.
Pinned three ways -- the loop oracle (oracle/ctc_oracle.py) at small shapes and three blanks, torch's float64 CPU ctc_loss at
2304 frames x 2047 labels, closed forms that go through no recursion -- and shown to tell itself from each of its MUTANTS, on
every input the GPU test uses, by at least 100 times the GPU tolerance: the GPU test can fail."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ctc_oracle as CO
from tests import ctc_loss_ref as R

SMALL = [(1, 3, 5, 12, 4, False), (2, 2, 7, 30, 9, False), (3, 2, 5, 9, 4, True), (4, 1, 4, 3, 3, False), (6, 2, 3, 20, 10, True),
         (10, 1, 2, 1, 1, False), (12, 2, 3, 2, 1, True), (13, 1, 5, 1, 3, False)]       # the small shapes of tests/test_ctc.py


def _small_case(seed, B, C, Tn, lmax, repeats, blank):
    rng = np.random.default_rng(seed)
    acts = rng.normal(size=(B, C, Tn)) * 1.5
    lens = rng.integers(0 if seed % 3 == 0 else 1, lmax + 1, size=B)
    pool = np.array([c for c in range(C) if c != blank])
    labels = pool[rng.integers(0, 1 if repeats else len(pool), size=(B, lmax))]
    return acts, labels, lens


@pytest.mark.parametrize("blank", [0, 1, -1])
@pytest.mark.parametrize("seed,B,C,Tn,lmax,repeats", SMALL)
def test_reference_agrees_with_the_loop_oracle(seed, B, C, Tn, lmax, repeats, blank):
    blank = blank % C                                                     # 0, 1 and C - 1
    acts, labels, lens = _small_case(seed, B, C, Tn, lmax, repeats, blank)
    in_len = None if seed % 2 else np.maximum(1, Tn - np.arange(B) * 2)
    nll, grad = R.ctc_ref(acts, labels, lens, blank=blank, input_lengths=in_len)
    for b in range(B):
        tb = Tn if in_len is None else int(in_len[b])
        n, g = CO.ctc_nll_and_grad(acts[b][:, :tb], [int(v) for v in labels[b][:lens[b]]], blank)
        if np.isinf(n):
            assert np.isinf(nll[b]) and nll[b] > 0 and not grad[b].any()
            continue
        assert abs(nll[b] - n) < 1e-9 * max(1.0, abs(n)), (b, nll[b], n)
        assert np.abs(grad[b][:, :tb] - g).max() < 1e-9
        assert not grad[b][:, tb:].any()


@functools.lru_cache(maxsize=None)
def _long():
    c = R.long_case()
    return c, R.reference(c)


def test_reference_agrees_with_torch_float64_at_2047_labels():
    c, (nll, grad) = _long()
    lab = c["labels"][0]
    assert c["acts"].shape == (1, 64, 2304) and len(lab) == 2047 and int((lab[1:] == lab[:-1]).sum()) >= 1
    x = torch.tensor(c["acts"], dtype=torch.float64, requires_grad=True)
    ref = F.ctc_loss(F.log_softmax(x.permute(2, 0, 1), dim=2), torch.tensor(c["labels"]), torch.tensor([2304]), torch.tensor([2047]),
                     blank=0, reduction="sum")
    ref.backward()
    ref = ref.detach()
    assert 5e3 < float(ref) < 5e4
    assert abs(nll[0] - float(ref)) < 1e-9 * abs(float(ref)), (nll[0], float(ref))
    g = x.grad.numpy()
    assert np.abs(grad - g).max() < 1e-9 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("blank", [0, 3])
def test_closed_form_no_labels(blank):
    acts = np.random.default_rng(5).normal(size=(2, 5, 11)) * 2.0
    nll, grad = R.ctc_ref(acts, np.full((2, 3), 1), [0, 0], blank=blank, input_lengths=[11, 7])
    for b, tb in enumerate((11, 7)):
        want, gwant = R.closed_form_path(acts[b][:, :tb], [blank] * tb)
        assert abs(nll[b] - want) < 1e-12 * abs(want)
        assert np.abs(grad[b][:, :tb] - gwant).max() < 1e-12 and not grad[b][:, tb:].any()


def test_closed_form_single_alignment():
    assert R.single_path(R.D_LABELS) == R.D_PATH and R.min_frames(R.D_LABELS) == 9
    acts = np.random.default_rng(6).normal(size=(1, 5, 9)) * 2.0
    nll, grad = R.ctc_ref(acts, [R.D_LABELS], [6])
    want, gwant = R.closed_form_path(acts[0], R.D_PATH)
    assert abs(nll[0] - want) < 1e-12 * abs(want)
    assert np.abs(grad[0] - gwant).max() < 1e-12
    x = torch.tensor(acts, requires_grad=True)                                # torch's float64 ctc_loss agrees with the closed form too
    ref = F.ctc_loss(F.log_softmax(x.permute(2, 0, 1), dim=2), torch.tensor([R.D_LABELS]), torch.tensor([9]), torch.tensor([6]),
                     reduction="sum")
    ref.backward()
    ref = ref.detach()
    assert abs(float(ref) - want) < 1e-12 * abs(want) and np.abs(x.grad.numpy()[0] - gwant).max() < 1e-12
    # with another blank and one frame short
    path = R.single_path([0, 0, 1], blank=2)
    assert path == [0, 2, 0, 1]
    n4, g4 = R.ctc_ref(acts[:, :, :4], [[0, 0, 1]], [3], blank=2)
    want4, gwant4 = R.closed_form_path(acts[0][:, :4], path)
    assert abs(n4[0] - want4) < 1e-12 * abs(want4) and np.abs(g4[0] - gwant4).max() < 1e-12
    n3, g3 = R.ctc_ref(acts[:, :, :3], [[0, 0, 1]], [3], blank=2)
    assert np.isinf(n3[0]) and not g3.any()


def test_reference_edges():
    rng = np.random.default_rng(8)
    acts = rng.normal(size=(2, 5, 10))
    # nothing past the length of a label row is read: any padding gives the same bits
    a = R.ctc_ref(acts, [[1, 2, 0, -1], [3, 99, -7, 1 << 40]], [2, 1])
    b = R.ctc_ref(acts, [[1, 2, 4, 4], [3, 1, 1, 1]], [2, 1])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # no frames: only the empty labelling is possible
    n, g = R.ctc_ref(acts, [[1], [1]], [0, 1], input_lengths=[0, 0])
    assert n[0] == 0.0 and np.isinf(n[1]) and not g.any()
    # -inf logits: finite loss and gradient, equal to the loop oracle's; a labelling through the dead frames is infeasible
    acts = rng.normal(size=(1, 5, 20)) * 1.5
    acts[0, 2, 3:9] = -np.inf
    n, g = R.ctc_ref(acts, [[1, 2, 3]], [3])
    no, go = CO.ctc_nll_and_grad(acts[0], [1, 2, 3])
    assert np.isfinite(n[0]) and np.isfinite(g).all() and abs(n[0] - no) < 1e-9 and np.abs(g[0] - go).max() < 1e-9
    assert not g[0, 2, 3:9].any()
    acts[0, 2, :] = -np.inf
    n, g = R.ctc_ref(acts, [[1, 2, 3]], [3])
    assert np.isinf(n[0]) and not g.any()


def separation(c, mutant=None):
    """how far the mutant's answer lies from the reference's on this input, in units of the GPU test's tolerances (inf where
    the mutant is not finite and the reference is, or one of the two is +inf and the other is not)"""
    nll, grad = _long()[1] if c["name"] == "L2047" else R.reference(c)
    mn, mg = R.reference(c, mutant=mutant or c["mutant"])
    worst = 0.0
    for b in range(len(nll)):
        if np.isinf(nll[b]) != np.isinf(mn[b]) or np.isnan(mn[b]) or not np.isfinite(mg[b]).all():
            return np.inf
        if np.isfinite(nll[b]):
            worst = max(worst, abs(mn[b] - nll[b]) / (R.LOSS_TOL * max(1.0, abs(nll[b]))))
        worst = max(worst, np.abs(mg[b] - grad[b]).max() / R.GRAD_TOL)
    return worst


@pytest.mark.parametrize("family", R.FAMILIES)
def test_every_gpu_input_separates_the_reference_from_its_mutant(family):
    cases = R.edge_cases(family)
    assert cases
    for c in cases:
        assert c["mutant"] in R.MUTANTS
        s = separation(c)
        print("%-16s %-14s %-38s separation %.3g x tolerance" % (family, c["name"], c["mutant"], s))
        assert s >= 100.0, (family, c["name"], c["mutant"], s)


def test_every_mutant_has_an_input_that_catches_it():
    assert {c["mutant"] for f in R.FAMILIES for c in R.edge_cases(f)} == set(R.MUTANTS)


def test_the_range_inputs_are_out_of_a_float64_rows_reach():
    peaked, wide = R.edge_cases("a_range")
    # the plain linear float64 recursion without any scaling: every path probability of the peaked input underflows to exactly 0
    nll, _ = R.reference(peaked)
    assert np.isfinite(nll).all() and nll.min() > 745.0, nll
    for b in range(2):
        y = np.exp(R.log_softmax(peaked["acts"][b]))
        ext = R._extended(peaked["labels"][b][:peaked["lens"][b]], 0)
        row = np.zeros(len(ext))
        row[:2] = 1.0
        row = row * y[ext, 0]
        for t in range(1, y.shape[1]):
            row = (row + R._shift(row, 1, 0.0) + np.where(R._skip(ext, 0), R._shift(row, 2, 0.0), 0.0)) * y[ext, t]
        assert row[-1] + row[-2] == 0.0
    # the constructed row: a state holding most of the probability lies further below its row's maximum than exp() reaches
    gap = R.row_gap(wide["acts"][0], wide["labels"][0][:wide["lens"][0]])
    print("wide row: nll %.1f, occupied state %.1f nats below the row maximum" % (R.reference(wide)[0][0], gap))
    assert gap > 745.0, gap
