"""GPU: the CTC loss kernels (csrc/wn_ctc.hip, through training.ctc_total and its backward) against the float64 reference
tests/ctc_loss_ref.py at the edges of their design: the range of the mantissa + exponent number format, all eight states per
thread and the 512-state slot boundaries up to the documented 2047 labels, the 32-frame staging chunk and the 16-frame gradient
block, frame counts of 0 and 1, closed forms, 2 / 63 / 64 classes, blanks other than 0, label padding as real callers write it,
independence of the utterances of a batch, input forms, lengths out of range and -inf logits.

The inputs come from ctc_loss_ref.edge_cases(); tests/test_ctc_loss_ref.py shows on the CPU that each of them separates the
reference from a named wrong variant by 100 times the bounds used here.  Bounds (tests/test_ctc.py's own): loss
2e-6 * max(1, |ref|) -- it leaves the kernel as fp32, 2^-24 relative --, gradient 2e-6 absolute -- alpha and beta pass through
HBM with fp32 mantissas, so an occupancy term carries 2 * 2^-24 on entries in [-1, 1], 2.4e-7 with the output rounding.
Per-utterance losses come from B = 1 calls.  Observed maxima: DESIGN.md section 7, "Edges and limits of the CTC loss"."""
import numpy as np
import pytest
import torch

from tests import ctc_loss_ref as R
from wavenet_speech_amd import check_device_flags
from wavenet_speech_amd import training as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(c, grad=True, labels=None, lens=None, input_lengths=None, acts=None):
    """one call on the device -> (loss, a 0-d fp32 tensor on the host; gradient as a tensor on the host, or None)"""
    x = torch.tensor(c["acts"] if acts is None else acts, dtype=torch.float32, device=DEV, requires_grad=grad)
    labels = torch.tensor(c["labels"], device=DEV) if labels is None else labels
    lens = torch.tensor(c["lens"], device=DEV) if lens is None else lens
    if input_lengths is None and c["input_lengths"] is not None:
        input_lengths = torch.tensor(c["input_lengths"], device=DEV)
    loss = T.ctc_total(x, labels, lens, blank=c["blank"], input_lengths=input_lengths)
    if grad:
        loss.backward()
    return loss.detach().cpu(), (x.grad.cpu() if grad else None)


def alone(c, b, grad=True):
    """utterance b of the case as a batch of one (same Lmax)"""
    one = dict(c, acts=c["acts"][b:b + 1], labels=c["labels"][b:b + 1], lens=c["lens"][b:b + 1],
               input_lengths=None if c["input_lengths"] is None else c["input_lengths"][b:b + 1])
    return run(one, grad=grad)


def check(family, c, ref=None):
    """loss (batch and per utterance) and gradient of one case against the reference; returns the device's (loss, gradient)"""
    nll, gref = R.reference(c) if ref is None else ref
    B, C, Tn = c["acts"].shape
    loss, g = run(c)
    g = g.numpy().astype(np.float64)
    keep = list(range(B))
    loss_err = 0.0
    per = [loss] if B == 1 else [alone(c, b, grad=False)[0] for b in range(B)]
    for b in keep:
        if np.isinf(nll[b]):
            assert torch.isinf(per[b]) and per[b] > 0, (c["name"], b, float(per[b]))
            assert not g[b].any()                                              # an infeasible utterance: no gradient at all
        else:
            e = abs(float(per[b]) - nll[b]) / max(1.0, abs(nll[b]))
            loss_err = max(loss_err, e)
    total = float(np.sum(nll))
    if np.isinf(total):
        assert torch.isinf(loss) and loss > 0
    else:
        loss_err = max(loss_err, abs(float(loss) - total) / max(1.0, abs(total)))
    assert np.isfinite(g[keep]).all(), c["name"]
    grad_err = float(np.abs(g[keep] - gref[keep]).max())
    print("OBSERVED %-15s %-14s loss err %.2e (bound %.0e), gradient err %.2e (bound %.0e)"
          % (family, c["name"], loss_err, R.LOSS_TOL, grad_err, R.GRAD_TOL))
    assert loss_err < R.LOSS_TOL, (c["name"], loss_err)
    assert grad_err < R.GRAD_TOL, (c["name"], grad_err)
    if c["input_lengths"] is not None:
        for b in keep:
            assert not g[b][:, int(c["input_lengths"][b]):].any()             # frames past the utterance: exactly 0
    return loss, g


# ---- a. range of the number format ------------------------------------------------------------------------------------------------
def test_a_peaked_logits_beyond_a_float64_probability():
    peaked = R.edge_cases("a_range")[0]
    assert peaked["acts"].shape == (2, 5, 64) and list(peaked["lens"]) == [8, 5]
    nll, _ = R.reference(peaked)
    print("peaked: nll", nll)
    assert np.isfinite(nll).all() and nll.min() > 745.0                       # p < exp(-745): 0 as a plain float64
    check("a_range", peaked)


def test_a_row_wider_than_float64_reaches():
    wide = R.edge_cases("a_range")[1]
    gap = R.row_gap(wide["acts"][0], wide["labels"][0][:wide["lens"][0]])
    print("wide row: nll %.1f, a state with occupancy > 0.5 lies %.1f nats below its row's largest alpha"
          % (R.reference(wide)[0][0], gap))
    assert gap > 745.0, gap                                                   # before the device is looked at
    check("a_range", wide)


# ---- b. states per thread, slot boundaries ---------------------------------------------------------------------------------------
def test_b_2047_labels_all_eight_slots():
    c = R.long_case()
    assert c["acts"].shape == (1, 64, 2304) and c["labels"].shape == (1, 2047)
    check("b_slots", c)


@pytest.mark.parametrize("index", range(1, 6), ids=["L255", "L256", "L511", "L512", "L300_and_L3"])
def test_b_slot_boundaries(index):
    c = R.edge_cases("b_slots")[index]
    if index < 5:
        assert 2 * c["labels"].shape[1] + 1 in (511, 513, 1023, 1025)
    check("b_slots", c)


# ---- c. frame boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("Tn", R.FRAME_COUNTS)
def test_c_frame_boundaries(Tn, ragged):
    c = R.frame_case(Tn, ragged)
    assert c["acts"].shape[2] == Tn
    if ragged:
        assert set(c["input_lengths"]) == {v for v in (Tn, 33, 32, 17, 16, 1) if v <= Tn}
        assert np.isfinite(R.reference(c)[0]).all()
    check("c_frames", c)


def test_c_no_frames():
    c = R.edge_cases("c_frames")[-1]
    assert list(c["input_lengths"]) == [0, 0, 9] and list(c["lens"]) == [0, 2, 2]
    loss, g = check("c_frames", c)
    assert torch.isinf(loss) and not g[0].any() and not g[1].any() and g[2].any()
    l0, g0 = alone(c, 0)
    l1, g1 = alone(c, 1)
    assert float(l0) == 0.0 and not g0.any()                                 # no frames, no labels: probability 1
    assert torch.isinf(l1) and l1 > 0 and not g1.any()                       # no frames, labels: impossible


# ---- d. closed forms --------------------------------------------------------------------------------------------------------------
def test_d_closed_forms_on_the_device():
    for c in R.edge_cases("d_closed"):
        assert list(c["input_lengths"]) == [9, 9, 8] and R.min_frames(R.D_LABELS) == 9
        loss, g = check("d_closed", c)
        assert torch.isinf(loss) and not g[2].any()                          # one frame short of the only alignment
        for b, path in ((0, [0] * 9), (1, R.D_PATH)):
            want, gwant = R.closed_form_path(c["acts"][b], path)
            got = float(alone(c, b, grad=False)[0])
            assert abs(got - want) < R.LOSS_TOL * max(1.0, abs(want)), (b, got, want)
            assert np.abs(g[b] - gwant).max() < R.GRAD_TOL
        # the infeasible neighbour changes nothing for the others: the same batch with utterance 2 feasible
        _, g9 = run(c, input_lengths=torch.tensor([9, 9, 9], device=DEV))
        assert np.array_equal(g9.numpy()[:2], g[:2].astype(np.float32)) and g9[2].any()


# ---- e. classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(3), ids=["C2", "C63", "C64"])
def test_e_class_counts(index):
    c = R.edge_cases("e_classes")[index]
    assert c["acts"].shape[1] == (2, 63, 64)[index]
    check("e_classes", c)


# ---- f. blank ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(3), ids=["blank0", "blank2", "blank4"])
def test_f_blank(index):
    c = R.edge_cases("f_blank")[index]
    assert c["blank"] == (0, 2, 4)[index]
    used = np.concatenate([c["labels"][b][:c["lens"][b]] for b in range(2)])
    assert c["blank"] not in used and (c["blank"] == 0 or 0 in used)
    check("f_blank", c)
    bad = torch.tensor(c["labels"], device=DEV)
    bad[1, 2] = c["blank"]
    with pytest.raises(RuntimeError, match="ctc labels"):
        run(c, grad=False, labels=bad)


# ---- g. padding -------------------------------------------------------------------------------------------------------------------
def test_g_padding_is_never_read():
    cases = R.edge_cases("g_padding")
    first = cases[0]
    assert [int(c["labels"][1, 0]) for c in cases[:3]] == [0, -1, 105] and first["labels"].shape == (3, 8)
    check_device_flags()
    loss0, g0 = check("g_padding", first)
    for c in cases[1:]:
        assert np.array_equal(c["acts"], first["acts"]) and not np.array_equal(c["labels"], first["labels"])
        loss, g = run(c)
        assert torch.equal(loss, loss0) and np.array_equal(g.numpy(), g0.astype(np.float32)), c["name"]
        loss_only, _ = run(c, grad=False)                                    # raises at once if a flag is set
        assert torch.equal(loss_only, loss0)
    check_device_flags()                                                     # no flag raised by any of them


# ---- h. independence --------------------------------------------------------------------------------------------------------------
def test_h_utterances_are_independent():
    c = R.edge_cases("h_independence")[0]
    B = c["acts"].shape[0]
    loss, g = check("h_independence", c)
    g = g.astype(np.float32)
    flipped = dict(c, acts=c["acts"][::-1].copy(), labels=c["labels"][::-1].copy(), lens=c["lens"][::-1].copy())
    _, gf = run(flipped)
    wide_labels, _ = R.pad_rows([c["labels"][b][:c["lens"][b]] for b in range(B)], fill=0, width=40)
    assert (2 * 40 + 1 + 63) // 64 != (2 * c["labels"].shape[1] + 1 + 63) // 64          # another row stride in the workspace
    lw, gw = run(dict(c, labels=wide_labels))
    per = []
    for b in range(B):
        lb, gb = alone(c, b)
        per.append(lb)
        assert np.array_equal(gb.numpy()[0], g[b]), b                         # alone
        assert np.array_equal(gf.numpy()[B - 1 - b], g[b]), b                 # at another batch index
        assert np.array_equal(gw.numpy()[b], g[b]), b                         # with a wider Lmax
    assert torch.equal(lw, loss)
    assert torch.equal(torch.stack(per).to(DEV).sum().cpu(), loss)            # the batch loss is the fp32 sum of the B = 1 losses


# ---- i. input forms ---------------------------------------------------------------------------------------------------------------
def test_i_input_forms_give_the_same_bits():
    c = R.edge_cases("i_forms")[0]
    loss, g = check("i_forms", c)
    g = g.astype(np.float32)
    # logits as a non-contiguous view of a [B, T, C] tensor
    xt = torch.tensor(c["acts"], dtype=torch.float32, device=DEV).permute(0, 2, 1).contiguous().requires_grad_(True)
    view = xt.permute(0, 2, 1)
    assert not view.is_contiguous()
    lv = T.ctc_total(view, torch.tensor(c["labels"], device=DEV), torch.tensor(c["lens"], device=DEV))
    lv.backward()
    assert torch.equal(lv.detach().cpu(), loss)
    assert np.array_equal(xt.grad.permute(0, 2, 1).cpu().numpy(), g)
    # labels and lengths as int32, and on the host
    for dtype, dev in ((torch.int32, DEV), (torch.int64, "cpu"), (torch.int32, "cpu")):
        l2, g2 = run(c, labels=torch.tensor(c["labels"], dtype=dtype, device=dev), lens=torch.tensor(c["lens"], dtype=dtype, device=dev),
                     input_lengths=torch.full((2,), c["acts"].shape[2], dtype=dtype, device=dev))
        assert torch.equal(l2, loss) and np.array_equal(g2.numpy(), g), (dtype, dev)
    # the loss-only launch (no gradient requested: dlogits = NULL, no beta pass)
    l3, _ = run(c, grad=False)
    assert torch.equal(l3, loss)


# ---- j. lengths out of range ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,value", [("input_lengths", "T+1"), ("input_lengths", -1), ("lens", "Lmax+1"), ("lens", -1)])
def test_j_lengths_out_of_range_are_refused(which, value):
    """csrc/wn_ctc.hip: ctc_pass_kernel and ctc_grad_kernel clamp such an utterance to Tb = Lb = 0 before any address is formed
    from its lengths; the pass kernel poisons its loss and raises the flag, the gradient kernel writes zeros"""
    c = R.bad_length_case()
    B, C, Tn = c["acts"].shape
    nll, gref = R.reference(c)
    bad = dict(c, lens=c["lens"].copy(), input_lengths=c["input_lengths"].copy())
    bad[which][1] = {"T+1": Tn + 1, "Lmax+1": c["labels"].shape[1] + 1}.get(value, value)
    check_device_flags()
    with pytest.raises(RuntimeError, match="ctc labels"):
        run(bad, grad=False)                                                 # without a gradient: at once
    try:
        loss, g = run(bad)                                                   # with one: NaN now, the exception deferred
        assert torch.isnan(loss)
        g = g.numpy()
        assert not g[1].any()
        assert np.abs(g[[0, 2]] - gref[[0, 2]]).max() < R.GRAD_TOL
        with pytest.raises(RuntimeError, match="ctc labels"):
            check_device_flags()
    finally:
        try:
            check_device_flags()                                             # nothing of this test reaches a later one
        except RuntimeError:
            pass
    check("j_bad_lengths", c, ref=(nll, gref))                               # a clean call afterwards
    check_device_flags()


# ---- k. -inf logits ---------------------------------------------------------------------------------------------------------------
def test_k_minus_infinity_logits():
    c = R.edge_cases("k_neg_inf")[0]
    assert np.isneginf(c["acts"][0, 2, 3:9]).all() and np.isfinite(R.reference(c)[0][0])
    loss, g = check("k_neg_inf", c)
    assert np.isfinite(g).all() and not g[0, 2, 3:9].any()
