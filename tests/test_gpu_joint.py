"""The joint NLL + CTC step (wavenet_speech_amd/training.py::joint_losses, the reference's legacy_code/train.py) against an fp64
reference: both losses, the gradient that arrives at the WaveNet's logits `pred`, and every parameter gradient of both networks.

`pred` is the one tensor of the step that receives two cotangents -- the NLL head's dlogits and the classifier's input gradient,
spread over the pooling windows by pool_unload_kernel -- and the CTC gradient, scaled by 1 / T', is what sets the f16 dynamic
gradient scale of the classifier's stack.  The reference restates training.py:90-100:

    pred  = wavenet(sig[:, :, :-1])                 oracle model in fp64 (f32, f16x3) / tests/halfref.py::wavenet (plain modes)
    trans = classifier(pred)                        tests/halfref.py::wavenet_classifier
    xe    = cross_entropy(pred, argmax(sig[:, :, 1:]), "sum") / B / sig.shape[2]        (the FULL signal length, one more than pred's)
    ctc   = ctc_loss(log_softmax(trans), seq + 1, "sum") / T',  T' = trans.shape[2]

f32 and f16x3: every tensor within 1e-4 (max-norm, relative) of the exact reference.  Plain modes: every tensor passes the halfref
predicate e_hip <= KAPPA e_fmt + FLOOR; the two losses are scalars, for which the rounding reference IS the prediction of what the
device computes, and are held to 1e-4 max(1, |loss|) of it as the fp32 step test holds them to the oracle's (their distances from the
exact losses are printed beside).  Every utterance admits a CTC alignment (T' >= 2 len + 1), which the CPU test below and every GPU
case assert on the reference first: nothing here can pass by comparing inf with inf."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as O
from tests import halfref as R
from tests.gpu_stack import PLAIN, TOL, condition as _condition, launched as _launched, plain_slopes as _plain_slopes
from tests.gpu_util import DEV

PRECISIONS = ("f32", "f16x3", "bf16", "f16")
MUTANTS = ("nll x B", "ctc not / T'", "classifier dx dropped", "labels not shifted")

CASES = {  # levels, WaveNet layers, classifier layers, classifier out_dim, num_labels, pool, L, label lengths (B of them)
    # 256 levels, 64 channels, pred length 599 = 3 x 199 + 2: the NLL gradient covers two frames the classifier's leaves at zero
    "levels256_64ch_pool3": (256, [(64, 64, 2, d) for d in (1, 2, 4, 8)], [(64, 64, 2, 1), (64, 64, 3, 2)], 64, 5, 3, 600, (40, 25)),
    "one_utterance": (32, [(32, 32, 2, d) for d in (1, 2, 4)], [(32, 32, 2, 1), (32, 32, 2, 2)], 32, 5, 3, 121, (12,)),
    # pred length 127 = 5 x 25 + 2
    "pool5_ragged_tail": (16, [(16, 16, 2, d) for d in (1, 2)], [(24, 24, 2, 1), (24, 24, 2, 3)], 24, 6, 5, 128, (9, 1, 12)),
}


def make_case(name):
    """(wavenet, classifier, sig one-hot [B, levels, L], seq [B, S] labels in 1 .. num_labels - 2, lengths) on the CPU.  Labels avoid 0
    so that the un-shifted labels of the mutant reference are still legal (never the blank)."""
    from wavenet_speech_amd.modules import WaveNet, WaveNetClassifier
    levels, wl, cl, cout, nlab, pool, L, lens = CASES[name]
    torch.manual_seed(len(name) + L)
    wavenet = _condition(WaveNet(levels, 2, wl, levels, softmax=False))
    ctcnet = _condition(WaveNetClassifier(levels, nlab, cl, cout, pool_kernel_size=pool, softmax=False))
    B = len(lens)
    g = torch.Generator().manual_seed(L)
    sig = O.one_hot_encoding(torch.randint(0, levels, (B, L), generator=g), levels)
    seq = torch.randint(1, nlab - 1, (B, max(lens)), generator=g)
    return wavenet, ctcnet, sig, seq, torch.tensor(lens), wl, cl, pool


def reference(sdw, sdc, sig, seq, lengths, wl, cl, pool, fmt, slopes_w=None, slopes_c=None, fused_w=True, fused_c=True, mutant=None):
    """{"avg_xe", "avg_ctc", "dpred", "wavenet.<name>", "ctcnet.<name>"} of the joint step in fp64 (fmt None: exact)"""
    DT = R.DT
    sdw = {k: v.detach().to(DT).requires_grad_(True) for k, v in sdw.items()}
    sdc = {k: v.detach().to(DT).requires_grad_(True) for k, v in sdc.items()}
    sig = sig.to(DT)
    B = sig.shape[0]
    pred = R.wavenet(sig[:, :, :-1], sdw, wl, fmt, slopes=slopes_w, fused_head=fused_w)
    pred.retain_grad()
    trans = R.wavenet_classifier(pred.detach() if mutant == "classifier dx dropped" else pred, sdc, cl, pool, fmt, slopes=slopes_c,
                                 fused=fused_c)
    xe = F.cross_entropy(pred, sig[:, :, 1:].argmax(dim=1), reduction="sum") / B
    if mutant == "nll x B":
        xe = xe * B
    T = trans.shape[2]
    labels = seq.long() + (0 if mutant == "labels not shifted" else 1)
    ctc = F.ctc_loss(F.log_softmax(trans.permute(2, 0, 1), dim=2), labels, torch.full((B,), T, dtype=torch.long), lengths.long(),
                     blank=0, reduction="sum", zero_infinity=False)
    avg_xe = xe / sig.shape[2]
    avg_ctc = ctc if mutant == "ctc not / T'" else ctc / T
    (avg_xe + avg_ctc).backward()
    out = {"avg_xe": avg_xe.detach(), "avg_ctc": avg_ctc.detach(), "dpred": pred.grad}
    out.update({"wavenet." + k: v.grad for k, v in sdw.items() if v.grad is not None})
    out.update({"ctcnet." + k: v.grad for k, v in sdc.items() if v.grad is not None})
    return out, T


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_cases_have_finite_ctc(case):
    """CPU: every utterance admits an alignment (T' >= 2 len + 1 is sufficient) and the reference losses are finite"""
    wavenet, ctcnet, sig, seq, lengths, wl, cl, pool = make_case(case)
    ref, T = reference(wavenet.state_dict(), ctcnet.state_dict(), sig, seq, lengths, wl, cl, pool, None)
    assert T == (sig.shape[2] - 1) // pool and all(T >= 2 * int(n) + 1 for n in lengths)
    assert math.isfinite(float(ref["avg_xe"])) and math.isfinite(float(ref["avg_ctc"])) and float(ref["avg_ctc"]) > 0
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    if (sig.shape[2] - 1) % pool:
        assert seq.min() >= 1          # (and the frames past the last window get the NLL gradient alone)
    assert case != "levels256_64ch_pool3" or len(set(int(n) for n in lengths)) > 1        # ragged label lengths


def gpu_step(wavenet, ctcnet, sig, seq, lengths, precision):
    """the two halves of joint_losses by hand, so that pred's gradient can be kept: (tensors, slopes of both networks, launched)"""
    import wavenet_speech_amd as W
    from wavenet_speech_amd import functional as HF
    from wavenet_speech_amd import training as T
    wavenet, ctcnet = wavenet.to(DEV), ctcnet.to(DEV)
    W.set_precision(wavenet, precision)
    W.set_precision(ctcnet, precision)
    sg, sq, ln = sig.to(DEV), seq.to(DEV), lengths.to(DEV)
    x = sg[:, :, :-1].contiguous()
    if precision in PLAIN:
        sw = _plain_slopes(wavenet, x)
        p0 = wavenet(x).detach()                # (training path, as the measured step; the fused output block gives the same bits)
        sc = _plain_slopes(ctcnet, p0.requires_grad_(True))
        removes = []
    else:
        (sw, r1), (sc, r2) = O.capture_leaky_slopes(wavenet), O.capture_leaky_slopes(ctcnet)
        removes = [r1, r2]
    for n in (wavenet, ctcnet):
        n.zero_grad(set_to_none=True)
    HF.profile_reset()
    HF.profile_enable(True)
    try:
        pred = wavenet(x)
        pred.retain_grad()
        transcription = ctcnet(pred)
        for r in removes:
            r()
        xe = T.sequence_nll(pred, sg[:, :, 1:].argmax(dim=1))
        ctc = T.ctc_total(transcription, sq.long() + 1, ln.long())
        avg_xe, avg_ctc = xe / sg.shape[2], ctc / transcription.shape[2]
        (avg_xe + avg_ctc).backward()
        torch.cuda.synchronize()
    finally:
        HF.profile_enable(False)
    W.check_device_flags()
    hip = {"avg_xe": avg_xe.detach().cpu(), "avg_ctc": avg_ctc.detach().cpu(), "dpred": pred.grad.cpu()}
    hip.update({"wavenet." + k: p.grad.cpu() for k, p in wavenet.named_parameters() if p.grad is not None})
    hip.update({"ctcnet." + k: p.grad.cpu() for k, p in ctcnet.named_parameters() if p.grad is not None})
    # the step as the library runs it gives the same bits
    for n in (wavenet, ctcnet):
        n.zero_grad(set_to_none=True)
    a, b, j = T.joint_losses(wavenet, ctcnet, sg, sq, ln)
    j.backward()
    assert float(a) == float(hip["avg_xe"]) and float(b) == float(hip["avg_ctc"])
    for name, net in (("wavenet.", wavenet), ("ctcnet.", ctcnet)):
        for k, p in net.named_parameters():
            assert (p.grad is None) == (name + k not in hip) and (p.grad is None or torch.equal(p.grad.cpu(), hip[name + k])), k
    W.check_device_flags()
    return hip, sw, sc, _launched()


def verdicts(hip, exact, rounded, precision, label, quiet=False):
    """{name: passes} for the losses and every tensor"""
    losses = ("avg_xe", "avg_ctc")
    ref = exact if rounded is None else rounded
    ok = {}
    for k in losses:
        d, de = abs(float(hip[k]) - float(ref[k])), abs(float(hip[k]) - float(exact[k]))
        ok[k] = d < 1e-4 * max(1.0, abs(float(ref[k])))
        if not quiet:
            print("%s %-8s %.8g  reference %.8g (distance %.2e; from the exact loss %.8g: %.2e)%s"
                  % (label, k, float(hip[k]), float(ref[k]), d, float(exact[k]), de, "" if ok[k] else "  FAIL"))
    names = [k for k in exact if k not in losses]
    if rounded is None:
        errs = {k: O.rel_err(hip[k].double(), exact[k]) for k in names}
        worst = max(errs, key=errs.get)
        if not quiet:
            print("%s dpred %.2e, worst %s %.2e" % (label, errs["dpred"], worst, errs[worst]))
        ok.update({k: errs[k] < TOL for k in names})
    else:
        res = R.compare(label, {k: hip[k] for k in names}, rounded, {k: exact[k] for k in names}, quiet=quiet)
        ok.update({k: v[2] for k, v in res.items()})
    return ok


def check_joint(case, precision, mutants=()):
    from wavenet_speech_amd.modules.block import fusable_head
    wavenet, ctcnet, sig, seq, lengths, wl, cl, pool = make_case(case)
    sdw, sdc = ({k: v.clone() for k, v in n.state_dict().items()} for n in (wavenet, ctcnet))
    hip, sw, sc, launched = gpu_step(wavenet, ctcnet, sig, seq, lengths, precision)
    assert launched.get("ctc_kernel", 0) > 0 and launched.get("hload_kernel", 0) >= 2, launched      # CTC; pooled load and unload
    kw = dict(slopes_w=sw, slopes_c=sc, fused_w=fusable_head(wavenet.output_stack, precision) is not None,
              fused_c=fusable_head(ctcnet.output_block, precision) is not None)
    plain = precision in PLAIN

    def refs(mutant):
        exact, T = reference(sdw, sdc, sig, seq, lengths, wl, cl, pool, None, mutant=mutant, **kw)
        assert all(T >= 2 * int(n) + 1 for n in lengths)
        assert math.isfinite(float(exact["avg_ctc"])) and math.isfinite(float(exact["avg_xe"])), "the reference loss must be finite"
        rounded = reference(sdw, sdc, sig, seq, lengths, wl, cl, pool, precision, mutant=mutant, **kw)[0] if plain else None
        assert rounded is None or (math.isfinite(float(rounded["avg_ctc"])) and set(rounded) == set(exact))
        return exact, rounded
    exact, rounded = refs(None)
    assert set(exact) == set(hip), sorted(set(exact) ^ set(hip))
    tail = (sig.shape[2] - 1) % pool
    if tail:           # past the last window pred's gradient is the NLL head's alone: nonzero, and part of the comparison
        assert float(hip["dpred"][:, :, -tail:].abs().max()) > 0
    label = "joint %s %s" % (precision, case)
    ok = verdicts(hip, exact, rounded, precision, label)
    bad = sorted(k for k, v in ok.items() if not v)
    assert not bad, (label, bad)
    for m in mutants:
        e2, r2 = refs(m)
        ok2 = verdicts(hip, e2, r2, precision, label + " mutant " + m, quiet=True)
        rej = sorted(k for k, v in ok2.items() if not v)
        print("%s mutant %s: rejected by %d of %d tensors, e.g. %s" % (label, m, len(rej), len(ok2), rej[:3]))
        assert rej, "mutant %s passes" % m


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_joint_step_vs_fp64(case, precision):
    check_joint(case, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_wrong_joint_steps_are_rejected(precision):
    """only the reference side changes: the NLL term scaled by B, the CTC term not divided by T', the classifier's input gradient
    missing from pred's cotangent, labels not shifted past the blank"""
    check_joint("levels256_64ch_pool3", precision, mutants=MUTANTS)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_graphed_joint_step_equals_the_eager_step(precision):
    """GraphedStep replays the joint step: both losses and every gradient bitwise those of the eager step on the same inputs"""
    import wavenet_speech_amd as W
    from wavenet_speech_amd import training as T
    wavenet, ctcnet, sig, seq, lengths, wl, cl, pool = make_case("one_utterance")
    nets = []
    for _ in range(2):
        w, c = copy.deepcopy(wavenet).to(DEV), copy.deepcopy(ctcnet).to(DEV)
        W.set_precision(w, precision)
        W.set_precision(c, precision)
        nets.append((w, c))
    sg, sq, ln = sig.to(DEV), seq.to(DEV), lengths.to(DEV)
    (w0, c0), (w1, c1) = nets
    xe, ctc, joint = T.joint_losses(w0, c0, sg, sq, ln)
    joint.backward()
    kept = {}

    def forward_loss():
        a, b, j = T.joint_losses(w1, c1, sg, sq, ln)
        kept["xe"], kept["ctc"] = a.detach(), b.detach()
        return j
    g = W.GraphedStep(forward_loss, list(w1.parameters()) + list(c1.parameters()), warmup=1)
    for _ in range(2):
        loss = g()
        g.check()
        assert float(loss) == float(joint.detach()) and float(kept["xe"]) == float(xe.detach()) and float(kept["ctc"]) == float(ctc.detach())
        for a, b in ((w0, w1), (c0, c1)):
            for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
                assert (p.grad is None) == (q.grad is None), k
                assert p.grad is None or torch.equal(p.grad, q.grad), k
