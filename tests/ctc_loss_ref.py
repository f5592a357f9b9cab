"""float64 log-space reference of the CTC loss and its gradient, vectorised over the blank-extended states (np.logaddexp on whole
rows), so it reaches the shapes oracle/ctc_oracle.py's T x S Python loop cannot: 2304 frames x 4095 states in about a second.
TEST INFRASTRUCTURE ONLY.  tests/test_ctc_loss_ref.py pins it to the loop oracle, to torch's float64 CPU ctc_loss and to closed
forms; tests/test_gpu_ctc_edges.py holds the HIP kernels (csrc/wn_ctc.hip) to it.

    ctc_ref(acts [B, C, T], labels [B, Lmax], label_lengths [B], blank=0, input_lengths=None) -> (nll [B], grad [B, C, T])

Graves et al. 2006, eqs. 5-16, warp-ctc's conventions: softmax inside, gradient with respect to the activations.  An infeasible
utterance gives +inf and a zero gradient; frames past input_lengths get a zero gradient; nothing of a label row past its length
is read; -inf logits are allowed (beta is kept WITHOUT the frame's own emission, so no occupancy divides by y = 0).

MUTANTS are named wrong variants of the same function (`ctc_ref(..., mutant=name)`): each is a mistake the device code could
make.  edge_cases(family) builds the inputs of tests/test_gpu_ctc_edges.py and names the mutant each one is there to catch;
the CPU test shows that every input separates the reference from its mutant by 100 times the device tolerance, i.e. that the
GPU test can fail.
"""
import numpy as np

MUTANTS = ("skip across repeats", "blank is 0", "input_lengths ignored", "labels read to Lmax", "beta labels unreversed",
           "linear rows scaled by their maximum")

LOSS_TOL = 2e-6          # relative to max(1, |nll|): the loss leaves the kernel as fp32 (2^-24 per utterance)
GRAD_TOL = 2e-6          # absolute: fp32 mantissas of alpha and beta in HBM (2 x 2^-24 per occupancy term) + fp32 output rounding


def log_softmax(acts):
    """acts [C, T] -> log softmax over C; -inf entries stay -inf (a frame needs one finite logit)"""
    m = acts.max(axis=0, keepdims=True)
    with np.errstate(divide="ignore"):
        return acts - m - np.log(np.exp(acts - m).sum(axis=0, keepdims=True))


def _extended(lab, blank):
    ext = np.full(2 * len(lab) + 1, blank, dtype=np.int64)
    ext[1::2] = lab
    return ext


def _skip(ext, blank, across_repeats=False):
    """skip[s]: the transition s-2 -> s exists (l'_s is a label and differs from l'_{s-2})"""
    skip = np.zeros(len(ext), dtype=bool)
    skip[2:] = ext[2:] != blank
    if not across_repeats:
        skip[2:] &= ext[2:] != ext[:-2]
    return skip


def _shift(row, n, fill):
    out = np.full_like(row, fill)
    out[n:] = row[:len(row) - n]
    return out


def _forward_log(logp, ext, skip):
    """alpha [T, S] in log space, and `pre` [T, S]: the same without frame t's own emission"""
    T, S = logp.shape[1], len(ext)
    em = logp[ext].T                                   # [T, S]
    alpha = np.full((T, S), -np.inf)
    pre = np.full((T, S), -np.inf)
    pre[0, :2] = 0.0                                   # paths start in the first blank or the first label
    alpha[0] = pre[0] + em[0]
    for t in range(1, T):
        prev = alpha[t - 1]
        p = np.logaddexp(prev, _shift(prev, 1, -np.inf))
        p = np.logaddexp(p, np.where(skip, _shift(prev, 2, -np.inf), -np.inf))
        pre[t] = p
        alpha[t] = p + em[t]
    return alpha, pre


def _forward_linear(y, ext, skip):
    """the plain linear float64 recursion, every row divided by its maximum (Rabiner's scaling); returns the scaled rows, the
    scaled rows without their own emission, and the log of the accumulated scale per row"""
    T, S = y.shape[1], len(ext)
    em = y[ext].T
    alpha = np.zeros((T, S))
    pre = np.zeros((T, S))
    logscale = np.zeros(T)
    pre[0, :2] = 1.0
    acc = 0.0
    with np.errstate(all="ignore"):
        for t in range(T):
            if t:
                prev = alpha[t - 1]
                pre[t] = prev + _shift(prev, 1, 0.0) + np.where(skip, _shift(prev, 2, 0.0), 0.0)
            row = pre[t] * em[t]
            m = row.max()
            alpha[t] = row / m
            pre[t] = pre[t] / m
            acc += np.log(m)
            logscale[t] = acc
    return alpha, pre, logscale


def tables(acts, lab, blank=0, mutant=None):
    """one utterance: acts [C, T] (T >= 1), lab: the labels.  Returns (ext [S], log alpha [T, S], log beta~ [T, S], log p);
    beta~ is beta without frame t's emission, so the occupancy of state s at frame t is exp(alpha + beta~ - log p)."""
    acts = np.asarray(acts, dtype=np.float64)
    lab = np.asarray(lab, dtype=np.int64)
    C, T = acts.shape
    if len(lab) and (lab.min() < 0 or lab.max() >= C):
        return None                                    # only a mutant gets here (it read the padding)
    ext = _extended(lab, blank)
    S = len(ext)
    skip = _skip(ext, blank, across_repeats=mutant == "skip across repeats")
    rext = ext if mutant == "beta labels unreversed" else ext[::-1]
    rskip = _skip(rext, blank, across_repeats=mutant == "skip across repeats")
    logp = log_softmax(acts)
    with np.errstate(all="ignore"):
        if mutant == "linear rows scaled by their maximum":
            y = np.exp(logp)
            a, _, ascale = _forward_linear(y, ext, skip)
            _, bpre, bscale = _forward_linear(y[:, ::-1], rext, rskip)
            alpha = np.log(a) + ascale[:, None]
            beta = (np.log(bpre) + np.concatenate(([0.0], bscale[:-1]))[:, None])[::-1, ::-1]
        else:
            alpha, _ = _forward_log(logp, ext, skip)
            _, bpre = _forward_log(logp[:, ::-1], rext, rskip)
            beta = bpre[::-1, ::-1]
        ll = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, S - 1]
    return ext, alpha, beta, ll


def _one(acts, lab, blank, mutant):
    """(nll, grad [C, T]) of one utterance"""
    C, T = acts.shape
    grad = np.zeros((C, T))
    if T == 0:
        return (0.0 if len(lab) == 0 else np.inf), grad
    tab = tables(acts, lab, blank, mutant)
    if tab is None:
        return np.nan, np.full((C, T), np.nan)
    ext, alpha, beta, ll = tab
    if np.isnan(ll):
        return np.nan, np.full((C, T), np.nan)
    if ll == -np.inf:
        return np.inf, grad
    with np.errstate(all="ignore"):
        occ = np.exp(alpha + beta - ll)                # [T, S]
        grad = np.exp(log_softmax(acts))
        for c in np.unique(ext):
            grad[c] -= occ[:, ext == c].sum(axis=1)
    return -ll, grad


def ctc_ref(acts, labels, label_lengths, blank=0, input_lengths=None, mutant=None):
    """acts [B, C, T]; labels [B, Lmax] (any padding past label_lengths); returns (nll [B], grad [B, C, T]) in float64"""
    assert mutant is None or mutant in MUTANTS, mutant
    acts = np.asarray(acts, dtype=np.float64)
    labels = np.asarray(labels).reshape(acts.shape[0], -1)
    B, C, T = acts.shape
    if mutant == "blank is 0":
        blank = 0
    nll, grad = np.zeros(B), np.zeros_like(acts)
    for b in range(B):
        tb = T if input_lengths is None or mutant == "input_lengths ignored" else int(input_lengths[b])
        lb = labels.shape[1] if mutant == "labels read to Lmax" else int(label_lengths[b])
        nll[b], grad[b][:, :tb] = _one(acts[b][:, :tb], labels[b][:lb], int(blank), mutant)
    return nll, grad


# ---- closed forms: no recursion anywhere ------------------------------------------------------------------------------------------
def single_path(lab, blank=0):
    """the one alignment of `lab` in exactly len(lab) + (adjacent repeats) frames: a blank between equal neighbours only"""
    path = []
    for j, l in enumerate(lab):
        if j and lab[j - 1] == l:
            path.append(int(blank))
        path.append(int(l))
    return path


def closed_form_path(acts, path):
    """acts [C, T] and the only alignment `path` [T]: nll = -sum_t log y_t(path_t), grad = y - onehot(path)"""
    logp = log_softmax(np.asarray(acts, dtype=np.float64))
    t = np.arange(logp.shape[1])
    grad = np.exp(logp)
    grad[np.asarray(path), t] -= 1.0
    return -logp[np.asarray(path), t].sum(), grad


def min_frames(lab):
    lab = list(lab)
    return len(lab) + sum(1 for j in range(1, len(lab)) if lab[j] == lab[j - 1])


def row_gap(acts, lab, blank=0, occupancy=0.5):
    """the largest distance in nats, over frames t and states s holding more than `occupancy` of the probability at t, from
    log alpha_t(s) to the largest log alpha of row t: what a row kept in one common scale would have to span"""
    ext, alpha, beta, ll = tables(acts, lab, blank)
    occ = np.exp(alpha + beta - ll)
    gap = alpha.max(axis=1, keepdims=True) - alpha
    return float(gap[occ > occupancy].max())


# ---- the inputs of tests/test_gpu_ctc_edges.py -------------------------------------------------------------------------------------
def f32(a):
    """the device reads fp32 activations: round once, so both sides see the same numbers"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def random_labels(rng, C, n, blank=0):
    pool = np.array([c for c in range(C) if c != blank])
    return pool[rng.integers(0, len(pool), size=n)]


def pad_rows(rows, fill=None, width=None, C=5, blank=0, rng=None):
    """rows of labels -> ([B, Lmax] int64, lengths [B]); the tail is `fill`, or random valid labels for fill=None"""
    width = max([len(r) for r in rows] + [1]) if width is None else width
    rng = np.random.default_rng(99) if rng is None else rng
    out = random_labels(rng, C, (len(rows), width), blank) if fill is None else np.full((len(rows), width), fill, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out.astype(np.int64), np.array([len(r) for r in rows], dtype=np.int64)


def case(name, acts, rows, mutant, blank=0, input_lengths=None, fill=None, width=None):
    acts = f32(acts)
    labels, lens = pad_rows(rows, fill=fill, width=width, C=acts.shape[1], blank=blank)
    return dict(name=name, acts=acts, labels=labels, lens=lens, blank=blank, mutant=mutant,
                input_lengths=None if input_lengths is None else np.asarray(input_lengths, dtype=np.int64))


def wide_row_case(seed=7):
    """T = 40, class 1 raised by 80 on the first 28 frames, labels [1] + [2, 3] * 12: the 12 tail frames cannot hold the 24
    remaining labels, so every alignment spends labels inside the peaked region, far below the all-ones state of those rows"""
    rng = np.random.default_rng(seed)
    acts = rng.normal(size=(1, 5, 40))
    acts[0, 1, :28] += 80.0
    return case("wide_row", acts, [[1] + [2, 3] * 12], "linear rows scaled by their maximum")


def long_case():
    """B=1, C=64, T=2304, L=2047: all 8 state slots of a pass thread live, S = 4095; T leaves room for the repeats"""
    rng = np.random.default_rng(2047)
    lab = random_labels(rng, 64, 2047)
    assert min_frames(lab) <= 2304
    return case("L2047", rng.normal(size=(1, 64, 2304)) * 1.5, [lab], "skip across repeats")


FAMILIES = ("a_range", "b_slots", "c_frames", "d_closed", "e_classes", "f_blank", "g_padding", "h_independence", "i_forms",
            "j_bad_lengths", "k_neg_inf")
FRAME_COUNTS = (31, 32, 33, 63, 64, 65)
D_LABELS = [1, 1, 2, 3, 3, 3]
D_PATH = [1, 0, 1, 2, 3, 0, 3, 0, 3]
PAD_FILLS = (0, -1, 105, None)                         # C + 100 at C = 5; None: random valid labels


def slot_case(L):
    rng = np.random.default_rng(1000 + L)
    lab = random_labels(rng, 5, L)
    return case("L%d" % L, rng.normal(size=(1, 5, min_frames(lab) + 40)) * 1.5, [lab], "skip across repeats")


def frame_case(T, ragged):
    rng = np.random.default_rng(300 + T)
    if not ragged:
        return case("T%d" % T, rng.normal(size=(2, 3, T)) * 1.5, [[1, 2, 2, 1, 2, 2], [1, 2]], "beta labels unreversed")
    in_len = [v for v in dict.fromkeys((T, 33, 32, 17, 16, 1)) if v <= T]
    rows = [random_labels(rng, 3, 1 if v == 1 else 2 + i % 4) for i, v in enumerate(in_len)]      # all feasible: L <= 5 in >= 16 frames
    return case("T%d_ragged" % T, rng.normal(size=(len(in_len), 3, T)) * 1.5, rows, "input_lengths ignored", input_lengths=in_len)


def padding_case(fill):
    rng = np.random.default_rng(71)
    acts = rng.normal(size=(3, 5, 20)) * 1.5
    return case("pad_%s" % fill, acts, [[1, 2, 2], [], [4, 3, 1, 1, 2]], "labels read to Lmax", fill=fill, width=8)


def bad_length_case():
    """three good utterances (input_lengths below T); test j overwrites one length of utterance 1"""
    rng = np.random.default_rng(91)
    return case("bad_lengths", rng.normal(size=(3, 5, 24)) * 1.5, [[1, 2, 3, 3], [2, 4], [4, 1, 1]], "input_lengths ignored",
                input_lengths=[20, 24, 17], width=6)


def edge_cases(family):
    """the inputs of one family of tests/test_gpu_ctc_edges.py, each with the mutant it must separate from the reference"""
    rng = np.random.default_rng(FAMILIES.index(family) + 40)
    if family == "a_range":
        peaked = case("peaked", rng.normal(size=(2, 5, 64)) * 40.0, [random_labels(rng, 5, 8), random_labels(rng, 5, 5)],
                      "linear rows scaled by their maximum")
        return [peaked, wide_row_case()]
    if family == "b_slots":
        lab = random_labels(rng, 5, 300)
        mixed = case("L300_and_L3", rng.normal(size=(2, 5, min_frames(lab) + 40)) * 1.5, [lab, [2, 2, 1]], "labels read to Lmax")
        return [long_case()] + [slot_case(L) for L in (255, 256, 511, 512)] + [mixed]
    if family == "c_frames":
        zero = case("no_frames", rng.normal(size=(3, 3, 9)) * 1.5, [[], [1, 2], [2, 1]], "input_lengths ignored",
                    input_lengths=[0, 0, 9])
        return [frame_case(T, r) for T in FRAME_COUNTS for r in (False, True)] + [zero]
    if family == "d_closed":
        # utterance 0: no labels (its row holds valid padding); 1: exactly feasible in 9 frames; 2: one frame short of feasible
        return [case("closed", rng.normal(size=(3, 5, 9)) * 1.5, [[], D_LABELS, D_LABELS], "skip across repeats",
                     input_lengths=[9, 9, 8]),
                case("closed_pad", rng.normal(size=(3, 5, 9)) * 1.5, [[], D_LABELS, D_LABELS], "labels read to Lmax",
                     input_lengths=[9, 9, 8], width=8)]
    if family == "e_classes":
        return [case("C2", rng.normal(size=(2, 2, 12)) * 1.5, [[1] * 5, [1]], "skip across repeats"),
                case("C63", rng.normal(size=(2, 63, 17)) * 1.5, [random_labels(rng, 63, 6), random_labels(rng, 63, 3)],
                     "beta labels unreversed"),
                case("C64", rng.normal(size=(2, 64, 17)) * 1.5, [random_labels(rng, 64, 6), random_labels(rng, 64, 3)],
                     "beta labels unreversed")]
    if family == "f_blank":
        out = []
        for blank in (0, 2, 4):
            pool = np.array([c for c in range(5) if c != blank])     # label 0 is an ordinary class wherever the blank is elsewhere
            rows = [pool[[0, 1, 1, 2, 3, 0]], pool[[2, 3, 0]]]
            out.append(case("blank%d" % blank, rng.normal(size=(2, 5, 25)) * 1.5, rows,
                            "blank is 0" if blank else "beta labels unreversed", blank=blank))
        return out
    if family == "g_padding":
        return [padding_case(fill) for fill in PAD_FILLS]
    if family == "h_independence":
        return [case("independent", rng.normal(size=(3, 5, 30)) * 1.5, [[1, 2, 2, 4], [3], [4, 4, 1, 2, 3, 1, 2]], "labels read to Lmax")]
    if family == "i_forms":
        return [case("forms", rng.normal(size=(2, 6, 21)) * 1.5, [[1, 5, 2, 2], [3, 4, 1]], "beta labels unreversed")]
    if family == "j_bad_lengths":
        return [bad_length_case()]
    if family == "k_neg_inf":
        acts = rng.normal(size=(1, 5, 20)) * 1.5
        acts[0, 2, 3:9] = -np.inf
        return [case("neg_inf", acts, [[1, 2, 3]], "beta labels unreversed")]
    raise KeyError(family)


def reference(c, mutant=None):
    return ctc_ref(c["acts"], c["labels"], c["lens"], blank=c["blank"], input_lengths=c["input_lengths"], mutant=mutant)
