"""CPU reference of CTC forced alignment (wavenet_speech_amd.ctc_forced_align, csrc/wn_align.hip), numpy float64.

Definition.  lp [C][T] are frame log-probabilities, l' the blank-extended labelling of S = 2 L + 1 states (even s: the blank,
odd s: label (s - 1) / 2).  A path pi_0 .. pi_{T-1} starts in state 0 or 1, ends in state S - 1 or S - 2 and moves by 0, +1, or
+2, the +2 move only onto a state that is not a blank and whose label differs from l'_{s-2}.  Its score is
sum_t lp[l'_{pi_t}][t]; the alignment is the path of maximum score.

Tie rule (part of the contract): at every (t, s) the predecessors are tried in the order s, s - 1, s - 2 and a later one
replaces an earlier one only if strictly greater; the final state is S - 1 unless delta(S - 2) is strictly greater; the path
is the back-trace of those backpointers."""
import itertools

import numpy as np


def extended(labels, blank):
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(labels, dtype=np.int64)
    return ext


def log_softmax(x):
    """x [C][T] float64 -> x - (m + log sum exp(x - m)), the order of operations the device uses"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=0, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=0, keepdims=True)))


def to_log_probs(x, kind):
    """the fp64 frame log-probabilities of an input tensor [C][T] of the given kind ("logits", "probs", "log_probs")"""
    x = np.asarray(x, dtype=np.float64)
    if kind == "logits":
        return log_softmax(x)
    if kind == "probs":
        with np.errstate(divide="ignore"):
            return np.log(x)
    assert kind == "log_probs"
    return x


def _skip_mask(ext, blank):
    S = len(ext)
    skip = np.zeros(S, dtype=bool)
    if S > 2:
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return skip


def _forward(lp, ext, skip):
    """delta [T][S] (emission of frame t included) and backpointers [T][S] in {0, 1, 2} under the tie rule"""
    T, S = lp.shape[1], len(ext)
    em = lp[ext, :].T                                    # [T][S]
    delta = np.full((T, S), -np.inf)
    bp = np.zeros((T, S), dtype=np.int8)
    if T == 0:
        return delta, bp
    delta[0, 0] = em[0, 0]
    if S > 1:
        delta[0, 1] = em[0, 1]
    p1 = np.full(S, -np.inf)
    p2 = np.full(S, -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            prev = delta[t - 1]
            p1[1:] = prev[:-1]
            p2[2:] = prev[:-2]
            m = prev.copy()
            b = np.zeros(S, dtype=np.int8)
            k = p1 > m
            m[k] = p1[k]
            b[k] = 1
            k = skip & (p2 > m)
            m[k] = p2[k]
            b[k] = 2
            delta[t] = m + em[t]
            bp[t] = b
    return delta, bp


def spans_of(states, L):
    """[L][2]: first frame in state 2 j + 1 and one past the last"""
    spans = np.full((L, 2), -1, dtype=np.int32)
    for j in range(L):
        (idx,) = np.nonzero(states == 2 * j + 1)
        if len(idx):
            spans[j] = (idx[0], idx[-1] + 1)
    return spans


def viterbi_align(lp, labels, blank=0):
    """lp [C][T] float64 log-probabilities, labels: ints (no blanks).  Returns (states [T] int32, score, spans [L][2] int32).
    No alignment (or none of probability > 0): score -inf, states and spans all -1.  T = 0: score 0 if L = 0 else -inf."""
    lp = np.asarray(lp, dtype=np.float64)
    labels = [int(v) for v in labels]
    T, L = lp.shape[1], len(labels)
    none = (np.full(T, -1, dtype=np.int32), -np.inf, np.full((L, 2), -1, dtype=np.int32))
    if T == 0:
        return (none[0], 0.0 if L == 0 else -np.inf, none[2])
    ext = extended(labels, blank)
    S = len(ext)
    delta, bp = _forward(lp, ext, _skip_mask(ext, blank))
    s = S - 1
    if S >= 2 and delta[T - 1, S - 2] > delta[T - 1, S - 1]:
        s = S - 2
    score = float(delta[T - 1, s])
    if not score > -np.inf:
        return none
    states = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return states, score, spans_of(states, L)


def frame_labels_of(states, labels, blank=0):
    ext = extended(labels, blank)
    return np.where(states >= 0, ext[np.maximum(states, 0)], -1).astype(np.int32)


def path_score(lp, labels, states, blank=0):
    """score of a given path under lp (and a check that it is a legal alignment of the labels)"""
    lp = np.asarray(lp, dtype=np.float64)
    ext = extended(labels, blank)
    S, T = len(ext), lp.shape[1]
    states = np.asarray(states, dtype=np.int64)
    assert len(states) == T and states[0] in (0, 1) and states[-1] in (S - 1, S - 2) and states.min() >= 0
    step = np.diff(states)
    assert ((step >= 0) & (step <= 2)).all()
    two = np.nonzero(step == 2)[0] + 1
    assert (_skip_mask(ext, blank)[states[two]]).all()
    return float(lp[ext[states], np.arange(T)].sum())


def frame_margins(lp, labels, states, blank=0):
    """[T]: score of the optimum minus the best score of a path that is NOT in state states[t] at frame t (forward plus backward
    max-marginals); +inf where no other state lies on a path of probability > 0"""
    lp = np.asarray(lp, dtype=np.float64)
    ext = extended(labels, blank)
    S, T = len(ext), lp.shape[1]
    skip = _skip_mask(ext, blank)
    delta, _ = _forward(lp, ext, skip)
    em = lp[ext, :].T
    beta = np.full((T, S), -np.inf)                      # best continuation from (t, s), emission of frame t excluded
    beta[T - 1, S - 1] = 0.0
    if S >= 2:
        beta[T - 1, S - 2] = 0.0
    n1 = np.full(S, -np.inf)
    n2 = np.full(S, -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(T - 2, -1, -1):
            nxt = beta[t + 1] + em[t + 1]
            n1[:-1] = nxt[1:]
            n2[:-2] = np.where(skip[2:], nxt[2:], -np.inf)
            beta[t] = np.maximum(nxt, np.maximum(n1, n2))
        through = delta + beta                           # best path through (t, s)
    through[np.isnan(through)] = -np.inf
    best = through[np.arange(T), states].copy()
    through[np.arange(T), states] = -np.inf
    with np.errstate(invalid="ignore"):
        return best - through.max(axis=1)


def collapse(path, blank=0):
    out, prev = [], None
    for v in path:
        v = int(v)
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def best_score_by_enumeration(lp, labels, blank=0):
    """max over all C^T frame strings that collapse to `labels` of their score; -inf if there is none"""
    lp = np.asarray(lp, dtype=np.float64)
    C, T = lp.shape
    want = [int(v) for v in labels]
    best = -np.inf
    for path in itertools.product(range(C), repeat=T):
        if collapse(path, blank) == want:
            best = max(best, float(sum(lp[c, t] for t, c in enumerate(path))))
    if T == 0:
        return 0.0 if not want else -np.inf
    return best
