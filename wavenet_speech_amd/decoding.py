"""
CTC decoding on the device: the tail every reference evaluation notebook runs after RawCTCNet / WaveNetClassifier
(softmax, argmax_decode + labels2strings of modules/sequence_decoders.py, then ctcdecode's CTCBeamDecoder), as HIP kernels
(csrc/wn_decode.hip) that read the model's [B][C][T] output in place.

    labels, lengths, frames = ctc_greedy_decode(logits)                        # argmax, repeats collapsed, blanks dropped
    labels, lengths, scores, frames = ctc_beam_decode(logits, beam_width=8)    # CTC prefix beam search, no language model
    labels_to_strings(labels[:, 0], lengths[:, 0])                             # host: " AGCT" lookup, 0 = blank

and CTC forced alignment (csrc/wn_align.hip): the best single alignment of a KNOWN label sequence to the frames,

    states, frame_labels, spans, score = ctc_forced_align(logits, targets, target_lengths)   # spans[b, j] = [first, end) frames

and global pairwise alignment with affine gaps (csrc/wn_pairalign.hip): how close a decoded read is to the truth, the
step the reference's evaluation notebook hands to EMBOSS needle,

    r = pairwise_align(targets, target_lengths, labels, lengths)     # r.score, r.matches, r.gaps, r.length, r.identity, r.ops
    edit_distance(targets, target_lengths, labels, lengths)          # Levenshtein distance, int32 [B]
    print("\n".join(format_alignment(targets[0], labels[0], r.ops[0])))

and per-base quality scores (csrc/wn_quality.hip): how much to trust each decoded base when the truth is not known,

    q = ctc_base_qualities(logits, labels, lengths, frames)          # q.error, q.qual, q.dwell, q.read_error, q.mean_qscore
    print("".join(fastq_records(names, labels, lengths, q.qual)))    # host: "@name\nSEQ\n+\nQUAL\n" per read

Results stay on the device (int32 labels / frames / lengths, fp32 scores); nothing is copied to the host.  Scores are the
natural log probability of each prefix summed over the alignments the search kept (higher is better), sorted descending.
There is no CPU fallback: CPU tensors raise.
"""
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream

MAX_CLASSES = 64
MAX_BEAM_WIDTH = 64
MAX_ALIGN_LABELS = 2047
INPUT_KINDS = {"logits": 0, "probs": 1, "log_probs": 2}
LAYOUTS = ("BCT", "BTC")
DEFAULT_ALPHABET = " AGCT"          # the reference's lookup (Decoder.py:26): 0 = blank, 1..4 = A, G, C, T


def _prep(x, layout, input_lengths, what):
    x = _args.gpu_tensor(x, what, "input")
    if x.dim() != 3:
        raise ValueError("wavenet_speech_amd.%s: input must be 3-d, got shape %s" % (what, tuple(x.shape)))
    if layout not in LAYOUTS:
        raise ValueError("wavenet_speech_amd.%s: layout must be one of %s, got %r" % (what, LAYOUTS, layout))
    if not x.is_floating_point():
        raise TypeError("wavenet_speech_amd.%s: input must be floating point, got %s" % (what, x.dtype))
    if x.dtype != torch.float32:
        x = x.float()
    if layout == "BCT":
        B, C, T = x.shape
        sb, sc, st = x.stride()
    else:
        B, T, C = x.shape
        sb, st, sc = x.stride()
    if B < 1 or T < 1 or C < 2:
        raise ValueError("wavenet_speech_amd.%s: need batch >= 1, length >= 1 and classes >= 2, got B=%d C=%d T=%d"
                         % (what, B, C, T))
    if C > MAX_CLASSES:
        raise ValueError("wavenet_speech_amd.%s: at most %d classes, got %d" % (what, MAX_CLASSES, C))
    if input_lengths is not None:
        input_lengths = torch.as_tensor(input_lengths)
        if input_lengths.shape != (B,):
            raise ValueError("wavenet_speech_amd.%s: input_lengths must have shape (%d,), got %s"
                             % (what, B, tuple(input_lengths.shape)))
        input_lengths = input_lengths.to(device=x.device, dtype=torch.int64).contiguous()
    return x, (B, C, T), (sb, sc, st), input_lengths


def _note(bad, C, blank, what):
    _args.note_bad(bad, lambda n, C=C, blank=blank: "wavenet_speech_amd.%s: input_lengths outside [0, T] or blank (%d) outside "
                   "[0, %d) in %d utterance(s)" % (what, blank, C, n))


def ctc_greedy_decode(x, blank=0, input_lengths=None, layout="BCT"):
    """argmax per frame (ties to the lowest class, as torch.argmax), repeats collapsed, blanks dropped.
    x: [B, C, T] (or [B, T, C] with layout="BTC") logits, probabilities or log-probabilities -- any of them, the argmax is the
    same.  Returns (labels [B, T] int32 zero-padded, lengths [B] int32, frames [B, T] int32: the frame of each label)."""
    x, (B, C, T), (sb, sc, st), in_len = _prep(x, layout, input_lengths, "ctc_greedy_decode")
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        labels = torch.empty(B, T, dtype=torch.int32, device=dev)
        frames = torch.empty(B, T, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_ctc_greedy_decode(_p(x), sb, sc, st, _p(in_len), B, C, T, int(blank), _p(labels), _p(frames),
                                            _p(lengths), _p(bad), _stream()), "wn_ctc_greedy_decode")
        _note(bad, C, int(blank), "ctc_greedy_decode")
    return labels, lengths, frames


def ctc_beam_decode(x, beam_width, blank=0, input_lengths=None, input="logits", layout="BCT"):
    """CTC prefix beam search without a language model.
    x: [B, C, T] (layout="BCT", the model's own output) or [B, T, C] (layout="BTC", ctcdecode's), read in place through its
    strides; input: "logits" (log-softmax over the classes is applied inside, as the CTC loss does), "probs" or "log_probs".
    Returns (labels [B, W, T] int32 zero-padded, lengths [B, W] int32, scores [B, W] fp32, frames [B, W, T] int32).
    scores: natural log probability, higher is better, sorted descending; slots beyond the distinct prefixes found have
    length 0 and score -inf.  frames: the frame at which each label was emitted on the beam's backpointer path."""
    if input not in INPUT_KINDS:
        raise ValueError("wavenet_speech_amd.ctc_beam_decode: input must be one of %s, got %r" % (sorted(INPUT_KINDS), input))
    W = int(beam_width)
    if W < 1 or W > MAX_BEAM_WIDTH:
        raise ValueError("wavenet_speech_amd.ctc_beam_decode: beam_width must be in [1, %d], got %d" % (MAX_BEAM_WIDTH, W))
    x, (B, C, T), (sb, sc, st), in_len = _prep(x, layout, input_lengths, "ctc_beam_decode")
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        ws_bytes = lib.wn_ctc_decode_workspace_bytes(B, C, T, W)
        if ws_bytes == 0:
            _lib.check(lib.wn_ctc_beam_decode(None, sb, sc, st, INPUT_KINDS[input], None, B, C, T, int(blank), W, None, None,
                                              None, None, None, 0, None, None), "wn_ctc_beam_decode")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        labels = torch.empty(B, W, T, dtype=torch.int32, device=dev)
        frames = torch.empty(B, W, T, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, W, dtype=torch.int32, device=dev)
        scores = torch.empty(B, W, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_ctc_beam_decode(_p(x), sb, sc, st, INPUT_KINDS[input], _p(in_len), B, C, T, int(blank), W, _p(labels),
                                          _p(frames), _p(lengths), _p(scores), _p(ws), ws_bytes, _p(bad), _stream()),
                   "wn_ctc_beam_decode")
        _note(bad, C, int(blank), "ctc_beam_decode")
    return labels, lengths, scores, frames


CTCAlignment = namedtuple("CTCAlignment", "states frame_labels spans score")


def ctc_forced_align(x, targets, target_lengths, input_lengths=None, blank=0, input="logits", layout="BCT"):
    """The best single CTC alignment (Viterbi path) of known labels to the frames.
    x, input, layout, input_lengths: as ctc_beam_decode.  targets: [B, Lmax] labels of any integer dtype (values in [0, C),
    none equal to blank), target_lengths: [B].  Returns CTCAlignment, all on the device:
      states [B, T] int32        state of the blank-extended labelling per frame (even: a blank, odd s: label (s - 1) // 2), -1 past
                                 the utterance
      frame_labels [B, T] int32  the class of that state, -1 in the same places
      spans [B, Lmax, 2] int32   label j occupies frames [spans[b, j, 0], spans[b, j, 1]); rows past target_lengths[b] are -1
      score [B] fp32             log-probability of the path; -inf (and every entry -1) when no alignment fits
    Ties go to the lower move: stay before advance before skip, the final blank before the final label.  A bad label or length
    gives score NaN and every entry -1, and is reported through check_device_flags()."""
    what = "ctc_forced_align"
    if input not in INPUT_KINDS:
        raise ValueError("wavenet_speech_amd.%s: input must be one of %s, got %r" % (what, sorted(INPUT_KINDS), input))
    x, (B, C, T), (sb, sc, st), in_len = _prep(x, layout, input_lengths, what)
    dev = x.device
    targets, target_lengths = torch.as_tensor(targets), torch.as_tensor(target_lengths)
    if targets.is_floating_point() or targets.dtype == torch.bool or targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("wavenet_speech_amd.%s: targets must be integers of shape (%d, Lmax), got %s %s"
                         % (what, B, targets.dtype, tuple(targets.shape)))
    if target_lengths.shape != (B,):
        raise ValueError("wavenet_speech_amd.%s: target_lengths must have shape (%d,), got %s" % (what, B, tuple(target_lengths.shape)))
    lmax = width = int(targets.shape[1])
    if lmax > MAX_ALIGN_LABELS:
        raise ValueError("wavenet_speech_amd.%s: at most %d labels per utterance, got %d" % (what, MAX_ALIGN_LABELS, lmax))
    if not 0 <= int(blank) < C:
        raise ValueError("wavenet_speech_amd.%s: blank must be in [0, %d), got %d" % (what, C, int(blank)))
    targets = targets.to(device=dev, dtype=torch.int64).contiguous()
    target_lengths = target_lengths.to(device=dev, dtype=torch.int64).contiguous()
    if lmax == 0:                                                    # the C ABI wants one column; no utterance may use it
        lmax, targets = 1, torch.zeros(B, 1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws_bytes = lib.wn_ctc_align_workspace_bytes(B, C, T, lmax)
        if ws_bytes == 0:
            _lib.check(lib.wn_ctc_align(None, sb, sc, st, INPUT_KINDS[input], None, None, None, B, C, T, lmax, int(blank), None, None,
                                        None, None, None, 0, None, None), "wn_ctc_align")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        states = torch.empty(B, T, dtype=torch.int32, device=dev)
        frame_labels = torch.empty(B, T, dtype=torch.int32, device=dev)
        spans = torch.empty(B, lmax, 2, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_ctc_align(_p(x), sb, sc, st, INPUT_KINDS[input], _p(targets), _p(target_lengths), _p(in_len), B, C, T, lmax,
                                    int(blank), _p(states), _p(frame_labels), _p(spans), _p(score), _p(ws), ws_bytes, _p(bad),
                                    _stream()), "wn_ctc_align")
        _args.note_bad(bad, lambda n, C=C, blank=int(blank): "wavenet_speech_amd.ctc_forced_align: labels outside [0, %d), equal to "
                       "the blank (%d), or lengths out of range in %d utterance(s)" % (C, blank, n))
    return CTCAlignment(states, frame_labels, spans[:, :width], score)


MAX_PAIR_QUERY = 8192
MAX_PAIR_REF = 65535
MAX_OPS = MAX_PAIR_REF + MAX_PAIR_QUERY       # op columns of a row: what pileup, pileup_evidence and left_align take
TILE = 256                                    # op columns per tile of the kernels that walk an op row (kPThreads in csrc/wn_opscan.h)
OP_PAD, OP_MATCH, OP_MISMATCH, OP_REF_GAP, OP_QUERY_GAP = 0, 1, 2, 3, 4


class PairwiseAlignment(namedtuple("PairwiseAlignment", "score matches mismatches gaps length ops ops_len")):
    """score [B] fp32; matches, mismatches, gaps (gap columns, end gaps included), length [B] int32; ops [B, N + M] uint8 front
    to back (1 match, 2 mismatch, 3 reference label against a gap, 4 query label against a gap, 0 padding) with ops_len [B]
    int32 -- ops and ops_len are None with return_ops=False.  All on the device."""
    __slots__ = ()

    @property
    def identity(self):
        """matches / length per pair (fp32, NaN for an empty alignment), as needle's 'Identity'"""
        return self.matches.float() / self.length.float()


def _pair_rows(rows, lengths, what, name):
    """label rows of any width (none: one unused column; labels are compared for equality only) with their [B] lengths"""
    rows = _args.int_rows(rows, what, name, pad_empty=True, lone_column_in_place=False)
    return rows, _args.lengths(lengths, int(rows.shape[0]), rows.device, what, name + "_lengths")


def _pair_align(what, ref, ref_lengths, query, query_lengths, costs, end_gaps_free, want_stats, want_ops):
    ref, ref_lengths = _pair_rows(ref, ref_lengths, what, "ref")
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, N, M = int(ref.shape[0]), int(ref.shape[1]), int(query.shape[1])
    if query.shape[0] != B or query.device != ref.device:
        raise ValueError("wavenet_speech_amd.%s: ref and query must hold the same number of rows on one device" % what)
    if B < 1:
        raise ValueError("wavenet_speech_amd.%s: need at least one pair" % what)
    if N > MAX_PAIR_REF or M > MAX_PAIR_QUERY:
        raise ValueError("wavenet_speech_amd.%s: at most %d reference and %d query labels per pair, got %d and %d"
                         % (what, MAX_PAIR_REF, MAX_PAIR_QUERY, N, M))
    lib = _lib.load()
    dev = ref.device
    with torch.cuda.device(dev):
        score = torch.empty(B, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        stats = ops = ops_len = ws = None
        ws_bytes = 0
        if want_stats or want_ops:
            ws_bytes = lib.wn_pair_align_workspace_bytes(B, N, M)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
        if want_ops:
            ops = torch.empty(B, N + M, dtype=torch.uint8, device=dev)
            ops_len = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_pair_align(_p(ref), ref.stride(0), _p(ref_lengths), _p(query), query.stride(0), _p(query_lengths), B, N, M,
                                     costs[0], costs[1], costs[2], costs[3], int(bool(end_gaps_free)), _p(score), _p(stats), _p(ops),
                                     _p(ops_len), _p(ws), ws_bytes, _p(bad), _stream()), "wn_pair_align")
        _args.note_bad(bad, lambda n, N=N, M=M: "wavenet_speech_amd.%s: ref_lengths outside [0, %d] or query_lengths outside "
                       "[0, %d] in %d pair(s)" % (what, N, M, n))
    return score, stats, ops, ops_len


def pairwise_align(ref, ref_lengths, query, query_lengths, match=5, mismatch=-4, gap_open=10, gap_extend=0.5, end_gaps_free=True,
                   return_ops=True):
    """Global alignment with affine gaps of query rows against reference rows.  The defaults are EMBOSS
    needle's for nucleotides as the reference's evaluation notebook runs it: EDNAFULL's 5 / -4 on A, C, G, T, gap open 10
    (a gap's first column), gap extend 0.5, end gaps not penalised.
    ref [B, N], query [B, M]: int32 or int64 GPU tensors with their lengths [B] -- `labels` / `lengths` of ctc_greedy_decode, a
    beam of ctc_beam_decode, `targets` / `target_lengths` as ctc_forced_align takes them: nothing passes through the host.
    Costs must be multiples of 0.5 (the kernel's arithmetic is integer, in half units: exact); the score comes back as fp32.
    Returns PairwiseAlignment.  Among equally scoring alignments the tie rule of DESIGN.md 7d decides, so needle may show
    another one of the same score.  A length outside its range poisons the pair (score -2^30, counts -1, ops_len 0) and is
    reported through check_device_flags()."""
    what = "pairwise_align"
    costs = _args.affine_costs(what, match, mismatch, gap_open, gap_extend)
    score, stats, ops, ops_len = _pair_align(what, ref, ref_lengths, query, query_lengths, costs, end_gaps_free, True, return_ops)
    if ops is not None:
        ops = ops[:, :int(ref.shape[1]) + int(query.shape[1])]       # a row without columns went in as one unused column
    return PairwiseAlignment(score.float() * 0.5, stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], ops, ops_len)


def edit_distance(a, a_lengths, b, b_lengths):
    """Levenshtein distance of every row pair, int32 [B] on the device: the score-only form of the alignment kernel with unit
    costs (no workspace, no trace).  -1 for a pair with a length outside its range (reported through check_device_flags())."""
    score, _, _, _ = _pair_align("edit_distance", a, a_lengths, b, b_lengths, (0, -1, 1, 1), False, False, False)
    return torch.where(score == -2 ** 31, torch.full_like(score, -1), -score)


MAX_BAND = 2048                               # diagonals of a stripe of banded_align
MAX_BANDED_LEN = 65535                        # labels of either row of banded_align; the tools downstream keep MAX_PAIR_QUERY


class BandedAlignment(namedtuple("BandedAlignment", "alignment status edge_hits diag_lo diag_hi")):
    """alignment: a PairwiseAlignment (every tool that takes pairwise_align's takes it); status [B] int8: 1 aligned, 0 no alignment
    inside the stripe (score -2^30, counts 0, ops_len 0), -1 a bad pair; edge_hits [B] int32: the path cells on the stripe's first
    or last diagonal, 0 when the stripe never held the path (None in the score-only form); diag_lo, diag_hi [B] int32: the stripes
    as the kernel took them.  All on the device."""
    __slots__ = ()


def banded_align(ref, ref_lengths, query, query_lengths, diag_lo, diag_hi, max_band, match=5, mismatch=-4, gap_open=10,
                 gap_extend=0.5, end_gaps_free=True, return_ops=True, score_only=False):
    """pairwise_align inside a stripe of diagonals per pair: cell (i, j) of reference label i against query
    label j takes part iff diag_lo[b] <= j - i <= diag_hi[b]; recurrence, tie rules, end-cell rule, costs and op rows are
    pairwise_align's.  Work and workspace go with (N + M) * max_band instead of N * M, and both rows may hold up to 65535 labels.
    diag_lo, diag_hi: [B] integers (band_from_ops and ReadMapping.band make them on the device); max_band: a host integer in
    [1, 2048], the widest stripe of the batch -- it sizes the launch and the workspace.  If the whole path of pairwise_align lies
    inside the stripe the result equals pairwise_align's, ties included; otherwise the score is at most its score.  A stripe
    that misses the rectangle (or, with end gaps penalised, its far corner) gives status 0; a length outside its range,
    diag_lo > diag_hi or a stripe wider than max_band poisons the pair (status -1; reported through check_device_flags()).
    return_ops=False leaves the op rows out (counts only); score_only=True runs no trace at all: counts, ops and edge_hits are None.
    Returns BandedAlignment."""
    what = "banded_align"
    costs = _args.affine_costs(what, match, mismatch, gap_open, gap_extend)
    ref, ref_lengths = _pair_rows(ref, ref_lengths, what, "ref")
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, N, M = int(ref.shape[0]), int(ref.shape[1]), int(query.shape[1])
    if query.shape[0] != B or query.device != ref.device:
        raise ValueError("wavenet_speech_amd.%s: ref and query must hold the same number of rows on one device" % what)
    if B < 1:
        raise ValueError("wavenet_speech_amd.%s: need at least one pair" % what)
    if N > MAX_BANDED_LEN or M > MAX_BANDED_LEN:
        raise ValueError("wavenet_speech_amd.%s: at most %d reference and query labels per pair, got %d and %d" % (what, MAX_BANDED_LEN, N, M))
    if isinstance(max_band, bool) or not isinstance(max_band, int) or not 1 <= max_band <= MAX_BAND:
        raise ValueError("wavenet_speech_amd.%s: max_band must be an integer in [1, %d], got %r" % (what, MAX_BAND, max_band))
    dev = ref.device
    diag_lo = _args.lengths(diag_lo, B, dev, what, "diag_lo")
    diag_hi = _args.lengths(diag_hi, B, dev, what, "diag_hi")
    lib = _lib.load()
    with torch.cuda.device(dev):
        score = torch.empty(B, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        stats = ops = ops_len = ws = edge_hits = None
        ws_bytes = 0
        if not score_only:
            ws_bytes = lib.wn_banded_align_workspace_bytes(B, N, M, max_band)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
            edge_hits = torch.empty(B, dtype=torch.int32, device=dev)
            if return_ops:
                ops = torch.empty(B, N + M, dtype=torch.uint8, device=dev)
                ops_len = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_banded_align(_p(ref), ref.stride(0), _p(ref_lengths), _p(query), query.stride(0), _p(query_lengths), _p(diag_lo),
                                       _p(diag_hi), B, N, M, max_band, costs[0], costs[1], costs[2], costs[3], int(bool(end_gaps_free)),
                                       _p(score), _p(stats), _p(ops), _p(ops_len), _p(status), _p(edge_hits), _p(ws), ws_bytes, _p(bad),
                                       _stream()), "wn_banded_align")
        _args.note_bad(bad, lambda n, N=N, M=M: "wavenet_speech_amd.%s: ref_lengths outside [0, %d], query_lengths outside [0, %d], "
                       "diag_lo > diag_hi or a stripe wider than max_band in %d pair(s)" % (what, N, M, n))
    cols = [None] * 4 if stats is None else [stats[:, k] for k in range(4)]
    return BandedAlignment(PairwiseAlignment(score.float() * 0.5, cols[0], cols[1], cols[2], cols[3], ops, ops_len), status, edge_hits,
                           diag_lo, diag_hi)


def _clamp_band(lo, hi, max_band):
    """[lo, hi] about its centre to at most max_band diagonals (tensors; None: as they are)"""
    if max_band is None:
        return lo, hi
    if isinstance(max_band, bool) or not isinstance(max_band, int) or max_band < 1:
        raise ValueError("wavenet_speech_amd: max_band must be a positive integer or None, got %r" % (max_band,))
    over = (hi - lo + 1 - max_band).clamp(min=0)
    lo = lo + torch.div(over, 2, rounding_mode="floor")
    return lo, torch.where(over > 0, lo + (max_band - 1), hi)


def band_from_ops(alignment, margin=0, max_band=None, end_gaps_free=True):
    """(diag_lo, diag_hi), [B] int32 on the device: the stripe of diagonals j - i the path of every op row of `alignment` (a
    PairwiseAlignment with ops) runs through, widened by `margin` on each side and, with max_band, clamped about its centre to that
    width.  The path is read off the row alone: with h the leading run of one gap kind and t the row's length less (with
    end_gaps_free) its trailing run of one gap kind, its cells are the cell before column h and the cell after every column in
    [h, t); a row of end gaps only is that single cell.  Under this stripe (margin 0) banded_align returns pairwise_align's result.
    torch ops on the device; nothing is read back."""
    what = "band_from_ops"
    ops, ops_len = _alignment_ops(alignment, what)
    if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
        raise ValueError("wavenet_speech_amd.%s: margin must be a non-negative integer, got %r" % (what, margin))
    B, P = int(ops.shape[0]), int(ops.shape[1])
    dev = ops.device
    n = ops_len.to(torch.int64).clamp(0, P)
    if P == 0:
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        return _clamp_band(zero - margin, zero + margin, max_band)
    col = torch.arange(P, device=dev).unsqueeze(0)
    inside = col < n.unsqueeze(1)
    first = ops[:, 0]
    last = ops.gather(1, (n - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
    # h: the columns before the first one that differs from a leading gap op; t: the same from the end
    differs = (ops != first.unsqueeze(1)) | ~inside
    h = torch.where(differs.any(1), differs.int().argmax(1), n)
    h = torch.where((first >= OP_REF_GAP) & (n > 0), h, torch.zeros_like(h))
    differs = ((ops != last.unsqueeze(1)) & inside).flip(1)          # from column P - 1 down
    run = torch.where(differs.any(1), differs.int().argmax(1) - (P - n), n)
    t = n - run if end_gaps_free else n
    t = torch.where((last >= OP_REF_GAP) & (n > 0), t, n)
    t = torch.maximum(t, h)
    step = ((ops != OP_REF_GAP) & inside).to(torch.int32) - ((ops != OP_QUERY_GAP) & inside).to(torch.int32)
    after = step.cumsum(1, dtype=torch.int32)                        # the diagonal after every column
    start = torch.where(h > 0, after.gather(1, (h - 1).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(after[:, 0]))
    on_path = (col >= h.unsqueeze(1)) & (col < t.unsqueeze(1))
    big = 1 << 30
    lo = torch.minimum(start, torch.where(on_path, after, torch.full_like(after, big)).amin(1))
    hi = torch.maximum(start, torch.where(on_path, after, torch.full_like(after, -big)).amax(1))
    return _clamp_band(lo - margin, hi + margin, max_band)


def format_alignment(ref_row, query_row, ops_row, alphabet=DEFAULT_ALPHABET):
    """host helper: the three text lines of one alignment as needle prints them -- the reference with '-' where the query has
    a label against a gap, '|' for a match and '.' for a mismatch, the query with '-' likewise.  alphabet[i] is the character
    of label i ('?' for a label outside it); ops_row may carry its zero padding."""
    ref = [int(v) for v in torch.as_tensor(ref_row).cpu().reshape(-1).tolist()]
    query = [int(v) for v in torch.as_tensor(query_row).cpu().reshape(-1).tolist()]
    char = lambda v: alphabet[v] if 0 <= v < len(alphabet) else "?"  # noqa: E731
    top, mid, bottom, i, j = [], [], [], 0, 0
    for op in torch.as_tensor(ops_row).cpu().reshape(-1).tolist():
        if op == OP_PAD:
            break
        if op in (OP_MATCH, OP_MISMATCH):
            top.append(char(ref[i])); mid.append("|" if op == OP_MATCH else "."); bottom.append(char(query[j]))
            i, j = i + 1, j + 1
        elif op == OP_REF_GAP:
            top.append(char(ref[i])); mid.append(" "); bottom.append("-")
            i += 1
        elif op == OP_QUERY_GAP:
            top.append("-"); mid.append(" "); bottom.append(char(query[j]))
            j += 1
        else:
            raise ValueError("format_alignment: op code %r" % (op,))
    return "".join(top), "".join(mid), "".join(bottom)


QUALITY_STATS = {"mean": 0, "best": 1}
MAX_QUAL = 93                       # the highest Phred value FASTQ can print ('~')

BaseQualities = namedtuple("BaseQualities", "error qual dwell read_error mean_qscore")
BaseQualities.__doc__ = """error [B, Lmax] fp32: the error probability of every base; qual [B, Lmax] uint8: its Phred quality in
[0, 93] (the FASTQ character is qual + 33); dwell [B, Lmax] int32: the frames of its run; read_error [B] fp32: the mean error of
the read's bases (NaN for an empty read); mean_qscore [B] fp32: qscale (-10 log10 read_error) + qbias.  All on the device."""


def ctc_base_qualities(x, labels, lengths, frames, input_lengths=None, blank=0, input="logits", layout="BCT", stat="mean",
                       qscale=1.0, qbias=0.0):
    """A Phred quality for every decoded base and a mean error per read.
    x, input, layout, input_lengths: as ctc_beam_decode -- the tensor the labels were decoded from.  labels, frames [B, Lmax]
    (int32 or int64, Lmax <= T) and lengths [B]: what ctc_greedy_decode returned, or one beam of ctc_beam_decode
    (labels[:, 0], frames[:, 0], lengths[:, 0]: read in place through their row stride).
    The run of a base is its emission frame and the frames after it, up to the next base's, for as long as the frame argmax
    stays its label.  The error of a frame is the softmax mass of every OTHER class (formed directly, never 1 - p); the error
    of the base is the mean over its run (stat="mean") or the least of it (stat="best").  Q = qscale (-10 log10 error) + qbias,
    rounded and clamped to [0, 93]; qscale / qbias are where a calibration against known reads goes.
    Returns BaseQualities; entries at and past lengths[b] are NaN / 0 / 0.  A base with a label outside [0, C) or equal to the
    blank, or a frame outside its utterance or not above its predecessor's, has error NaN, qual 0, dwell 0, makes its read's
    read_error NaN, and is reported through check_device_flags()."""
    what = "ctc_base_qualities"
    if input not in INPUT_KINDS:
        raise ValueError("wavenet_speech_amd.%s: input must be one of %s, got %r" % (what, sorted(INPUT_KINDS), input))
    if stat not in QUALITY_STATS:
        raise ValueError("wavenet_speech_amd.%s: stat must be one of %s, got %r" % (what, sorted(QUALITY_STATS), stat))
    qscale, qbias = float(qscale), float(qbias)
    if not (0.0 < qscale < float("inf")) or not (-float("inf") < qbias < float("inf")):
        raise ValueError("wavenet_speech_amd.%s: need a finite qscale > 0 and a finite qbias, got %r and %r" % (what, qscale, qbias))
    x, (B, C, T), (sb, sc, st), in_len = _prep(x, layout, input_lengths, what)
    if not 0 <= int(blank) < C:
        raise ValueError("wavenet_speech_amd.%s: blank must be in [0, %d), got %d" % (what, C, int(blank)))
    labels, frames = (_args.int_rows(r, what, name, B=B, shape="(%d, Lmax)" % B) for r, name in ((labels, "labels"), (frames, "frames")))
    if labels.device != x.device or frames.device != x.device or labels.shape != frames.shape:
        raise ValueError("wavenet_speech_amd.%s: labels and frames must have one shape, on the device of the input" % what)
    lmax = width = int(labels.shape[1])
    if lmax > T:
        raise ValueError("wavenet_speech_amd.%s: at most one label per frame: Lmax = %d, T = %d" % (what, lmax, T))
    dev = x.device
    lengths = _args.lengths(lengths, B, dev, what, "lengths")
    if lmax == 0:                                                    # the C ABI wants one column; no read may use it
        lmax, labels, frames = 1, torch.zeros(B, 1, dtype=torch.int32, device=dev), torch.zeros(B, 1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        error = torch.empty(B, lmax, dtype=torch.float32, device=dev)
        qual = torch.empty(B, lmax, dtype=torch.uint8, device=dev)
        dwell = torch.empty(B, lmax, dtype=torch.int32, device=dev)
        read_error = torch.empty(B, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_ctc_base_quality(_p(x), sb, sc, st, INPUT_KINDS[input], _p(in_len), _p(labels), labels.stride(0), _p(frames),
                                           frames.stride(0), _p(lengths), B, C, T, lmax, int(blank), QUALITY_STATS[stat], qscale,
                                           qbias, _p(error), _p(qual), _p(dwell), _p(read_error), _p(bad), _stream()),
                   "wn_ctc_base_quality")
        _args.note_bad(bad, lambda n, C=C, blank=int(blank): "wavenet_speech_amd.ctc_base_qualities: %d base(s) or read(s) with a "
                       "label outside [0, %d) or equal to the blank (%d), a frame outside its utterance or out of order, or a "
                       "length out of range" % (n, C, blank))
        mean_qscore = torch.log10(read_error) * (-10.0 * qscale) + qbias
    return BaseQualities(error[:, :width], qual[:, :width], dwell[:, :width], read_error, mean_qscore)


QUAL_ROWS = MAX_QUAL + 1            # rows of q_counts
DWELL_ROWS = 33                     # rows of dwell_counts: dwell 0..31, and 32 for everything above
OUT_NONE, OUT_MATCH, OUT_MISMATCH, OUT_INSERTION, OUT_END = 0, 1, 2, 3, 4


class QualityProfile(namedtuple("QualityProfile", "q_counts dwell_counts confusion read_counts outcome ref_index")):
    """q_counts [94, 3] int64: per claimed quality the (matches, mismatches, insertions) among the query bases; dwell_counts
    [33, 3] int64: the same per dwell (row 32 = 32 and above); confusion [C + 1, C + 1] int64: [true label][called label], index C
    = the gap (row C: insertions, column C: deletions); read_counts [B, 5] int32: matches, mismatches, insertions, deletions,
    end columns per read; outcome [B, M] uint8: 1 match, 2 mismatch, 3 insertion, 4 end, 0 past the read; ref_index [B, M] int32:
    the reference position of a matched or mismatched base, -1 otherwise.  q_counts / dwell_counts are None when no qual / dwell
    went in.  All on the device; the ratios below are torch ops on the device too."""
    __slots__ = ()

    @staticmethod
    def _rate(table):
        t = table.double()
        return (t[:, 1] + t[:, 2]) / t.sum(1)

    @property
    def error_by_quality(self):
        """[94] float64: (mismatches + insertions) / bases per claimed quality, NaN for an empty row"""
        return self._rate(self.q_counts)

    @property
    def error_by_dwell(self):
        """[33] float64: (mismatches + insertions) / bases per dwell, NaN for an empty row"""
        return self._rate(self.dwell_counts)

    @property
    def substitution_rates(self):
        """[C, C] float64: row t = the share of each called label among the aligned bases whose true label is t (NaN for a
        label never seen); the diagonal is the per-class accuracy of the aligned bases"""
        t = self.confusion[:-1, :-1].double()
        return t / t.sum(1, keepdim=True)

    @property
    def rates(self):
        """[B, 4] float64: mismatches, insertions, deletions per aligned column (end columns left out), and the identity
        matches / aligned columns; NaN for a read without aligned columns or a bad read"""
        c = self.read_counts.double()
        cols = c[:, :4].sum(1)
        cols = torch.where((cols > 0) & (c[:, 0] >= 0), cols, torch.full_like(cols, float("nan")))
        return torch.stack([c[:, 1], c[:, 2], c[:, 3], c[:, 0]], 1) / cols[:, None]


def _profile_rows(rows, B, M, dtype, what, name):
    """the optional qual / dwell rows of a query: at least its M columns (none: one unused column, as _pair_rows)"""
    if rows is None:
        return None
    return _args.int_rows(rows, what, name, B=B, shape="(%d, >= %d)" % (B, M), min_width=M, dtypes=(dtype,), pad_empty=True)


def _alignment_ops(alignment, what):
    """(ops, ops_len) of a PairwiseAlignment with ops, GPU tensors: the first step of every walker of an op row"""
    if not isinstance(alignment, PairwiseAlignment) or alignment.ops is None or alignment.ops_len is None:
        raise ValueError("wavenet_speech_amd.%s: alignment must be a PairwiseAlignment with ops (return_ops=True)" % what)
    return _args.gpu_tensor(alignment.ops, what, "alignment.ops"), _args.gpu_tensor(alignment.ops_len, what, "alignment.ops_len")


def _op_rows(ops, ops_len, B, dev, what, on=None, cap=MAX_OPS, pad_empty=True):
    """the second step, with B and the device known -> (ops, ops_len, max_ops) as the C ABI takes them.  on: the noun the message
    names the device by (None: the caller has compared the devices); cap: the most columns (None: none); pad_empty: rows without
    columns become one unused column"""
    if ops.device != dev or ops_len.device != dev or ops.dtype != torch.uint8 or ops.dim() != 2 or ops.shape[0] != B or \
            ops_len.dtype != torch.int32 or ops_len.shape != (B,):
        raise ValueError("wavenet_speech_amd.%s: alignment.ops must be uint8 of shape (%d, n) and ops_len int32 of shape (%d,)%s"
                         % (what, B, B, ", on the device of the %s" % on if on else ""))
    max_ops = int(ops.shape[1])
    if cap is not None and max_ops > cap:
        raise ValueError("wavenet_speech_amd.%s: at most %d op columns per read, got %d" % (what, cap, max_ops))
    if pad_empty and max_ops < 1:                                    # no columns: one unused column
        ops, max_ops = torch.zeros(B, 1, dtype=torch.uint8, device=dev), 1
    if ops.shape[1] > 1 and ops.stride(1) != 1 or ops.stride(0) < 0:
        ops = ops.contiguous()
    return ops, ops_len.contiguous(), max_ops


def quality_profile(alignment, ref, ref_lengths, query, query_lengths, qual=None, dwell=None, classes=5, count_ends=False,
                    into=None):
    """Walks each alignment of `pairwise_align(ref, ref_lengths, query, query_lengths)` and tabulates, for every query base,
    whether it was right against the quality and the dwell claimed for it: the input of
    fit_quality_calibration, and the error profile of a basecaller -- confusion matrix, insertions and deletions, error by dwell.
    alignment: a PairwiseAlignment with ops; ref / query and their lengths: what it was made from; qual [B, >= M] uint8 and dwell
    [B, >= M] int32: BaseQualities.qual (made with qscale=1, qbias=0) and .dwell of the query, either may be left out; classes:
    labels lie in [0, classes).
    End columns -- the unaligned head and tail that an alignment with end_gaps_free=True leaves before the first and after the last
    match-or-mismatch column -- are no basecall errors and enter no table unless count_ends=True.  Deletions carry no quality:
    they enter the confusion matrix and the per-read counts, not the quality or dwell tables.
    into: an earlier QualityProfile whose three tables are accumulated in place (and returned); its per-read fields are replaced.
    Returns QualityProfile.  A pair whose ops do not fit its labels (a poisoned pair of pairwise_align, a label outside [0, classes),
    a qual above 93, a negative dwell, ...) has outcome 0, ref_index -1, read_counts -1, adds nothing to the tables and is
    reported through check_device_flags()."""
    what = "quality_profile"
    ops, ops_len = _alignment_ops(alignment, what)
    width = int(query.shape[1]) if isinstance(query, torch.Tensor) and query.dim() == 2 else 0
    ref, ref_lengths = _pair_rows(ref, ref_lengths, what, "ref")
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, N, M = int(ref.shape[0]), int(ref.shape[1]), int(query.shape[1])
    dev = ref.device
    C = int(classes)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError("wavenet_speech_amd.%s: classes must be in [1, %d], got %d" % (what, MAX_CLASSES, C))
    if B < 1 or query.shape[0] != B or query.device != dev or ops.device != dev or ops_len.device != dev:
        raise ValueError("wavenet_speech_amd.%s: ref, query and the alignment must hold the same rows (at least one) on one device" % what)
    if N > MAX_PAIR_REF or M > MAX_PAIR_QUERY:
        raise ValueError("wavenet_speech_amd.%s: at most %d reference and %d query labels per pair, got %d and %d"
                         % (what, MAX_PAIR_REF, MAX_PAIR_QUERY, N, M))
    ops, ops_len, max_ops = _op_rows(ops, ops_len, B, dev, what, cap=None)
    max_ops = min(max_ops, N + M)
    qual = _profile_rows(qual, B, width, torch.uint8, what, "qual")
    dwell = _profile_rows(dwell, B, width, torch.int32, what, "dwell")
    if (qual is not None and qual.device != dev) or (dwell is not None and dwell.device != dev):
        raise ValueError("wavenet_speech_amd.%s: qual and dwell must be on the device of the labels" % what)
    if into is not None and not isinstance(into, QualityProfile):
        raise ValueError("wavenet_speech_amd.%s: into must be a QualityProfile, got %s" % (what, type(into).__name__))
    if into is not None and ((into.q_counts is None) != (qual is None) or (into.dwell_counts is None) != (dwell is None)):
        raise ValueError("wavenet_speech_amd.%s: into carries a table for which no qual / dwell is given, or the reverse" % what)
    lib = _lib.load()
    with torch.cuda.device(dev):
        q_counts = _args.into_table(into, "q_counts", (QUAL_ROWS, 3), dev, what) if qual is not None else None
        dwell_counts = _args.into_table(into, "dwell_counts", (DWELL_ROWS, 3), dev, what) if dwell is not None else None
        confusion = _args.into_table(into, "confusion", (C + 1, C + 1), dev, what)
        read_counts = torch.empty(B, 5, dtype=torch.int32, device=dev)
        outcome = torch.empty(B, M, dtype=torch.uint8, device=dev)
        ref_index = torch.empty(B, M, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_quality_profile(_p(ops), ops.stride(0), _p(ops_len), _p(ref), ref.stride(0), _p(ref_lengths), _p(query),
                                          query.stride(0), _p(query_lengths), _p(qual), qual.stride(0) if qual is not None else 0,
                                          _p(dwell), dwell.stride(0) if dwell is not None else 0, B, N, M, max_ops, C,
                                          int(bool(count_ends)), _p(q_counts), _p(dwell_counts), _p(confusion), _p(read_counts),
                                          _p(outcome), _p(ref_index), _p(bad), _stream()), "wn_quality_profile")
        _args.note_bad(bad, lambda n, C=C: "wavenet_speech_amd.quality_profile: %d pair(s) whose ops do not fit their labels: a "
                       "length out of range, an op outside 1..4, labels consumed or compared wrongly, a label outside [0, %d), a "
                       "qual above %d or a negative dwell" % (n, C, MAX_QUAL))
    return QualityProfile(q_counts, dwell_counts, confusion, read_counts, outcome[:, :width], ref_index[:, :width])


QualityCalibration = namedtuple("QualityCalibration", "qscale qbias bins_used bases_used q_empirical")
QualityCalibration.__doc__ = """qscale, qbias: Python floats, the slope and intercept that go into ctc_base_qualities /
Basecaller.qualities; bins_used: how many quality values carried at least min_count bases; bases_used: the bases in them;
q_empirical [94] float64 on the device of the table: the empirical Phred quality of each used bin, NaN elsewhere."""


def fit_quality_calibration(q_counts, min_count=100):
    """A straight line through the binned empirical error: for every claimed quality q with at least
    min_count bases, p_q = (mismatches + insertions + 0.5) / (bases + 1) and Qe_q = -10 log10 p_q; qscale and qbias are the least
    squares line Qe = qscale q + qbias over the used bins, weighted by their bases.  q_counts: QualityProfile.q_counts ([94, 3]
    int64), made from qualities with qscale=1, qbias=0.  float64 torch ops on the table's device; one read-back at the end.
    Raises ValueError for fewer than two used bins or a slope that is not finite and positive.  Returns QualityCalibration."""
    what = "fit_quality_calibration"
    if not isinstance(q_counts, torch.Tensor) or tuple(q_counts.shape) != (QUAL_ROWS, 3) or q_counts.is_floating_point():
        raise ValueError("wavenet_speech_amd.%s: q_counts must be an integer tensor of shape (%d, 3)" % (what, QUAL_ROWS))
    if int(min_count) < 1:
        raise ValueError("wavenet_speech_amd.%s: min_count must be at least 1, got %r" % (what, min_count))
    t = q_counts.double()
    n = t.sum(1)
    used = n >= float(int(min_count))
    w = torch.where(used, n, torch.zeros_like(n))
    qe = -10.0 * torch.log10((t[:, 1] + t[:, 2] + 0.5) / (n + 1.0))
    q = torch.arange(QUAL_ROWS, dtype=torch.float64, device=t.device)
    total = w.sum()
    q_mean, qe_mean = (w * q).sum() / total, (w * qe).sum() / total
    slope = (w * (q - q_mean) * (qe - qe_mean)).sum() / (w * (q - q_mean) ** 2).sum()
    bias = qe_mean - slope * q_mean
    slope, bias, bins, bases = torch.stack([slope, bias, used.sum().double(), total]).tolist()       # the one read-back
    if bins < 2:
        raise ValueError("wavenet_speech_amd.%s: %d quality value(s) with at least %d bases; a line needs two" % (what, int(bins), int(min_count)))
    if not (0.0 < slope < float("inf")) or not (-float("inf") < bias < float("inf")):
        raise ValueError("wavenet_speech_amd.%s: the fitted line (slope %r, intercept %r) is no calibration: the error does not fall "
                         "as the claimed quality rises" % (what, slope, bias))
    return QualityCalibration(slope, bias, int(bins), int(bases), torch.where(used, qe, torch.full_like(qe, float("nan"))))


def fastq_records(names, labels, lengths, qual, alphabet=DEFAULT_ALPHABET):
    """host helper: one FASTQ record "@name\nSEQ\n+\nQUAL\n" per read from label rows [N, L], their lengths [N] and the qual
    rows [N, L] of ctc_base_qualities (device or host; each is copied once).  SEQ is labels_to_strings' text, QUAL the
    characters chr(qual + 33); an empty read has empty SEQ and QUAL lines."""
    names = [str(n) for n in names]
    seqs = labels_to_strings(labels, lengths, alphabet)
    rows = torch.as_tensor(labels).cpu().tolist()
    quals = torch.as_tensor(qual).cpu().tolist()
    ns = [int(n) for n in torch.as_tensor(lengths).cpu().reshape(-1).tolist()]
    if not (len(names) == len(rows) == len(quals) == len(ns)):
        raise ValueError("fastq_records: %d names, %d label rows, %d qual rows, %d lengths" % (len(names), len(rows), len(quals), len(ns)))
    out = []
    for name, seq, row, q, n in zip(names, seqs, rows, quals, ns):
        if any(not 0 <= int(v) <= MAX_QUAL for v in q[:n]):
            raise ValueError("fastq_records: a quality outside [0, %d] in read %r" % (MAX_QUAL, name))
        text = "".join(chr(int(v) + 33) for v, lab in zip(q[:n], row[:n]) if int(lab) != 0)   # a blank prints nothing in SEQ either
        out.append("@%s\n%s\n+\n%s\n" % (name, seq, text))
    return out


def labels_to_strings(labels, lengths=None, alphabet=DEFAULT_ALPHABET):
    """host helper: label rows [N, T] (device or host) with their lengths [N] -> list of N strings; alphabet[i] is the
    character of label i, and label 0 (the blank) maps to the empty string, as the reference's lookup does (Decoder.py:26)"""
    rows = torch.as_tensor(labels).cpu().tolist()
    if lengths is None:
        ns = [len(r) for r in rows]
    else:
        ns = [int(n) for n in torch.as_tensor(lengths).cpu().reshape(-1).tolist()]
    if len(ns) != len(rows):
        raise ValueError("labels_to_strings: %d rows but %d lengths" % (len(rows), len(ns)))
    table = [""] + list(alphabet[1:])
    return ["".join(table[int(v)] for v in r[:n]) for r, n in zip(rows, ns)]


class CTCBeamDecoder(object):
    """The calling shape of ctcdecode's CTCBeamDecoder as the reference notebook uses it,
        decoder = CTCBeamDecoder(alphabet, beam_width=7, blank_id=0)
        beam_results, beam_scores, timesteps, out_lens = decoder.decode(probs)      # probs (B, T, C)
    on ctc_beam_decode: results stay on the device.  No language model (model_path, alpha, beta are not supported).
    beam_scores here are natural log probabilities, higher is better; ctcdecode's own score convention is not claimed."""

    def __init__(self, labels, beam_width=100, blank_id=0, log_probs_input=False):
        self.labels = list(labels)
        if len(self.labels) > MAX_CLASSES:
            raise ValueError("CTCBeamDecoder: at most %d labels, got %d" % (MAX_CLASSES, len(self.labels)))
        if not 1 <= int(beam_width) <= MAX_BEAM_WIDTH:
            raise ValueError("CTCBeamDecoder: beam_width must be in [1, %d], got %d" % (MAX_BEAM_WIDTH, beam_width))
        self.beam_width = int(beam_width)
        self.blank_id = int(blank_id)
        self.log_probs_input = bool(log_probs_input)

    def decode(self, probs, seq_lens=None):
        """probs: (B, T, C) probabilities (log-probabilities with log_probs_input=True).
        Returns (beam_results [B, W, T], beam_scores [B, W], timesteps [B, W, T], out_lens [B, W])."""
        labels, lengths, scores, frames = ctc_beam_decode(probs, self.beam_width, blank=self.blank_id, input_lengths=seq_lens,
                                                          input="log_probs" if self.log_probs_input else "probs", layout="BTC")
        return labels, scores, frames, lengths
