"""
Indel left-alignment on the device (csrc/wn_leftalign.hip through wn_gap_left_align): the step between
pairwise_align and pileup that bcftools norm and GATK LeftAlignIndels run.  pairwise_align places a gap inside a repeat by its tie
rule in READ orientation, so forward and reverse reads put it at opposite ends of the repeat and split its support; left_align
moves every gap run of every row as far toward the start of the FORWARD strand as the sequences allow.

    ref, ref_lengths = m.labels(flank=8)
    aln = pairwise_align(ref, ref_lengths, labels, lengths)
    aln = left_align(aln, ref, ref_lengths, labels, lengths, m.strand).alignment
    pile = pileup(aln, *m.window(flank=8), m.strand, labels, lengths, index.R)

Labels are only compared for equality, so results equal the host reference of tests/leftalign_ref.py exactly and two runs are
bitwise identical.  One launch, no host synchronisation, graph-capturable.  There is no CPU fallback: CPU tensors raise.
"""
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import MAX_OPS, MAX_PAIR_QUERY, MAX_PAIR_REF, _alignment_ops, _op_rows, _pair_rows
from .readmap import _int_in

MAX_PASSES = 64

LeftAligned = namedtuple("LeftAligned", "alignment passes settled")
LeftAligned.__doc__ = """alignment: a PairwiseAlignment with the new ops [B, n] uint8, and the input's ops_len, matches, mismatches,
gaps and length (the multiset of ops is kept) and the input's score AS IT WAS: two runs that come to lie side by side merge, which
can only raise the true score; passes [B] int32: the passes that moved a run (0: the row was normalised already); settled [B] int8:
1 a fixed point was reached, 0 max_passes ran and each moved something (the row is that many passes along and still a valid
alignment), -1 a bad pair.  All on the device."""


def left_align(alignment, ref, ref_lengths, query, query_lengths, strand, max_passes=8):
    """Moves every gap run of every op row as far toward the start of the forward strand as the sequences allow (DESIGN.md section
    7s), one launch.
    alignment: a PairwiseAlignment with ops, exactly as pairwise_align(ref, ref_lengths, query, query_lengths) returns it; ref [B, N]
    (N <= 65535) and query [B, M] (M <= 8192) int32 or int64 GPU rows with their [B] lengths: what it was made from, the window in
    READ orientation (mapping.labels(flank)); strand [B]: mapping.strand -- on strand 1 the row is walked back to front, as pileup
    walks it; max_passes in [1, 64].
    In walk orientation a run of l equal gap ops at column c, strictly between the first and the last aligned column, moves left by
    the largest s such that it passes only aligned columns, stays behind the previous gap column (or the first aligned column) and
    seq[x - t] == seq[x - t + l] for t = 1..s, where seq is the reference for a deletion and the read for an insertion and x the
    run's index in it.  Passes repeat until one moves nothing; a run that lands beside another of its kind is one run from then on.
    Returns LeftAligned.  A read with strand < 0 or ref_lengths == 0 is copied unchanged (passes 0, settled 1).  A pair whose ops do
    not fit (an op outside 1..4, a length outside its row, labels not consumed exactly, strand > 1; a poisoned pair of
    pairwise_align) is copied unchanged with settled -1 and reported through check_device_flags()."""
    what = "left_align"
    max_passes = _int_in(what, "max_passes", max_passes, 1, MAX_PASSES)
    ops, ops_len = _alignment_ops(alignment, what)
    ref, ref_lengths = _pair_rows(ref, ref_lengths, what, "ref")
    query, query_lengths = _pair_rows(query, query_lengths, what, "query")
    B, N, M = int(ref.shape[0]), int(ref.shape[1]), int(query.shape[1])
    dev = ref.device
    if query.shape[0] != B or query.device != dev:
        raise ValueError("wavenet_speech_amd.%s: ref and query must hold the same number of rows on one device" % what)
    if B < 1 or B > 65535 or N > MAX_PAIR_REF or M > MAX_PAIR_QUERY:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 pairs of at most %d reference and %d query labels, got %d of %d and %d"
                         % (what, MAX_PAIR_REF, MAX_PAIR_QUERY, B, N, M))
    ops, ops_len, max_ops = _op_rows(ops, ops_len, B, dev, what, on="labels", pad_empty=False)
    strand = _args.lengths(strand, B, dev, what, "strand")
    passes = torch.empty(B, dtype=torch.int32, device=dev)
    settled = torch.empty(B, dtype=torch.int8, device=dev)
    if max_ops < 1:                                                  # no columns: nothing to move
        passes.zero_()
        settled.fill_(1)
        return LeftAligned(alignment._replace(ops=ops.clone()), passes, settled)
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty(B, max_ops, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_gap_left_align(_p(ops), ops.stride(0), _p(ops_len), _p(ref), ref.stride(0), _p(ref_lengths), _p(query),
                                         query.stride(0), _p(query_lengths), _p(strand), B, N, M, max_ops, max_passes, _p(out),
                                         out.stride(0), _p(passes), _p(settled), None, 0, _p(bad), _stream()), "wn_gap_left_align")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.left_align: %d pair(s) whose ops do not fit: an op outside 1..4, a length out "
                       "of range, labels not consumed exactly or a strand above 1" % n)
    return LeftAligned(alignment._replace(ops=out, ops_len=ops_len), passes, settled)
