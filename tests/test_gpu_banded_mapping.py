"""GPU: base-level extension of mapped reads inside the chain's stripe (ReadMapping.band into banded_align) on the
planted mapping run of tests/readmap_cases.py: the full alignment's path of every read stays within 9 diagonals of the stripe of the
chain's two end points, so under a margin of 32 the banded result is pairwise_align's, op for op, for all 64 reads."""
import pytest
import torch

from tests import readmap_cases as C
from tests.gpu_labels import package as _W
from tests.gpu_util import dev as _dev
from tests.gpu_util import no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu


def test_the_planted_reads_inside_their_chain_stripes():
    W = _W()
    p = C.planted()
    labels, lengths = _dev(p["labels"]), _dev(p["lengths"])
    m = W.map_reads(labels, lengths, W.read_index(C.planted_reference_bases(), device=labels.device))
    ref, ref_lengths = m.labels(20)
    full = W.pairwise_align(ref, ref_lengths, labels, lengths)
    lo, hi = m.band(flank=20, margin=32)
    assert lo.dtype == torch.int32 and lo.is_cuda and bool((hi - lo >= 64).all())
    width = int((hi - lo).max()) + 1
    print("widest stripe %d diagonals" % width)
    got = W.banded_align(ref, ref_lengths, labels, lengths, lo, hi, width)
    assert got.status.eq(1).all()
    for u, v, what in zip(got.alignment, full, full._fields):
        assert torch.equal(u, v), what                              # all 64 reads, op for op
    assert got.edge_hits.eq(0).all()
    plo, phi = W.band_from_ops(full)                                 # the path's own stripe lies strictly inside the chain's
    print("least distance of a path from its stripe's edges: %d and %d diagonals" % ((plo - lo).min().item(), (hi - phi).min().item()))
    assert bool((plo > lo).all()) and bool((phi < hi).all())
    trimmed, trimmed_lengths = W.trim_reads(labels, lengths, torch.stack([m.query_start, m.query_end], dim=1))
    tight, tight_lengths = m.labels()
    tlo, thi = m.band(margin=32)
    tw = int((thi - tlo).max()) + 1
    # the stripe is in whole-read coordinates: the trimmed read starts query_start columns later
    shift = m.query_start
    banded = W.banded_align(tight, tight_lengths, trimmed, trimmed_lengths, tlo - shift, thi - shift, tw)
    aln = W.pairwise_align(tight, tight_lengths, trimmed, trimmed_lengths)
    for u, v, what in zip(banded.alignment, aln, aln._fields):
        assert torch.equal(u, v), "trimmed " + what
    least = min(banded.alignment.identity.cpu().tolist())
    print("least identity %.4f" % least)
    assert round(least, 3) == 0.903                                  # what tests/test_gpu_readmap.py records for these stretches
    # clamped about its centre
    clo, chi = m.band(flank=20, margin=32, max_band=48)
    assert bool((chi - clo == 47).all()) and bool(((clo + chi) - (lo + hi)).abs().le(1).all())
    W.check_device_flags()
