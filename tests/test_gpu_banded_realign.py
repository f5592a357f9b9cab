"""GPU: realign(first=, band=) (wavenet_speech_amd/realign.py through banded_align) on the planted phased runs of
tests/realign_cases.py, on the planted windows.  The device result equals the host reference -- tests/banded_align_ref.py inside the
stripes [lo1 - n4 - band, hi1 + n3 + band], composed by tests/realign_ref.py -- its scores are at most the full run's, the reads
that differ from the full run are the constant of tests/banded_align_cases.py (none at band 16), and the figures downstream are the
host run's.  The banded reference costs 45 ms a row on the host, so it is run for every fifth read on both haplotypes; all 320 rows
are held to the device's full pairwise_align rows, which tests/test_gpu_realign.py holds to the same reference chain."""
import types

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import banded_align_cases as BC
from tests import banded_align_ref as B
from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import pairwise_align_ref as A
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import realign_cases as RC
from tests import realign_ref as RR
from tests.gpu_calls import capture
from tests.gpu_util import assert_equal_arrays, dev, i32
from tests.gpu_util import no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("noisy", [False, True])
def test_banded_realign_on_the_planted_phased_runs(noisy):
    run = PC.planted(noisy)
    labels, lengths, qual = dev(run["labels"]), dev(run["lengths"]), dev(run["qual"])
    index = W.read_index(i32(run["ref"]), k=11, w=5)
    lo, ref_len, strand = i32([v[0] for v in run["window"]]), i32([v[1] for v in run["window"]]), i32(run["strand"])
    ref_rows = dev(C.rows(RC.windows_of(run)[2])[0])
    w = W.genotype_weights(K.SCALE)

    def tables(alignment):
        aln = W.left_align(alignment, ref_rows, ref_len, labels, lengths, strand).alignment
        reads = (aln, lo, ref_len, strand, labels, lengths)
        pile = W.pileup(*reads, index.R, qual=qual, min_qual=PC.MIN_QUAL)
        ev = W.pileup_evidence(*reads, index.R, w, qual=qual, min_qual=PC.MIN_QUAL)
        return reads, W.call_genotypes(pile, ev, index, w)

    first = W.pairwise_align(ref_rows, ref_len, labels, lengths)
    reads, calls = tables(first)
    sites = W.phase_sites(calls)
    phasing = W.phase_chain(W.phase_links(*reads, sites, qual=qual, min_qual=PC.MIN_QUAL, reach=PC.REACH), sites)
    tags = W.haplotag(*reads, sites, phasing, qual=qual, min_qual=PC.MIN_QUAL)
    hcalls = W.haplotype_calls(calls, sites, phasing)
    full = W.realign(ref_rows, ref_len, labels, lengths, lo, strand, hcalls, index)
    got = W.realign(ref_rows, ref_len, labels, lengths, lo, strand, hcalls, index, first=first, band=BC.REALIGN_BAND)
    graph, captured = capture(lambda: W.realign(ref_rows, ref_len, labels, lengths, lo, strand, hcalls, index, first=first, band=BC.REALIGN_BAND))
    graph.replay()
    W.check_device_flags()
    flat = lambda r: [r.pick, r.hp, r.delta, r.scores] + list(r.alignment)      # noqa: E731
    assert all(torch.equal(u, v) for u, v in zip(flat(captured), flat(got))), "the captured graph replays another result"
    # the stripes on the host, from the device's first rows and windows; the rows realign made inside them
    cap = int(ref_rows.shape[1]) * (1 + int(hcalls.ins_bases.shape[2]))
    windows = W.haplotype_windows(hcalls, index, lo, ref_len, strand, max_hap_ops=cap)
    f_ops, f_len = first.ops.cpu().numpy(), first.ops_len.cpu().tolist()
    h_ops, h_len = windows.ops.cpu().numpy(), windows.ops_len.cpu().numpy()
    n_reads = len(f_len)
    stripes = []
    for h in range(2):
        for b in range(n_reads):
            l1, h1 = B.band_from_ops(f_ops[b][:f_len[b]])
            row = h_ops[h][b][:h_len[h][b]]
            stripes.append((l1 - int((row == 4).sum()) - BC.REALIGN_BAND, h1 + int((row == 3).sum()) + BC.REALIGN_BAND))
    widest = max(s[1] - s[0] + 1 for s in stripes)
    print("widest stripe %d diagonals" % widest)
    assert widest == BC.REALIGN_WIDEST
    rows = []
    for h in range(2):
        part = stripes[h * n_reads:(h + 1) * n_reads]
        out = W.banded_align(windows.labels[h], windows.lengths[h], labels, lengths, i32([s[0] for s in part]), i32([s[1] for s in part]), widest)
        assert out.status.eq(1).all()
        rows.append((out.alignment.ops.cpu().numpy(), out.alignment.ops_len.cpu().tolist()))
        assert torch.equal(out.alignment.score, got.scores[:, h]), "realign's stripes are not [lo1 - n4 - band, hi1 + n3 + band]"
    # the banded reference itself, for every fifth read on both haplotypes
    hap_labels, hap_len = windows.labels.cpu().numpy(), windows.lengths.cpu().numpy()
    for h in range(2):
        for b in range(0, n_reads, 5):
            want = B.align(hap_labels[h][b][:hap_len[h][b]], run["reads"][b], *stripes[h * n_reads + b], *A.EMBOSS, True)
            assert_equal_arrays(rows[h][0][b][:rows[h][1][b]], want.ops, "read %d against haplotype %d" % (b, h))
    # composed by the reference: windows, scores, pick, hp, delta and the lifted rows
    host_sites = H.Sites(sites.pos.cpu().tolist(), [tuple(a) for a in sites.alleles.cpu().tolist()], sites.site_of.cpu().tolist())
    hc = RR.haplotype_calls_ref(G.Calls(*[None if t is None else t.cpu().numpy() for t in calls]), host_sites, H.Chain(*[t.cpu().tolist() for t in phasing]))
    lo_h, n_h = lo.cpu().tolist(), ref_len.cpu().tolist()
    refs = [row[:n].tolist() for row, n in zip(ref_rows.cpu().numpy(), n_h)]
    want = RR.realign_ref(refs, n_h, run["reads"], lo_h, run["strand"], hc, run["ref"], align=lambda h, b, hap, read: rows[h][0][b][:rows[h][1][b]])
    assert got.pick.cpu().tolist() == want.pick and got.hp.cpu().tolist() == want.hp
    assert (got.delta.cpu().numpy() * 2).astype(np.int64).tolist() == want.delta and (got.scores.cpu().numpy() * 2).astype(np.int64).tolist() == want.scores
    al, width = got.alignment, min(int(got.alignment.ops.shape[1]), want.lifted.ops.shape[1])
    assert_equal_arrays(al.ops.cpu().numpy()[:, :width], want.lifted.ops[:, :width], "lifted ops")
    assert_equal_arrays(al.ops_len.cpu().numpy(), np.asarray(want.lifted.ops_len, dtype=np.int32), "lifted ops_len")
    assert_equal_arrays((al.score.cpu().numpy().astype(np.float64) * 2).astype(np.int64), np.asarray(want.lifted.score, dtype=np.int64), "lifted score")
    assert want.lifted.bad == 0 and want.windows.bad == 0
    # beside the full run: never a greater score, and the constants of the host run
    assert bool((got.scores <= full.scores).all())
    assert int((got.scores < full.scores).sum()) == BC.REALIGN_LOWER[noisy]
    differ = (got.pick != full.pick) | (got.hp != full.hp) | (al.ops_len != full.alignment.ops_len) | (al.ops != full.alignment.ops).any(1)
    print("reads that differ from the full run: %d" % int(differ.sum()))
    assert int(differ.sum()) == BC.REALIGN_DIFFER[noisy]
    # downstream: the conditions of tests/realign_cases.py on the device's tables, NEITHER_AFTER and the unchanged calls among them
    reads2, calls2 = tables(al)
    before = RC.recall(run, reads[0].ops.cpu().numpy(), reads[0].ops_len.cpu().numpy(), lo_h, n_h, host_sites)
    after = RC.recall(run, reads2[0].ops.cpu().numpy(), reads2[0].ops_len.cpu().numpy(), lo_h, n_h, host_sites)
    for name in ("alleles", "flags", "ins_copies", "ins_len"):
        assert_equal_arrays(getattr(calls2, name).cpu().numpy(), getattr(after["calls"], name), "calls after, " + name)
    own_scores = [A.rescore(row[:k], *A.EMBOSS, True) for row, k in zip(reads[0].ops.cpu().numpy(), reads[0].ops_len.cpu().tolist())]
    RC.check_conditions(run, dict(sites=host_sites, tags=types.SimpleNamespace(hp=tags.hp.cpu().tolist())),
                        types.SimpleNamespace(hp=want.hp, delta=want.delta, lifted=want.lifted), before, after, noisy, own_scores=own_scores,
                        windows=(lo_h, n_h), exact=True)
    W.check_device_flags()


def test_first_and_band_come_together_and_the_default_path_is_unchanged():
    run = PC.planted(False)
    with pytest.raises(ValueError, match="first and band come together"):
        W.realign(dev(C.rows(RC.windows_of(run)[2])[0]), i32([v[1] for v in run["window"]]), dev(run["labels"]), dev(run["lengths"]),
                  i32([v[0] for v in run["window"]]), i32(run["strand"]), None, None, band=16)
