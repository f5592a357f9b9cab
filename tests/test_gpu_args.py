"""GPU: the shared argument preparers of wavenet_speech_amd/_args.py under signal_align and kmer_events.  The signal as a [B, 1, L]
view into a wider buffer (row stride 256, not L), int64 labels and Python lists of lengths must give, bit for bit, what contiguous
[B, L] samples, int32 labels and device lengths give: a copy where a view was meant (or the reverse) in the signal, label or
lengths preparation shows here."""
import pytest
import torch

import wavenet_speech_amd as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, L, LABELS, K, BAND = 3, 200, 40, 3, 64


def _reads():
    """three reads of 38 3-mers, five samples per k-mer at integer levels with small integer noise: exact in float32 and int16"""
    g = torch.Generator().manual_seed(11)
    means = torch.arange(4 ** K, dtype=torch.float64) * 7.0 + 300.0
    model = W.signal_model(means, torch.full((4 ** K,), 4.0, dtype=torch.float64))
    labels = torch.randint(1, 5, (B, LABELS), generator=g)
    label_lengths = [40, 38, 30]
    signal_lengths = [200, 190, 170]
    kmers = ((labels - 1).unfold(1, K, 1) * torch.tensor([16, 4, 1])).sum(-1)                   # [B, 38]
    wide = torch.zeros(B, 1, 256, dtype=torch.int16)
    level = means[kmers].repeat_interleave(5, dim=1)[:, :L - 10]                                # 190 samples
    wide[:, 0, 5:5 + level.shape[1]] = (level + torch.randint(-3, 4, level.shape, generator=g)).to(torch.int16)
    wide[:, 0, 5 + level.shape[1]:205] = 300
    return wide, labels, label_lengths, signal_lengths, model


def _outputs(signal, signal_lengths, labels, label_lengths, model):
    al = W.signal_align(signal, signal_lengths, labels, label_lengths, model, first=0, band=BAND, want_states=True)
    ev = W.kmer_events(signal, signal_lengths, labels, label_lengths, starts=al.starts, k=K, first=0)
    return list(al) + list(ev)


def test_views_int64_labels_and_list_lengths_match_dense_copies():
    wide16, labels, label_lengths, signal_lengths, model = _reads()
    for dtype in (torch.float32, torch.int16):
        wide = wide16.to(device=DEV, dtype=dtype)
        view = wide[:, :, 5:205]                                                                # [3, 1, 200], row stride 256
        assert view.stride(0) == 256 and not view.is_contiguous() and labels.dtype == torch.int64
        got = _outputs(view, signal_lengths, labels.to(DEV), label_lengths, model)
        dense = view[:, 0].contiguous()
        i32 = dict(dtype=torch.int32, device=DEV)
        want = _outputs(dense, torch.tensor(signal_lengths, **i32), labels.to(**i32).contiguous(), torch.tensor(label_lengths, **i32), model)
        assert len(got) == len(want) == 12
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g, w)
        W.check_device_flags()
        starts, score, band_hits = got[0], got[1], got[2]
        assert bool((score < 2 ** 62).all()) and bool((score > -2 ** 62).all())                # every read was aligned, none was bad
        assert starts[:, 0].tolist() == [0, 0, 0] and int(got[9][:, 0].min()) > 0               # and events were used in every read
