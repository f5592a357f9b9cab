"""
Surface of the reference's modules/sequence_decoders.py that its Decoder(..., 'argmax') path uses, so that code written
against it gets identical strings here:

    argmax_decode(logits)       logits (batch, sequence, classes) -> per-frame argmax labels (batch, sequence); NO collapse of
                                repeats and NO blank removal, exactly as the reference (which leaves both to the reader)
    labels2strings(labels)      rows of labels -> strings through the reference's lookup {0: '', 1: 'A', 2: 'G', 3: 'C', 4: 'T'}

For an actual CTC read use wavenet_speech_amd.decoding (greedy with collapse, or prefix beam search, on the device).
The reference's OpenNMT-style BeamSearchDecoder is deliberately not mirrored.
"""
import torch

DEFAULT_LOOKUP = {0: "", 1: "A", 2: "G", 3: "C", 4: "T"}


def argmax_decode(logits):
    """(batch, sequence, classes) -> int64 (batch, sequence): the class of largest value per frame (ties to the lowest)"""
    return torch.argmax(logits, dim=2)


def labels2strings(labels, lookup=None):
    """(batch, sequence) integer labels -> list of strings, one character (or '') per label through `lookup`"""
    table = DEFAULT_LOOKUP if lookup is None else lookup
    rows = torch.as_tensor(labels).cpu().tolist()
    return ["".join(table[int(v)] for v in row) for row in rows]
