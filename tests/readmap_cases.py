"""The inputs that tests/test_readmap_ref.py (CPU) and tests/test_gpu_readmap.py share, each built once with its reference result
(tests/readmap_ref.py): the planted run of the issue -- a seeded random 20 000-base reference with [3000, 3600) copied to
[15000, 15600), 64 reads of 400 to 1200 bases on alternating strands with 8 % errors split evenly among deletions, insertions and
substitutions -- and one read drawn wholly inside the repeat."""
import functools

import numpy as np

from tests import readmap_ref as R

PLANT_SEED = 1
PLANT_REF = 20000
PLANT_REPEAT = (3000, 3600, 15000)            # [from, to) copied to
PLANT_READS = 64
PLANT_ERRORS = 0.08
REPEAT_SEED = 11
REPEAT_ERRORS = 0.12


def random_bases(rng, n):
    return [int(v) for v in rng.integers(1, 5, size=n)]


def mutate(rng, seq, rate):
    """every base independently: deleted, followed by an inserted base, or substituted (by another base), each at rate / 3"""
    out = []
    for v in seq:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(v)
            out.append(int(rng.integers(1, 5)))
        elif u < rate:
            out.append((v - 1 + int(rng.integers(1, 4))) % 4 + 1)
        else:
            out.append(v)
    return out


def rows(seqs, width=None):
    """(labels [B, width] int32 zero-padded, lengths [B] int32)"""
    width = max(1, max(len(s) for s in seqs)) if width is None else width
    labels = np.zeros((len(seqs), width), dtype=np.int32)
    for b, s in enumerate(seqs):
        labels[b, :len(s)] = s
    return labels, np.array([len(s) for s in seqs], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def planted_reference_bases():
    rng = np.random.default_rng(PLANT_SEED)
    ref = random_bases(rng, PLANT_REF)
    a, b, to = PLANT_REPEAT
    ref[to:to + b - a] = ref[a:b]
    return ref


@functools.lru_cache(maxsize=None)
def planted():
    """dict: ref (list), reads (list of lists), truth [(strand, start, end)], labels, lengths"""
    rng = np.random.default_rng(PLANT_SEED + 1)
    ref = planted_reference_bases()
    reads, truth = [], []
    for b in range(PLANT_READS):
        n = int(rng.integers(400, 1201))
        start = int(rng.integers(0, PLANT_REF - n + 1))
        seq = mutate(rng, ref[start:start + n], PLANT_ERRORS)
        strand = b & 1
        reads.append(R.revcomp(seq) if strand else seq)
        truth.append((strand, start, start + n))
    labels, lengths = rows(reads)
    return dict(ref=ref, reads=reads, truth=truth, labels=labels, lengths=lengths)


@functools.lru_cache(maxsize=None)
def planted_index():
    return R.index_ref(planted_reference_bases(), R.DEFAULTS["k"], R.DEFAULTS["w"])


@functools.lru_cache(maxsize=None)
def planted_results():
    """the reference's result of every planted read at the defaults, want_pred included"""
    index = planted_index()
    return [R.map_read_ref(read, index) for read in planted()["reads"]]


@functools.lru_cache(maxsize=None)
def repeat_read():
    """(read, (strand, start, end)): 500 bases from inside the lower copy of the repeat, 12 % errors, forward strand"""
    rng = np.random.default_rng(REPEAT_SEED)
    ref = planted_reference_bases()
    a, b, _ = PLANT_REPEAT
    start = a + 40
    end = start + 500
    assert a <= start and end <= b
    return mutate(rng, ref[start:end], REPEAT_ERRORS), (0, start, end)


FIELDS = ("score", "strand", "ref_start", "ref_end", "query_start", "query_end", "n_anchors", "runner_up")


def result_rows(results):
    """[B, 8] int64 of the reference's result dicts, in the order of the kernel's result row"""
    return np.array([[r[f] for f in FIELDS] for r in results], dtype=np.int64)
