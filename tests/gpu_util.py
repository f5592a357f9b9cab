"""What the GPU tests share whatever the tool (tests/test_gpu_*.py): the device, host arrays onto it, the strided
view, tuple and bitwise equality, the fixture that clears a flag another test left, and the logits and the small basecaller that
several tools are fed with.  The drivers of one family of tools are in tests/gpu_calls.py, gpu_signal.py, gpu_labels.py and
gpu_stack.py.  Nothing here is rewritten by pytest, so every assert carries its message."""
import numpy as np
import pytest
import torch

DEV = torch.device("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def i32(v):
    return dev(np.asarray(v, dtype=np.int32))


def u8(v):
    return dev(np.asarray(v, dtype=np.uint8))


def i64(a):
    """a host array of Python integers as int64, exactly"""
    return np.array(a.tolist(), dtype=np.int64).reshape(a.shape)


def strided(a, channel):
    """the rows of `a` as a view into a wider device buffer (row stride L + 5, one element in); [B, 1, L] with channel"""
    B, L = a.shape
    wide = torch.zeros(B, L + 5, dtype=torch.from_numpy(a[:1, :1]).dtype, device=DEV)
    wide[:, 1:1 + L] = dev(a)
    view = wide[:, 1:1 + L]
    assert not view.is_contiguous() or B == 1, (B, L, view.stride())
    return view.unsqueeze(1) if channel else view


def same(a, b):
    """two result tuples hold equal tensors; None matches None"""
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    """bitwise equality of two result tuples (NaN payloads included)"""
    return all(torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


def first_difference(got, want):
    """'' where two host arrays are equal in shape and in every element, else the shapes or the first differing index with both values"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    at = np.argwhere(got != want)
    if not len(at):
        return ""
    i = tuple(int(v) for v in at[0])
    return "%d differ, first at %s: %s, expected %s" % (len(at), i, got[i], want[i])


def assert_equal_arrays(got, want, what):
    """exact equality of two host arrays, shape included; the message names `what` and the first difference"""
    diff = first_difference(got, want)
    assert not diff, "%s: %s" % (what, diff)


@pytest.fixture(autouse=True)
def no_stale_flags():
    """a test that failed between a call with bad rows and its check leaves their flag behind: it is not this test's.  A module
    imports this name to have it run before each of its tests"""
    import wavenet_speech_amd as W
    try:
        W.check_device_flags()
    except RuntimeError:
        pass


def random_logits(seed, B, C, T, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, T, generator=g) * scale


def peaked_logits(seed, B, C, T, margin=5.0):
    """'trained-looking' output: a random path of runs (the blank between runs) well above noisy other classes -> (logits, the
    run path [B][T])"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, C, T)) * 1.0
    path = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        t = 0
        while t < T:
            c = int(rng.integers(0, C))
            d = int(rng.integers(1, 6))
            x[b, c, t:t + d] += margin * rng.uniform(0.6, 1.0)
            path[b, t:t + d] = c
            t += d
    return torch.tensor(x, dtype=torch.float32), path


def basecall_model(softmax=False):
    """the 16-channel RawCTCNet of tests/test_gpu_basecall.py, seeded"""
    from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet
    torch.manual_seed(21)
    return RawCTCNet(16, 3, 5, [(16, 16, 2, d) for d in (1, 2, 4, 3)], 16, softmax=softmax, causal=False).to(DEV)
