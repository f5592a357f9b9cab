"""CPU: the C ABI of the signal mapping (csrc/wn_sigmap.hip): the exported symbols, the ctypes rows against the header argument by
argument, the size functions, and every host-side rejection on both sides of its limit and in its documented order (shape,
unsupported, NULL, workspace), with fake pointers: every call below returns before anything would be launched.  And what
map_reference / signal_map refuse before they reach the library, and the reverse-complement join."""
import ctypes

import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, check_row, header_names, header_text

NAME = "wn_signal_map"
ARGS = ["signal", "signal_kind", "signal_stride", "signal_lengths", "scale_shift", "prepared", "ref_len", "k", "batch", "max_signal",
        "frac_bits", "weight_shift", "max_cost", "strip_states", "score", "end", "start", "runner_up", "block_cost", "block_end", "end_cost",
        "workspace", "workspace_bytes", "bad", "stream"]
REQUIRED = ("signal", "signal_lengths", "prepared", "score", "end", "start", "runner_up", "block_cost", "block_end", "workspace")
REF_ARGS = ["ref", "ref_len", "model", "k", "prepared", "prepared_bytes", "bad", "stream"]


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in (NAME, NAME + "_workspace_bytes", NAME + "_reference", NAME + "_reference_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.wn_version() == 300                                   # additive entry points
    assert "#define WN_MAP_GRANULE 64" in header_text()


def test_signature_rows_match_the_header():
    for name, count in ((NAME, 25), (NAME + "_workspace_bytes", 5), (NAME + "_reference", 8), (NAME + "_reference_bytes", 2)):
        check_row(name, count=count, opaque=True)
    assert header_names(NAME) == ARGS and header_names(NAME + "_reference") == REF_ARGS


def test_size_functions(lib):
    size = lib.wn_signal_map_reference_bytes
    for args in ((0, 1), (-3, 1), (4, 5), (10, 0), (10, 7), (2 ** 26 + 1, 5)):
        assert size(*args) == 0, args
    for R, k in ((1, 1), (5, 5), (6, 5), (1000, 3), (48502 * 2 + 1, 5), (2 ** 26, 6)):
        M = R - k + 1
        need = 4 * (M + 3 * 4 ** k)                                  # one int32 per state and the model
        assert need <= size(R, k) < need + 32 and size(R, k) % 16 == 0, (R, k)
    ws = lib.wn_signal_map_workspace_bytes
    for args in ((0, 10, 100, 5, 0), (65536, 10, 100, 5, 0), (1, 0, 100, 5, 0), (1, 4097, 100, 5, 0), (1, 10, 4, 5, 0), (1, 10, 100, 0, 0),
                 (1, 10, 100, 7, 0), (1, 10, 2 ** 26 + 1, 5, 0), (1, 10, 100, 5, 32), (1, 10, 100, 5, 96), (1, 10, 100, 5, -64),
                 (1, 10, 100, 5, 2 ** 20 + 64)):
        assert ws(*args) == 0, args
    for B, L, R, k, strip in ((1, 1, 1, 1, 0), (3, 700, 4102, 3, 64), (65535, 4096, 100, 5, 2 ** 20), (4, 2048, 2 ** 26, 6, 0)):
        G = (R - k + 1 + 63) // 64
        assert 4 * B * G <= ws(B, L, R, k, strip) < 4 * B * G + 16 and ws(B, L, R, k, strip) % 16 == 0     # one origin per block
    assert ws(2, 100, 1000, 5, 64) == ws(2, 100, 1000, 5, 0) == ws(2, 4096, 1000, 5, 576)                  # the strip tunes, it sizes nothing


def _ref_call(lib, **kw):
    a = dict(ref=FAKE, ref_len=1000, model=FAKE, k=5, prepared=FAKE, prepared_bytes=0, bad=None, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib.wn_signal_map_reference(*[a[n] for n in REF_ARGS])


def test_reference_rejects_on_the_host_in_order(lib):
    assert _ref_call(lib) == WN_ERR_WORKSPACE                        # prepared_bytes 0: never launches
    for kw in (dict(ref_len=0), dict(ref_len=-1), dict(ref_len=4), dict(ref_len=4, k=7)):
        assert _ref_call(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    for kw in (dict(k=0), dict(k=-1), dict(k=7), dict(ref_len=2 ** 26 + 1)):
        assert _ref_call(lib, **kw) == WN_ERR_UNSUPPORTED, kw
    for kw in (dict(k=1), dict(k=6), dict(ref_len=5), dict(ref_len=2 ** 26), dict(ref_len=1, k=1)):
        assert _ref_call(lib, ref=None, **kw) == WN_ERR_NULL, kw
    for name in ("ref", "model", "prepared"):
        assert _ref_call(lib, **{name: None}) == WN_ERR_NULL, name
    need = lib.wn_signal_map_reference_bytes(1000, 5)
    assert _ref_call(lib, prepared_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _ref_call(lib, prepared=ctypes.c_void_p((1 << 20) + 8), prepared_bytes=need) == WN_ERR_WORKSPACE
    assert _ref_call(lib, ref_len=0, k=7, ref=None) == WN_ERR_BAD_SHAPE
    assert _ref_call(lib, k=7, ref=None) == WN_ERR_UNSUPPORTED
    assert _ref_call(lib, model=None, prepared_bytes=0) == WN_ERR_NULL


def _call(lib, **kw):
    a = dict(signal=FAKE, signal_kind=0, signal_stride=1000, signal_lengths=FAKE, scale_shift=FAKE, prepared=FAKE, ref_len=5000, k=5,
             batch=2, max_signal=1000, frac_bits=12, weight_shift=40, max_cost=2 ** 31 - 1, strip_states=0, score=FAKE, end=FAKE,
             start=FAKE, runner_up=FAKE, block_cost=FAKE, block_end=FAKE, end_cost=FAKE, workspace=FAKE, workspace_bytes=0, bad=None,
             stream=None)                                            # workspace_bytes 0: never launches
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib.wn_signal_map(*[a[n] for n in ARGS])


def test_rejects_on_the_host_in_order(lib):
    assert _call(lib) == WN_ERR_WORKSPACE                            # everything else about the default call is accepted
    for kw in (dict(batch=0), dict(batch=-2), dict(max_signal=0), dict(max_signal=-5), dict(ref_len=0), dict(ref_len=-1), dict(ref_len=4),
               dict(signal_stride=-1), dict(signal_kind=2), dict(signal_kind=-1)):
        assert _call(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    for kw in (dict(k=0), dict(k=7, ref_len=5000), dict(frac_bits=-1), dict(frac_bits=21), dict(weight_shift=15), dict(weight_shift=64),
               dict(max_cost=0), dict(max_cost=-1), dict(max_signal=4097), dict(ref_len=2 ** 26 + 1), dict(batch=65536),
               dict(strip_states=32), dict(strip_states=96), dict(strip_states=-64), dict(strip_states=2 ** 20 + 64), dict(strip_states=1)):
        assert _call(lib, **kw) == WN_ERR_UNSUPPORTED, kw
    # the accepted side of each limit goes on to the pointer checks
    for kw in (dict(k=1), dict(k=6), dict(frac_bits=0), dict(frac_bits=20), dict(weight_shift=16), dict(weight_shift=63), dict(max_cost=1),
               dict(max_cost=2 ** 31 - 1), dict(max_signal=4096), dict(max_signal=1), dict(ref_len=2 ** 26), dict(ref_len=5), dict(batch=65535),
               dict(batch=1), dict(strip_states=64), dict(strip_states=576), dict(strip_states=2 ** 20), dict(signal_kind=1),
               dict(signal_stride=0), dict(ref_len=1, k=1)):
        assert _call(lib, signal=None, **kw) == WN_ERR_NULL, kw
    # a grid of 2^31 workgroups or more: 2^20 strips of 64 states for each of 2048 reads; one strip fewer per read passes
    assert _call(lib, ref_len=2 ** 26, k=1, strip_states=64, batch=2048, signal=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, ref_len=2 ** 26 - 64, k=1, strip_states=64, batch=2048, signal=None) == WN_ERR_NULL
    assert _call(lib, ref_len=2 ** 26, k=1, strip_states=128, batch=2048, signal=None) == WN_ERR_NULL
    for name in REQUIRED:
        assert _call(lib, **{name: None}) == WN_ERR_NULL, name
    for name in ("scale_shift", "end_cost", "bad"):                  # optional
        assert _call(lib, **{name: None}) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and a signal off its element size
    need = lib.wn_signal_map_workspace_bytes(2, 1000, 5000, 5, 0)
    assert need == (2 * 4 * 79 + 15) // 16 * 16                      # 4996 states: 79 blocks
    assert _call(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _call(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert _call(lib, signal=ctypes.c_void_p((1 << 20) + 2), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert _call(lib, signal=ctypes.c_void_p((1 << 20) + 1), signal_kind=1, workspace_bytes=need) == WN_ERR_WORKSPACE
    assert _call(lib, batch=3, workspace_bytes=need) == WN_ERR_WORKSPACE             # the size follows the batch
    # the order: shape, then unsupported, then NULL, then workspace
    assert _call(lib, batch=0, k=7, signal=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, signal_kind=2, strip_states=96, prepared=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, ref_len=4, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, k=7, signal=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, weight_shift=64, score=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_signal=4097, workspace=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, prepared=None, workspace_bytes=0) == WN_ERR_NULL


def _hand_model():
    import wavenet_speech_amd as W
    return W.SignalModel(torch.tensor([[10, 1 << 16, 0], [20, 1 << 16, 0], [30, 1 << 16, 0], [40, 1 << 16, 0]]), 16, frac_bits=0, cost_bits=0)


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    from wavenet_speech_amd import mapping
    assert W.signal_map is mapping.signal_map and W.map_reference is mapping.map_reference
    assert W.MapReference is mapping.MapReference and W.SignalMapping is mapping.SignalMapping
    model = _hand_model()
    with pytest.raises(ValueError, match="SignalModel"):
        W.map_reference([1, 2, 3], (torch.zeros(4), torch.ones(4)))
    for bases in ([], [[1, 2], [3, 4]], [1.0, 2.0], [True, False]):
        with pytest.raises(ValueError, match="1-d integers"):
            W.map_reference(bases, model)
    five = W.SignalModel(torch.tensor([[10, 1 << 16, 0]] * 1024), 16)
    with pytest.raises(ValueError, match="at least k = 5"):
        W.map_reference([1, 2, 3, 4], five)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.map_reference([1, 2, 3, 4], model, device="cpu")
    # signal_map looks at its signal first, as signal_align does; then at the reference
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.signal_map(torch.zeros(1, 10), [10], None)


def test_reverse_complement_join():
    import wavenet_speech_amd as W
    from tests import signal_map_ref as R
    assert W.join_strands(torch.tensor([1, 2, 2, 4])).tolist() == [1, 2, 2, 4, 0, 1, 3, 3, 4]
    assert W.join_strands(torch.tensor([1, 0, 3], dtype=torch.int32)).tolist() == [1, 0, 3, 0, 2, 0, 4]       # a break stays a break
    assert W.join_strands([4, 7, -1, 1]).tolist() == [4, 7, -1, 1, 0, 4, -1, 7, 1]                            # faults stay, to be counted
    gen = torch.Generator().manual_seed(3)
    bases = torch.randint(0, 5, (300,), generator=gen)
    joined = W.join_strands(bases)
    assert joined.dtype == bases.dtype and joined.tolist() == R.join_strands(bases.tolist())
    assert W.join_strands(joined[301:]).tolist()[301:] == bases.tolist()                                       # an involution
