"""CPU: the C ABI of the signal mapping (csrc/wn_sigmap.hip): the exported symbols, the ctypes rows against the header argument by
argument, the size functions, and every host-side rejection on both sides of its limit and in its documented order (shape,
unsupported, NULL, workspace), with fake pointers: every call below returns before anything would be launched.  And what
map_reference / signal_map refuse before they reach the library, and the reverse-complement join."""
import ctypes

import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry, header_text
from tests.abi_util import lib  # noqa: F401

MAP = Entry("wn_signal_map", dict(signal=FAKE, signal_kind=0, signal_stride=1000, signal_lengths=FAKE, scale_shift=FAKE, prepared=FAKE, ref_len=5000,
                                  k=5, batch=2, max_signal=1000, frac_bits=12, weight_shift=40, max_cost=2 ** 31 - 1, strip_states=0, score=FAKE,
                                  end=FAKE, start=FAKE, runner_up=FAKE, block_cost=FAKE, block_end=FAKE, end_cost=FAKE, workspace=FAKE,
                                  workspace_bytes=0, bad=None, stream=None))         # workspace_bytes 0: never launches
MAP_SIZE = Entry("wn_signal_map_workspace_bytes", dict(batch=2, max_signal=1000, ref_len=5000, k=5, strip_states=0))
REFERENCE = Entry("wn_signal_map_reference", dict(ref=FAKE, ref_len=1000, model=FAKE, k=5, prepared=FAKE, prepared_bytes=0, bad=None,
                                                  stream=None))      # prepared_bytes 0: never launches
REFERENCE_SIZE = Entry("wn_signal_map_reference_bytes", dict(ref_len=1000, k=5))


def test_symbols_are_exported(lib):
    for entry in (MAP, MAP_SIZE, REFERENCE, REFERENCE_SIZE):
        entry.check_exported(lib)
    assert "#define WN_MAP_GRANULE 64" in header_text()


def test_signature_rows_match_the_header():
    for entry in (MAP, MAP_SIZE, REFERENCE, REFERENCE_SIZE):         # 25, 5, 8 and 2 arguments
        entry.check_declared()


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


def test_reference_rejects_on_the_host_in_order(lib):
    assert REFERENCE(lib) == WN_ERR_WORKSPACE
    REFERENCE.rejects(lib, "ref", shape=(dict(ref_len=0), dict(ref_len=-1), dict(ref_len=4), dict(ref_len=4, k=7)),
                      unsupported=(dict(k=0), dict(k=-1), dict(k=7), dict(ref_len=2 ** 26 + 1)),
                      accepted=(dict(k=1), dict(k=6), dict(ref_len=5), dict(ref_len=2 ** 26), dict(ref_len=1, k=1)),
                      required=("ref", "model", "prepared"))
    need = REFERENCE_SIZE(lib)
    assert REFERENCE(lib, prepared_bytes=need - 1) == WN_ERR_WORKSPACE
    assert REFERENCE(lib, prepared=ctypes.c_void_p((1 << 20) + 8), prepared_bytes=need) == WN_ERR_WORKSPACE
    assert REFERENCE(lib, ref_len=0, k=7, ref=None) == WN_ERR_BAD_SHAPE
    assert REFERENCE(lib, k=7, ref=None) == WN_ERR_UNSUPPORTED
    assert REFERENCE(lib, model=None, prepared_bytes=0) == WN_ERR_NULL


def test_rejects_on_the_host_in_order(lib):
    assert MAP(lib) == WN_ERR_WORKSPACE                              # everything else about the default call is accepted
    MAP.rejects(lib, "signal",
                shape=(dict(batch=0), dict(batch=-2), dict(max_signal=0), dict(max_signal=-5), dict(ref_len=0), dict(ref_len=-1), dict(ref_len=4),
                       dict(signal_stride=-1), dict(signal_kind=2), dict(signal_kind=-1)),
                unsupported=(dict(k=0), dict(k=7, ref_len=5000), dict(frac_bits=-1), dict(frac_bits=21), dict(weight_shift=15),
                             dict(weight_shift=64), dict(max_cost=0), dict(max_cost=-1), dict(max_signal=4097), dict(ref_len=2 ** 26 + 1),
                             dict(batch=65536), dict(strip_states=32), dict(strip_states=96), dict(strip_states=-64),
                             dict(strip_states=2 ** 20 + 64), dict(strip_states=1),
                             # a grid of 2^31 workgroups or more: 2^20 strips of 64 states for each of 2048 reads
                             dict(ref_len=2 ** 26, k=1, strip_states=64, batch=2048, signal=None)),
                accepted=(dict(k=1), dict(k=6), dict(frac_bits=0), dict(frac_bits=20), dict(weight_shift=16), dict(weight_shift=63),
                          dict(max_cost=1), dict(max_cost=2 ** 31 - 1), dict(max_signal=4096), dict(max_signal=1), dict(ref_len=2 ** 26),
                          dict(ref_len=5), dict(batch=65535), dict(batch=1), dict(strip_states=64), dict(strip_states=576),
                          dict(strip_states=2 ** 20), dict(signal_kind=1), dict(signal_stride=0), dict(ref_len=1, k=1),
                          # one strip fewer per read passes, and so do strips twice as wide
                          dict(ref_len=2 ** 26 - 64, k=1, strip_states=64, batch=2048), dict(ref_len=2 ** 26, k=1, strip_states=128, batch=2048)),
                required=("signal", "signal_lengths", "prepared", "score", "end", "start", "runner_up", "block_cost", "block_end", "workspace"))
    for name in ("scale_shift", "end_cost", "bad"):                  # optional
        assert MAP(lib, **{name: None}) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and a signal off its element size
    need = MAP_SIZE(lib)
    assert need == (2 * 4 * 79 + 15) // 16 * 16                      # 4996 states: 79 blocks
    assert MAP(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert MAP(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert MAP(lib, signal=ctypes.c_void_p((1 << 20) + 2), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert MAP(lib, signal=ctypes.c_void_p((1 << 20) + 1), signal_kind=1, workspace_bytes=need) == WN_ERR_WORKSPACE
    assert MAP(lib, batch=3, workspace_bytes=need) == WN_ERR_WORKSPACE               # the size follows the batch
    # the order: shape, then unsupported, then NULL, then workspace
    assert MAP(lib, batch=0, k=7, signal=None) == WN_ERR_BAD_SHAPE
    assert MAP(lib, signal_kind=2, strip_states=96, prepared=None) == WN_ERR_BAD_SHAPE
    assert MAP(lib, ref_len=4, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert MAP(lib, k=7, signal=None) == WN_ERR_UNSUPPORTED
    assert MAP(lib, weight_shift=64, score=None) == WN_ERR_UNSUPPORTED
    assert MAP(lib, max_signal=4097, workspace=None) == WN_ERR_UNSUPPORTED
    assert MAP(lib, prepared=None, workspace_bytes=0) == WN_ERR_NULL


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
