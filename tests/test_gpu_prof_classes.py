"""GPU: the launches of the units outside wn_api.hip / wn_half_api.hip are booked under their own kernel classes.  The embedding
gather, the signal generator, the CTC loss and the front-end kernels name their class by the enumerator of the one table in
csrc/wn_host.h; what wn_prof_* then reports for them is pinned here.  (tests/test_gpu_joint.py and tests/test_gpu_classifier.py
see ctc_kernel and hload_kernel among a whole step's launches; none of them holds a unit to exactly its class.)"""
import ctypes

import pytest
import torch

from wavenet_speech_amd import _lib
from wavenet_speech_amd import functional as F
from wavenet_speech_amd import functional_half as HF
from wavenet_speech_amd import synthetic as S
from wavenet_speech_amd import training as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _launches():
    torch.cuda.synchronize()
    return {k: v[1] for k, v in F.profile_read().items()}


def _gained(before):
    after = _launches()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


@pytest.fixture
def profiling():
    F.profile_reset()
    F.profile_enable(True)
    yield
    F.profile_enable(False)
    F.profile_reset()


def _feature_args(mode_name="f16"):
    """batch 1, length 64, 8 features, 3 taps, as _HalfStackFn.forward sets the call up (the layer lengthens the series by k - 1)"""
    torch.manual_seed(0)
    lib = _lib.load()
    x = torch.randn(1, 1, 64, device=DEV)
    params = [torch.randn(8, 1, 3, device=DEV), torch.randn(8, device=DEV), torch.randn(8, 8, 1, device=DEV), torch.randn(8, device=DEV)]
    c = HF._hcall(lib, 1, HF.HalfLayout(64 + 3 - 1, 1), torch.device(DEV), HF._Mode(mode_name))
    return lib, c, x, params


def test_each_unit_books_its_own_class(profiling):
    torch.manual_seed(0)
    # embedding gather: batch 1, 100 levels (one column tile), 8 classes -> 16 channels, 2 taps
    before = _launches()
    with torch.no_grad():
        F.embed_conv(torch.randint(0, 8, (1, 100), device=DEV), torch.randn(16, 8, 2, device=DEV), torch.randn(16, device=DEV))
    assert _gained(before) == {"embed_kernel": 1}
    # signal generator: one read of 4 bases
    before = _launches()
    S.hip_bases(1, 4, 7, DEV)
    assert _gained(before) == {"synth_kernel": 1}
    # CTC loss: 8 frames, 5 classes, a target of length 2
    before = _launches()
    x = torch.randn(1, 5, 8, device=DEV, requires_grad=True)
    T.ctc_total(x, torch.tensor([[1, 2]], device=DEV), torch.tensor([2], device=DEV))
    assert _gained(before) == {"ctc_kernel": 1}
    # feature layer: the entry point alone, with the arguments functional_half._input_series gives it (the wrapper itself also
    # packs and runs the layer's 1x1 conv: below)
    lib, c, x, (fw0, fb0, _fw1, _fb1) = _feature_args()
    f1 = HF._lease(c, 8)
    before = _launches()
    _lib.check(lib.wn_hfeature_forward(c.mode.code, F._p(x), F._p(fw0), F._p(fb0), F._p(f1), 1, 64, 8, 3, c.layout.ld, c.layout.halo,
                                       ctypes.c_float(c.rs), ctypes.c_float(0.01), F._p(c.flag), F._stream()), "wn_hfeature_forward")
    assert _gained(before) == {"hload_kernel": 1}
    # and over all four: exactly these classes gained launches
    assert {k for k, n in _launches().items() if n} == {"embed_kernel", "synth_kernel", "ctc_kernel", "hload_kernel"}
    # the wrapper itself, functional_half._input_series with a feature layer: wn_hfeature_forward again, then the pack and the
    # series forward of the layer's 1x1 conv, which wn_half_api.hip books under their own classes
    lib, c, x, params = _feature_args()
    before = _launches()
    HF._input_series(c, x, 1, (0.01, 0.01), params)
    assert _gained(before) == {"hload_kernel": 1, "pack_kernel": 1, "hgemm_kernel<conv_fwd>": 1}
    HF.check_fp16_overflow()
