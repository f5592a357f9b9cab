"""CPU: the host-side decisions of the stack functions (functional / functional_half) that need no device -- the parameter shapes of
a block, what the pack-table and packed-weight cache keys depend on, and the backward-data form chosen for a block."""
import itertools

import pytest
import torch

from wavenet_speech_amd import functional_half as FH
from wavenet_speech_amd.functional import BlockSpec, PackCache
from wavenet_speech_amd.modules.block import packed_weights_key


@pytest.mark.parametrize("k", [2, 3])
def test_param_shapes_are_the_c_abi_order(k):
    ci, co, ms = 5, 7, 3
    assert BlockSpec(ci, co, ms, k, 4, True).param_shapes() == [
        (7, 5, k), (7,), (7, 5, k), (7,), (7, 7), (7,), (3, 7), (3,), (7, 5), (7,)]


def _stack(wf, bf, params):
    """(specs, caller's tensors, prepared tensors) of a two-block stack: nn.Parameters, the skip projections slices of wf / bf"""
    specs = [BlockSpec(8, 8, 4, 2, d, True) for d in (1, 2)]
    flat, prepped = [], []
    for l in range(2):
        blk = list(params[8 * l:8 * l + 6]) + [wf[l], bf[l]] + list(params[8 * l + 6:8 * l + 8])
        flat += blk
        prepped.append([t.detach() for t in blk])
    return specs, flat, prepped


def _half_key(wf, bf, params):
    specs, flat, prepped = _stack(wf, bf, params)
    storages = FH.StackPackTable.dynamic_storages(flat)
    assert len(storages) == 2
    return FH.StackPackTable.key_of(specs, FH._Mode("bf16"), 2, FH.HalfLayout(100, 2), prepped, storages, True)


def test_half_pack_table_key_follows_the_plan_switches(monkeypatch):
    shapes = [(8, 8, 2), (8,), (8, 8, 2), (8,), (8, 8, 1), (8,), (8, 8), (8,)] * 2
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    wf, bf = torch.zeros(2, 4, 8), torch.zeros(2, 4)
    monkeypatch.delenv("WN_FUSED_FWD", raising=False)
    monkeypatch.delenv("WN_COL_BWD", raising=False)
    base = _half_key(wf, bf, params)
    assert _half_key(wf, bf, params) == base
    wf2, bf2 = torch.ones(2, 4, 8), torch.ones(2, 4)         # the dynamic tensors move: new storages of the same sizes
    assert wf2.data_ptr() != wf.data_ptr() and bf2.data_ptr() != bf.data_ptr()
    assert _half_key(wf2, bf2, params) == base
    keys = {base}
    for name in ("WN_FUSED_FWD", "WN_COL_BWD"):
        monkeypatch.setenv(name, "0")
        keys.add(_half_key(wf, bf, params))
        assert _half_key(wf2, bf2, params) == _half_key(wf, bf, params)
        monkeypatch.delenv(name)
    assert len(keys) == 3 and _half_key(wf, bf, params) == base


class _Layout(object):
    def key(self):
        return ("layout",)


def test_kept_packed_weights_follow_the_plan_switches(monkeypatch):
    monkeypatch.delenv("WN_FUSED_FWD", raising=False)
    monkeypatch.delenv("WN_COL_BWD", raising=False)
    params = [torch.nn.Parameter(torch.zeros(3))]
    for name in ("WN_FUSED_FWD", "WN_COL_BWD"):
        c = PackCache()
        c.validate(params, packed_weights_key("bf16"))
        c.put(0, _Layout(), 1, "packed")
        c.validate(params, packed_weights_key("bf16"))
        assert c.get(0, _Layout(), 1) == "packed"            # nothing changed: kept
        monkeypatch.setenv(name, "0")
        c.validate(params, packed_weights_key("bf16"))
        assert not c.packed and c.get(0, _Layout(), 1) is None
        assert packed_weights_key("f32") == ("f32",)         # the fp32 plan reads no switch
        monkeypatch.delenv(name)


T, P, I, N, M, D = FH.BWD_TOP_PAIR, FH.BWD_PAIR, FH.BWD_INPUT, FH.BWD_NOTHING, FH.BWD_MASKED, FH.BWD_PLAIN
# (paired, have_dz, dx wanted as a series, dense dx wanted, masked) -> the branch the if/elif chain of the former backward took
FORMS = {
    (0, 0, 0, 0, 0): D, (0, 0, 0, 0, 1): M, (0, 0, 0, 1, 0): D, (0, 0, 0, 1, 1): M,
    (0, 0, 1, 0, 0): D, (0, 0, 1, 0, 1): M, (0, 0, 1, 1, 0): D, (0, 0, 1, 1, 1): M,
    (0, 1, 0, 0, 0): N, (0, 1, 0, 0, 1): N, (0, 1, 0, 1, 0): I, (0, 1, 0, 1, 1): I,
    (0, 1, 1, 0, 0): I, (0, 1, 1, 0, 1): I, (0, 1, 1, 1, 0): I, (0, 1, 1, 1, 1): I,
    (1, 0, 0, 0, 0): T, (1, 0, 0, 0, 1): T, (1, 0, 0, 1, 0): T, (1, 0, 0, 1, 1): T,
    (1, 0, 1, 0, 0): T, (1, 0, 1, 0, 1): T, (1, 0, 1, 1, 0): T, (1, 0, 1, 1, 1): T,
    (1, 1, 0, 0, 0): P, (1, 1, 0, 0, 1): P, (1, 1, 0, 1, 0): P, (1, 1, 0, 1, 1): P,
    (1, 1, 1, 0, 0): P, (1, 1, 1, 0, 1): P, (1, 1, 1, 1, 0): P, (1, 1, 1, 1, 1): P,
}


def test_backward_data_form_is_the_former_if_chain():
    assert len(FORMS) == 32 and len({T, P, I, N, M, D}) == 6
    for args in itertools.product((0, 1), repeat=5):
        form = FH.backward_data_form(*[bool(a) for a in args])
        assert form == FORMS[args], args
        if not (args[2] or args[3]):
            assert form != I, args             # the input-only launch with no destination would write through a null pointer
