"""CPU: the host-side argument layer (wavenet_speech_amd/_args.py), helper by helper.  Nothing here launches or loads the library:
a CPU tensor is enough to reach the refusal of a CPU tensor, and the rules that come after it are exercised on CPU tensors that
answer is_cuda with True."""
import pytest
import torch

from wavenet_speech_amd import _args

CPU = torch.device("cpu")


@pytest.fixture
def as_gpu(monkeypatch):
    """the dtype, shape and stride rules of the helpers, on CPU tensors: while it holds, every tensor answers is_cuda with True"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def test_a_cpu_tensor_is_refused_by_every_helper_that_takes_device_data():
    x = torch.zeros(2, 8)
    rows = torch.ones(2, 4, dtype=torch.int32)
    for call in (lambda: _args.gpu_tensor(x, "tool", "x"), lambda: _args.gpu_tensor([1.0], "tool", "x"),
                 lambda: _args.signal_rows(x, "tool"), lambda: _args.signal_rows(x, "tool", error=TypeError, dense=True),
                 lambda: _args.int_rows(rows, "tool", "labels"), lambda: _args.lengths(torch.tensor([1, 2]), 2, CPU, "tool", "n", on_gpu=True),
                 lambda: _args.scale_shift(torch.zeros(2, 2), 2, CPU, "tool")):
        with pytest.raises(RuntimeError, match=r"wavenet_speech_amd\.tool: \w+ must be a GPU tensor \(there is no CPU fallback\)"):
            call()
    assert _args.scale_shift(None, 2, CPU, "tool") is None


def test_a_wrong_dtype_raises_the_class_passed_in(as_gpu):
    x = torch.zeros(2, 8, dtype=torch.float64)
    for error in (TypeError, ValueError):
        with pytest.raises(error, match="x must be float32 or int16, got torch.float64") as hit:
            _args.gpu_tensor(x, "tool", "x", (torch.float32, torch.int16), error)
        assert type(hit.value) is error
        with pytest.raises(error, match="signal must be float32 or int16") as hit:
            _args.signal_rows(x, "tool", error=error)
        assert type(hit.value) is error
    with pytest.raises(ValueError, match="labels must be int32 or int64 of shape"):
        _args.int_rows(torch.zeros(2, 3, dtype=torch.int16), "tool", "labels")
    with pytest.raises(ValueError, match="scale_shift must be float32"):
        _args.scale_shift(torch.zeros(2, 2, dtype=torch.float64), 2, CPU, "tool")


def test_signal_rows_shapes_and_the_two_contiguity_rules(as_gpu):
    wide = torch.arange(3 * 256, dtype=torch.float32).reshape(3, 1, 256)
    view = wide[:, :, 5:205]
    got = _args.signal_rows(view, "tool")
    assert tuple(got.shape) == (3, 200) and got.stride() == (256, 1) and got.data_ptr() == view.data_ptr()      # read in place
    dense = _args.signal_rows(view, "tool", dense=True)
    assert dense.is_contiguous() and dense.data_ptr() != view.data_ptr() and torch.equal(dense, got)
    strided = wide[:, 0, ::2]
    got = _args.signal_rows(strided, "tool")
    assert got.is_contiguous() and torch.equal(got, strided)         # a non-unit inner stride is copied
    column = wide[:, 0, ::256]
    assert _args.signal_rows(column, "tool").data_ptr() == column.data_ptr()        # one sample per read: any stride does
    same = torch.zeros(4, 16, dtype=torch.int16)
    assert _args.signal_rows(same, "tool", dense=True).data_ptr() == same.data_ptr()
    for bad in (torch.zeros(8), torch.zeros(2, 2, 8), torch.zeros(0, 8), torch.zeros(2, 0), torch.zeros(2, 1, 0)):
        with pytest.raises(ValueError, match=r"signal must be \[B, L\] or \[B, 1, L\]"):
            _args.signal_rows(bad, "tool")


def test_int_rows(as_gpu):
    beam = torch.arange(2 * 3 * 7, dtype=torch.int32).reshape(2, 3, 7)
    best = _args.int_rows(beam[:, 0], "tool", "labels", B=2)
    assert best.data_ptr() == beam.data_ptr() and best.stride() == (21, 1)           # a row stride is read in place
    long_rows = torch.arange(14, dtype=torch.int64).reshape(2, 7)
    got = _args.int_rows(long_rows, "tool", "labels")
    assert got.dtype == torch.int32 and torch.equal(got.long(), long_rows)
    qual = torch.zeros(2, 7, dtype=torch.uint8)
    assert _args.int_rows(qual, "tool", "qual", B=2, min_width=7, dtypes=(torch.uint8,)) .dtype == torch.uint8
    # a width-0 block becomes one unused column, only where asked for
    empty = torch.zeros(2, 0, dtype=torch.int64)
    padded = _args.int_rows(empty, "tool", "query", pad_empty=True)
    assert tuple(padded.shape) == (2, 1) and padded.dtype == torch.int32 and int(padded.abs().sum()) == 0
    assert tuple(_args.int_rows(empty, "tool", "query").shape) == (2, 0)
    # the inner stride: copied when it is not 1; a single column only under the pairwise tools' rule
    assert _args.int_rows(beam[:, 0, ::2], "tool", "labels").is_contiguous()
    lone = beam[:, 0, ::7]
    assert _args.int_rows(lone, "tool", "labels").data_ptr() == lone.data_ptr()
    copied = _args.int_rows(lone, "tool", "ref", lone_column_in_place=False)
    assert copied.data_ptr() != lone.data_ptr() and copied.stride(1) == 1 and torch.equal(copied, lone)
    for bad, kw in ((beam, {}), (beam[0, 0], {}), (beam[:, 0], dict(B=3)), (beam[:, 0], dict(min_width=8)),
                    (beam[:, 0].float(), {}), (qual, {})):
        with pytest.raises(ValueError, match="labels must be int32 or int64 of shape SHAPE, got"):
            _args.int_rows(bad, "tool", "labels", shape="SHAPE", **kw)


def test_lengths_keep_each_callers_strictness(as_gpu):
    got = _args.lengths([3, 4], 2, CPU, "tool", "n")
    assert got.dtype == torch.int32 and got.tolist() == [3, 4] and got.is_contiguous()
    assert _args.lengths(torch.tensor([3, 4], dtype=torch.int64)[::1], 2, CPU, "tool", "n").tolist() == [3, 4]
    for bad in ([3.0, 4.0], [True, False], [3, 4, 5], [[3, 4]], 3):
        with pytest.raises(ValueError, match=r"n must be integers of shape \(2,\)"):
            _args.lengths(bad, 2, CPU, "tool", "n")
        with pytest.raises(ValueError, match=r"n must be integers of shape \(2,\)"):
            _args.lengths(torch.as_tensor(bad), 2, CPU, "tool", "n", on_gpu=True)
    assert _args.lengths([[3.0], [4.0]], 2, CPU, "tool", "n", flatten=True).tolist() == [3, 4]      # the event tools' lenient form
    with pytest.raises(ValueError, match="n must hold 2 lengths, got 3"):
        _args.lengths([3, 4, 5], 2, CPU, "tool", "n", flatten=True)


def test_scale_shift(as_gpu):
    pair = torch.arange(8, dtype=torch.float32).reshape(2, 4)[:, ::2]
    got = _args.scale_shift(pair, 2, CPU, "tool")
    assert got.is_contiguous() and torch.equal(got, pair)
    for bad in (torch.zeros(3, 2), torch.zeros(2, 3), torch.zeros(2)):
        with pytest.raises(ValueError, match=r"scale_shift must be \[2, 2\]"):
            _args.scale_shift(bad, 2, CPU, "tool")


def test_into_table():
    class Earlier(object):
        counts = torch.ones(4, 5, dtype=torch.int64)
        missing = None

    fresh = _args.into_table(None, "counts", (4, 5), CPU, "tool")
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (4, 5) and int(fresh.abs().sum()) == 0
    assert _args.into_table(Earlier, "counts", (4, 5), CPU, "tool") is Earlier.counts                  # accumulated in place
    assert int(_args.into_table(Earlier, "missing", (4, 5), CPU, "tool").abs().sum()) == 0
    for table, shape in ((Earlier.counts, (5, 4)), (Earlier.counts.int(), (4, 5)), (torch.ones(5, 4, dtype=torch.int64).t(), (4, 5)),
                         ([[0] * 5] * 4, (4, 5))):
        Earlier.other = table
        with pytest.raises(ValueError, match="into.other must be a contiguous int64 tensor"):
            _args.into_table(Earlier, "other", shape, CPU, "tool")
    # the int32 tables of pileup: the same rules with the dtype named
    fresh = _args.into_table(None, "counts", (4, 5), CPU, "tool", torch.int32)
    assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (4, 5) and int(fresh.abs().sum()) == 0
    Earlier.small = torch.ones(4, 5, dtype=torch.int32)
    assert _args.into_table(Earlier, "small", (4, 5), CPU, "tool", torch.int32) is Earlier.small
    with pytest.raises(ValueError, match="into.counts must be a contiguous int32 tensor"):
        _args.into_table(Earlier, "counts", (4, 5), CPU, "tool", torch.int32)


def test_note_bad_without_a_counter_is_a_no_op(monkeypatch):
    class Watch(object):
        calls = []

        def poll(self):
            self.calls.append("poll")

        def note(self, flag, message, at_once):
            self.calls.append(("note", flag, at_once))

    monkeypatch.setattr(_args._flags, "WATCH", Watch())
    _args.note_bad(None, "never formatted")
    assert Watch.calls == []
    flag = torch.zeros(1, dtype=torch.int32)
    _args.note_bad(flag, "message")
    _args.note_bad(flag, "message", at_once=True)
    assert Watch.calls == ["poll", ("note", flag, False), "poll", ("note", flag, True)]           # earlier flags first, then this one


def test_alloc_bytes_raises_the_librarys_status_for_a_refused_shape(monkeypatch):
    seen = []
    monkeypatch.setattr(_args._lib, "check", lambda status, what: seen.append((status, what)))
    assert _args._alloc_bytes(48, "wn_query", CPU).numel() == 48 and seen == []
    _args._alloc_bytes(0, "wn_query", CPU, status=-2)
    assert seen == [(-2, "wn_query")]
    assert _args._p(None) is None and _args._p(4096).value == 4096
    t = torch.zeros(3)
    assert _args._p(t).value == t.data_ptr()
