"""GPU: the call schedule and the statistics of tools/gputime.timed, the one device-event timer of the tool benches.  Without
min_seconds the number of calls is exact: warmup + windows * (warm_each + calls)."""
import pytest
import torch

from tools.gputime import timed

pytestmark = pytest.mark.gpu


@pytest.fixture
def counted():
    x, n = torch.zeros(1, device="cuda:0"), [0]

    def fn():
        n[0] += 1
        x.add_(1)
    return fn, n, x


def test_the_calls_are_warmup_plus_windows_of_warm_each_and_calls(counted):
    fn, n, x = counted
    t = timed(fn, calls=5, windows=3, warmup=2)
    assert n[0] == 17 and t.calls == 5 and len(t.ms) == 3
    n[0] = 0
    timed(fn, calls=5, windows=3, warmup=2, warm_each=1)
    assert n[0] == 20
    assert int(x.item()) == 37                                       # every call ran on the device


@pytest.mark.parametrize("windows", [1, 2, 5])
def test_the_windows_come_sorted_and_the_median_is_element_n_over_2(counted, windows):
    t = timed(counted[0], calls=3, windows=windows)
    assert len(t.ms) == windows and t.ms == sorted(t.ms) and all(v > 0 for v in t.ms)
    assert (t.least, t.median, t.greatest) == (t.ms[0], t.ms[windows // 2], t.ms[-1])
    if windows == 1:
        assert t.least == t.median == t.greatest


def test_short_windows_are_thrown_away_and_grown_by_four(counted):
    fn, n, _ = counted
    t = timed(fn, calls=1, windows=2, warmup=3, min_seconds=0.02)
    sizes = [4 ** k for k in range(7)]
    assert t.calls in sizes                                          # a power of 4, at most 4096
    assert n[0] == 3 + sum(s for s in sizes if s < t.calls) + 2 * t.calls
    assert len(t.ms) == 2
    # the first kept window lasted min_seconds or the growth hit its ceiling.  Which of two sorted values came first is not
    # known, so the greater is the necessary half; with one window the kept one is the first
    assert t.greatest * t.calls >= 20.0 or t.calls == 4096
    one = timed(fn, calls=1, min_seconds=0.02)
    assert one.calls in sizes and (one.median * one.calls >= 20.0 or one.calls == 4096)
