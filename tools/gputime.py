"""The one device-event timer of the tool benches, and the tail they share: where a report goes."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Timing = collections.namedtuple("Timing", "least median greatest ms calls")


def timed(fn, calls=1, windows=1, warmup=0, warm_each=0, min_seconds=0.0, max_calls=4096):
    """ms per call of `fn` over `windows` windows: `warmup` calls and a synchronise; then per window `warm_each` calls and a
    synchronise, one event pair around `calls` calls, a synchronise.  While no window has been kept, one that lasted under
    `min_seconds` is thrown away and `calls` multiplied by 4, up to `max_calls`.  The kept windows sorted (`ms`), their least,
    median (element n // 2) and greatest, and the `calls` of a kept window."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    kept = []
    while len(kept) < windows:
        for _ in range(warm_each):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        if not kept and ms < 1e3 * min_seconds and calls < max_calls:
            calls *= 4
            continue
        kept.append(ms / calls)
    kept.sort()
    return Timing(kept[0], kept[len(kept) // 2], kept[-1], kept, calls)


def next_profile_dir():
    """profiles/rNN of the next free NN"""
    base = os.path.join(ROOT, "profiles")
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)$", n) for n in (os.listdir(base) if os.path.isdir(base) else [])) if m]
    return os.path.join(base, "r%02d" % (max(taken, default=0) + 1))


class Report:
    """the lines a tool prints, kept for the file it writes"""

    def __init__(self):
        self.lines = []

    def emit(self, line):
        print(line, flush=True)
        self.lines.append(line)

    def save(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(self.lines) + "\n")
