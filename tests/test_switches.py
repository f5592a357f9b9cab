"""CPU: what the product library and the package read from the environment is what csrc/wn_knobs.h and INTEGRATION.md section 5
say, and the measurement knobs (which change packed layouts and switch stores off) do not reach libwavenet_amd.so at all."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

from tests.abi_util import ROOT

KNOBS_H = os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_knobs.h")


def _list(macro):
    """the names of one X-macro list of wn_knobs.h"""
    body = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)" % macro, open(KNOBS_H).read()).group(1)
    return re.findall(r"X\((WN_[A-Z0-9_]+)\)", body)


def test_the_product_library_holds_the_switches_and_no_measurement_knob():
    from wavenet_speech_amd import _lib
    product, measure = _list("WN_PRODUCT_SWITCHES"), _list("WN_MEASURE_KNOBS")
    assert len(product) == 5 and len(measure) == 11 and not set(product) & set(measure), (product, measure)
    image = open(_lib.LIB_PATH, "rb").read()
    assert [n for n in product if n.encode() + b"\0" not in image] == []
    assert [n for n in measure if n.encode() in image] == []


def test_the_documented_switches_are_the_ones_that_are_read():
    read = set()
    for path in glob.glob(os.path.join(ROOT, "wavenet_speech_amd", "**", "*.py"), recursive=True):
        read |= set(re.findall(r"""os\.environ(?:\.get\(|\[)\s*["'](WN_[A-Z0-9_]+)["']""", open(path).read()))
    assert {"WN_FUSED_FWD", "WN_NLL_CHECK", "WN_HEAD_F32"} <= read, sorted(read)         # the expression finds them
    section = re.search(r"^## 5\. .*?(?=^## |\Z)", open(os.path.join(ROOT, "INTEGRATION.md")).read(), re.S | re.M).group(0)
    documented = set()
    for row in re.findall(r"^\|(.*?)\|", section, re.M):
        documented |= set(re.findall(r"WN_[A-Z0-9_]+", row))
    assert documented == read | set(_list("WN_PRODUCT_SWITCHES")), sorted(documented ^ (read | set(_list("WN_PRODUCT_SWITCHES"))))


LAYOUT_KNOBS = {"WN_MT2_MASK": "7", "WN_DZ_MT": "4", "WN_GEMM_VARIANT": "1", "WN_HGEMM16_COLS": "128"}


def _f32_block_sizes():
    """(wn_block_packed_bytes, wn_block_wgrad_workspace_bytes) of the f32 block in = out = skip = 160, k = 2, d = 1, B = 1, L = 256:
    five 32-channel tiles, the smallest width at which 64-row against 128-row slabs change the packed size (dz: 6 tile rows at MT 2,
    8 at MT 4; gate: 10 at MT 2, 12 at MT 4)"""
    from wavenet_speech_amd import _lib
    lib = _lib.load()
    ld, halo = _lib.series_layout(256, 1)
    shape = _lib.BlockShape(1, 256, 160, 160, 160, 2, 1, 1, ld, halo)
    return [lib.wn_block_packed_bytes(ctypes.byref(shape)), lib.wn_block_wgrad_workspace_bytes(ctypes.byref(shape))]


def test_layout_knobs_do_not_move_the_packed_layout(monkeypatch):
    for name in LAYOUT_KNOBS:
        monkeypatch.delenv(name, raising=False)
    here = _f32_block_sizes()
    assert here[0] > 0 and here[1] > 0, here
    r = subprocess.run([sys.executable, "-c", "import json; from tests.test_switches import _f32_block_sizes as f; print(json.dumps(f()))"],
                       env=dict(os.environ, **LAYOUT_KNOBS), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == here
