"""What the C ABI tests share (tests/test_*_abi.py, tests/test_cabi_symbols.py): the status codes, a fake device pointer, and the
rule that holds a ctypes row of wavenet_speech_amd._lib.SIGNATURES against its declaration in include/wavenet_amd.h."""
import ctypes
import os
import re

WN_OK, WN_ERR_BAD_SHAPE, WN_ERR_UNSUPPORTED, WN_ERR_NULL, WN_ERR_WORKSPACE = 0, -1, -2, -3, -5
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced: every call made with it returns before it would be used
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wavenet_amd.h")

SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
           "double": ctypes.c_double, "unsigned long long": ctypes.c_ulonglong}
STRUCTS = {"wn_block_shape": "BlockShape", "wn_block_params": "BlockParams", "wn_skipsum_shape": "SkipSumShape",
           "wn_mem_range": "MemRange", "wn_conv_shape": "ConvShape", "wn_pack_conv": "PackConv"}       # header -> _lib


def header_text():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_row(name):
    """(result type, [parameter declarations]) of a function as the header writes them, white space normalised"""
    m = re.search(r"(\w[\w ]*?\*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, header_text())
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return " ".join(m.group(1).split()), [] if params == ["void"] else params


def header_names(name):
    return [p.replace("*", " ").split()[-1] for p in header_row(name)[1]]


def _fits(decl, ctype, opaque):
    """the argument-type rule: a scalar is its ctypes type; const char* as a result is c_char_p; a pointer to a wn_* struct is
    POINTER of the matching Structure; any other pointer is c_void_p or a ctypes POINTER (only c_void_p with opaque=True: a row
    whose pointers are all device pointers, which travel as integers); wn_stream_t is c_void_p"""
    from wavenet_speech_amd import _lib
    if decl == "const char*":
        return ctype is ctypes.c_char_p
    if decl == "wn_stream_t":
        return ctype is ctypes.c_void_p
    if "*" in decl:
        base = decl.replace("const", "").replace("*", "").strip()
        if base in STRUCTS and not opaque:
            return ctype is ctypes.POINTER(getattr(_lib, STRUCTS[base]))
        return ctype is ctypes.c_void_p or (not opaque and isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))
    return ctype is SCALARS[decl]


def check_row(name, count=None, opaque=False):
    """_lib.SIGNATURES[name] has the header's result type, its number of arguments (and `count`, if given) and its types"""
    from wavenet_speech_amd import _lib
    res_text, params = header_row(name)
    res, args = _lib.SIGNATURES[name]
    assert _fits(res_text, res, opaque), (name, res_text, res)
    assert len(params) == len(args), (name, len(params), len(args))
    assert count is None or len(args) == count, (name, len(args), count)
    for p, ctype in zip(params, args):
        assert _fits(p.rsplit(" ", 1)[0], ctype, opaque), (name, p, ctype)            # the declaration without the argument's name
