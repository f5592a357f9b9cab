"""What the C ABI tests share (tests/test_*_abi.py, tests/test_cabi_symbols.py): the status codes, a fake device pointer, the
rule that holds a ctypes row of wavenet_speech_amd._lib.SIGNATURES against its declaration in include/wavenet_amd.h, and Entry:
one entry point with its default arguments, called by keyword and held to the header and to its refusals."""
import ctypes
import os
import re

import pytest

WN_OK, WN_ERR_BAD_SHAPE, WN_ERR_UNSUPPORTED, WN_ERR_NULL, WN_ERR_WORKSPACE = 0, -1, -2, -3, -5
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced: every call made with it returns before it would be used
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wavenet_amd.h")

SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
           "double": ctypes.c_double, "unsigned long long": ctypes.c_ulonglong}
STRUCTS = {"wn_block_shape": "BlockShape", "wn_block_params": "BlockParams", "wn_skipsum_shape": "SkipSumShape",
           "wn_mem_range": "MemRange", "wn_conv_shape": "ConvShape", "wn_pack_conv": "PackConv"}       # header -> _lib


@pytest.fixture(scope="module")
def lib():
    """libwavenet_amd.so; a test module imports this name to use it"""
    from wavenet_speech_amd import _lib
    return _lib.load()


def header_text():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared_functions():
    """the wn_* names the header declares"""
    return sorted(set(re.findall(r"\b(wn_[a-z0-9_]+)\s*\(", header_text())))


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


class Entry:
    """One entry point of the C ABI.  `defaults` maps every argument, by the header's name and in the header's order, to the value
    a call passes unless told otherwise; a function there is called with the merged arguments (a stride that follows a shape)."""

    def __init__(self, name, defaults, version=300):
        self.name, self.defaults, self.version = name, defaults, version

    def __call__(self, lib, **kw):
        assert set(kw) <= set(self.defaults), kw
        a = dict(self.defaults, **kw)
        args = [v(a) if callable(v) else v for v in a.values()]
        return getattr(lib, self.name)(*[ctypes.cast(v, ctypes.c_void_p) if isinstance(v, ctypes.Array) else v for v in args])

    def check_exported(self, lib):
        from wavenet_speech_amd import _lib
        assert self.name in _lib.SIGNATURES and hasattr(lib, self.name), self.name
        assert lib.wn_version() == self.version                     # every entry point since has been additive

    def check_declared(self, opaque=True):
        """the ctypes row against the header, type by type, and `defaults` against its count and its argument names"""
        check_row(self.name, count=len(self.defaults), opaque=opaque)
        assert header_names(self.name) == list(self.defaults), self.name

    def rejects(self, lib, null, shape=(), unsupported=(), accepted=(), required=()):
        """both sides of every limit: every accepted case goes on to the NULL check (`null`=None), so nothing is ever launched"""
        for kw in shape:
            assert self(lib, **kw) == WN_ERR_BAD_SHAPE, kw
        for kw in unsupported:
            assert self(lib, **kw) == WN_ERR_UNSUPPORTED, kw
        for kw in accepted:
            assert self(lib, **dict(kw, **{null: None})) == WN_ERR_NULL, kw
        for name in required:
            assert self(lib, **{name: None}) == WN_ERR_NULL, name


# ---- the read batch: the 16 arguments that wn_pileup, wn_pileup_evidence, wn_phase_links and wn_haplotag begin with (one
# ReadBatch, checked by one check_read_batch in csrc/wn_host.h), and the limits of those, of min_qual and of the optional `bad`,
# which each takes later.  What an entry point adds (max_ins, reach, flat_qual, n_sites, its least reference_len) is in its own file
READ_BATCH = dict(ops=FAKE, ops_stride=900, ops_len=FAKE, lo=FAKE, ref_lengths=FAKE, strand=FAKE, query=FAKE, query_stride=400,
                  query_lengths=FAKE, qual=None, qual_stride=0, keep=None, batch=2, max_query_len=400, max_ops=900, reference_len=5000)
READ_REQUIRED = ("ops", "ops_len", "lo", "ref_lengths", "strand", "query", "query_lengths")
READ_SHAPE = (dict(batch=0), dict(batch=-1), dict(max_query_len=0), dict(max_ops=0), dict(reference_len=0), dict(ops_stride=-1),
              dict(query_stride=-1), dict(qual_stride=-1), dict(min_qual=-1))
READ_UNSUPPORTED = (dict(batch=65536), dict(max_query_len=8193), dict(max_ops=65535 + 8192 + 1), dict(reference_len=2 ** 26 + 1),
                    dict(min_qual=94))
READ_ACCEPTED = (dict(batch=1), dict(batch=65535), dict(max_query_len=1), dict(max_query_len=8192), dict(max_ops=1),
                 dict(max_ops=65535 + 8192), dict(reference_len=2 ** 26), dict(min_qual=0), dict(min_qual=93), dict(ops_stride=0),
                 dict(qual=FAKE, qual_stride=400), dict(keep=FAKE), dict(bad=FAKE))


def host_alignment(B=2, n=30):
    """a PairwiseAlignment whose ops are on the host: what the Python surfaces refuse"""
    import torch
    import wavenet_speech_amd as W
    return W.PairwiseAlignment(None, None, None, None, None, torch.ones(B, n, dtype=torch.uint8), torch.full((B,), n, dtype=torch.int32))


def hand_made_genotypes():
    """the case of tests/test_genotype_ref.py::test_records_by_hand as tensors"""
    import torch
    import wavenet_speech_amd as W
    U = W.Genotypes
    ref = [1, 2, 3, 4, 1, 2, 3, 4]
    alleles = [(0, 0), (2, 0), (1, 0), (4, 0), (2, 2), (2, 0), (0, 0), (1, 2)]
    flags = [U.DELETION, U.DELETION | U.HET, U.SUBSTITUTION | U.DELETION | U.HET, U.DELETION | U.HET, U.SUBSTITUTION | U.INSERTION | U.INS_HET,
             U.DELETION | U.HET, U.DELETION, U.SUBSTITUTION | U.HET]
    R = len(ref)
    counts = torch.zeros(R, 2, 6, dtype=torch.int32)
    counts[:, 0, 0] = torch.arange(R, dtype=torch.int32) + 3
    pile = W.Pileup(counts, torch.zeros(R, 3, dtype=torch.int32), torch.zeros(R, 2, 4, dtype=torch.int32), None)
    u8 = lambda v: torch.tensor(v, dtype=torch.uint8)                # noqa: E731
    i32 = lambda k, c: (torch.arange(R) * k + c).to(torch.int32)     # noqa: E731
    ins_bases = torch.zeros(R, 2, dtype=torch.uint8)
    ins_bases[4] = u8([4, 1])
    g = W.Genotypes(u8(alleles), i32(100, 1), i32(1000, 2), u8(flags), u8([0, 0, 0, 0, 1, 0, 0, 0]), u8([0, 0, 0, 0, 2, 0, 0, 0]), ins_bases,
                    i32(10, 5), i32(10, 7), None)
    return ref, g, pile
