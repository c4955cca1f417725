"""CPU-side checks of the checked call path (no GPU): abi.PROTOTYPES keeps what the header's prototypes say, lib.ops holds exactly the
launch entry points, and every pointer argument / pointer member is checked against its declaration BEFORE anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from stylesinger_amd import abi
from stylesinger_amd import lib as L

POINTEES = {"float", "double", "int32_t", "int64_t", "int16_t", "uint16_t", "uint8_t", "uint64_t", "int", "char", "void"} | set(abi.STRUCTS)


def test_every_declaration_has_a_prototype_with_the_same_shape():
    decl = abi.declarations()
    assert set(decl) == set(abi.PROTOTYPES) and len(decl) >= 100
    for name, (restype, argtypes) in decl.items():
        p = abi.PROTOTYPES[name]
        assert p.name == name and p.restype is restype and len(p.params) == len(argtypes), name
        for a, t in zip(p.params, argtypes):
            assert a.name, (name, a)
            assert (a.pointee is not None) == (t is ctypes.c_void_p), (name, a)
            if a.pointee is None:
                assert a.ctype is t and not a.const, (name, a)
            else:
                assert a.ctype is None and a.pointee in POINTEES, (name, a)
        last = p.params[-1] if p.params else None
        assert p.launch == (last is not None and last.pointee == "void" and last.name in ("stream", "stream_")), name
        assert p.text.split("(")[0].endswith(name)
    t = abi.PROTOTYPES["ss_table_add"].params
    assert [(a.name, a.pointee, a.const) for a in t[:4]] == [("pos", "int32_t", True), ("table", "float", True), ("table_rows", None, False), ("out", "float", False)]


def test_struct_pointees_cover_exactly_the_pointer_members():
    for name, fields in abi.STRUCTS.items():
        def is_ptr(t):
            while hasattr(t, "_length_"):
                t = t._type_
            return t is ctypes.c_void_p
        assert set(abi.STRUCT_POINTEES[name]) == {f for f, t in fields if is_ptr(t)}, name
    lp = abi.STRUCT_POINTEES["ss_layer512_args"]
    assert (lp["Hin"], lp["P"], lp["E512"], lp["lens"]) == ("uint16_t", "void", "float", "int32_t")
    assert abi.STRUCT_POINTEES["ss_gemm_bf16_args"]["C"] == "void" and abi.STRUCT_POINTEES["ss_wavenet"]["w_dil_h"] == "uint16_t"
    assert abi.STRUCT_POINTEES["ss_f0track_params"] == {}


@pytest.mark.parametrize("what, snippet, offending", [
    ("unnamed parameter", "int ss_x(const float*, int n, void* stream);", "const float*"),
    ("unnamed scalar", "int ss_x(const float* x, int, void* stream);", "'int'"),
    ("unknown pointee", "int ss_x(const half* x, int n, void* stream);", "const half* x"),
    ("struct the header does not define", "int ss_x(const ss_nothing* a, void* stream);", "const ss_nothing* a"),
    ("unknown scalar", "int ss_x(size_t n, void* stream);", "size_t n"),
    ("pointer to pointer", "int ss_x(float** x, void* stream);", "float** x"),
])
def test_prototype_parser_refuses_what_it_cannot_read(what, snippet, offending):
    with pytest.raises(abi.HeaderError) as e:
        abi.parse_prototypes(snippet, abi.STRUCTS)
    assert offending in str(e.value) and "ss_x" in str(e.value), (what, str(e.value))


def test_prototype_parser_reads_the_accepted_grammar():
    got = abi.parse_prototypes("int ss_x(const ss_wavenet* net, uint64_t seed, const uint64_t *seed_dev, float s, void* stream_);\n"
                               "int64_t ss_bytes(int B);\nconst char* ss_why(void);", abi.STRUCTS)
    x = got["ss_x"]
    assert x.launch and x.restype is ctypes.c_int
    assert [tuple(p) for p in x.params] == [("net", None, "ss_wavenet", True), ("seed", ctypes.c_uint64, None, False), ("seed_dev", None, "uint64_t", True),
                                            ("s", ctypes.c_float, None, False), ("stream_", None, "void", False)]
    assert not got["ss_bytes"].launch and got["ss_bytes"].restype is ctypes.c_int64
    assert got["ss_why"].params == () and got["ss_why"].restype is ctypes.c_char_p and not got["ss_why"].launch


def test_ops_holds_exactly_the_launch_prototypes():
    L.load()
    launch = {n for n, p in abi.PROTOTYPES.items() if p.launch}
    assert 0 < len(launch) < len(abi.PROTOTYPES)
    assert {n for n in vars(L.ops) if n.startswith("ss_")} == launch
    for n in sorted(set(abi.PROTOTYPES) - launch):
        with pytest.raises(AttributeError) as e:
            getattr(L.ops, n)
        assert n in str(e.value) and "load()" in str(e.value)
    with pytest.raises(AttributeError):
        L.ops.ss_no_such_function
    assert L.ops.ss_layernorm.__name__ == "ss_layernorm" and "const float* x" in L.ops.ss_layernorm.__doc__


class _Stub:
    """stands where the C function does: records what ctypes would have been handed"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __call__(self, *a):
        self.calls.append(a)
        return self.rc


@pytest.fixture
def no_stream(monkeypatch):
    """the stream L.ops supplies, without a device: a marker value, and a count of how often it was asked for"""
    asked = []
    monkeypatch.setattr(L, "stream_ptr", lambda: asked.append(1) or 0xABC0)
    return asked


def _op(name, rc=0):
    stub = _Stub(rc)
    return L._op(abi.PROTOTYPES[name], stub), stub


def test_marshalling_of_host_arrays_null_and_raw_addresses(no_stream):
    op, stub = _op("ss_layernorm")   # (const float* x, float* y, const float* gamma, const float* beta, 7 ints, float eps, const int32_t* lens, int mask_rows, stream)
    x = np.zeros(8, np.float32)
    lens = np.ones(1, np.int32)
    op(x, 0x1000, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, lens, 0)
    assert stub.calls == [(x.ctypes.data, 0x1000, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, lens.ctypes.data, 0, 0xABC0)] and no_stream == [1]
    for bad, word in ((np.zeros(8, np.float64), "float64"), (np.zeros(8, np.int32), "int32"), (np.zeros((4, 4), np.float32)[:, 1], "C-contiguous"),
                      (True, "bool"), (1.5, "float"), ("x", "str"), (b"x", "bytes"), ([x], "list"), (L.ConvGemmArgs(), "ss_conv_gemm_args")):
        with pytest.raises(TypeError) as e:
            op(bad, None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0)
        assert "ss_layernorm" in str(e.value) and "'x'" in str(e.value) and "float*" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(TypeError) as e:
        op(x, None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, np.ones(1, np.int64), 0)
    assert "'lens'" in str(e.value) and "int32_t*" in str(e.value) and "int64" in str(e.value)
    assert len(stub.calls) == 1 and no_stream == [1], "a refused call reaches neither the library nor the stream"


def test_arity_and_the_given_stream(no_stream):
    op, stub = _op("ss_layernorm")
    full = (None, None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0)
    op(*full, 0x5150)
    op(*full, None)   # an explicit NULL stream stays NULL
    assert [c[-1] for c in stub.calls] == [0x5150, None] and no_stream == [], "a full-length call supplies no stream of its own"
    op(*full)
    assert stub.calls[-1][-1] == 0xABC0 and no_stream == [1]
    for args in (full[:-1], full + (0x5150, 0), ()):
        with pytest.raises(TypeError) as e:
            op(*args)
        assert "int ss_layernorm(const float* x, float* y" in str(e.value) and f"{len(args)} given" in str(e.value)
    assert len(stub.calls) == 3


def test_struct_arguments_go_by_reference_and_only_as_their_own_type(no_stream):
    op, stub = _op("ss_conv_gemm")
    a = L.ConvGemmArgs()
    op(a)
    ref = stub.calls[0][0]
    assert ctypes.cast(ref, ctypes.c_void_p).value == ctypes.addressof(a)
    for bad in (L.GemmBf16Args(), L.Layer512Args(), np.zeros(100, np.float32), True):
        with pytest.raises(TypeError) as e:
            op(bad)
        assert "ss_conv_gemm:" in str(e.value) and "'args'" in str(e.value) and "ss_conv_gemm_args*" in str(e.value)
    op512, stub512 = _op("ss_layer512")
    with pytest.raises(TypeError):
        op512(a)
    assert len(stub.calls) == 1 and stub512.calls == []


def test_tensor_dtypes_by_pointee():
    """On a machine without a GPU a tensor of an accepted dtype gets as far as the device check; a wrong one is refused before it."""
    def address(t, pointee):
        return L._address(t, pointee, "ss_fn", "p")
    accepted = {"float": [torch.float32], "double": [torch.float64], "int32_t": [torch.int32], "int64_t": [torch.int64], "int16_t": [torch.int16],
                "uint8_t": [torch.uint8], "uint16_t": [torch.bfloat16, torch.float16, torch.int16, torch.uint16], "uint64_t": [torch.int64, torch.uint64]}
    every = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16, torch.uint16, torch.int32, torch.int64,
             torch.uint64, torch.bool]
    for pointee, ok in accepted.items():
        for dt in every:
            t = torch.zeros(4, dtype=dt)
            if dt in ok:
                with pytest.raises(L.StyleSingerHipError) as e:
                    address(t, pointee)
                assert "needs device tensors" in str(e.value) and "ss_fn" in str(e.value) and "'p'" in str(e.value)
            else:
                with pytest.raises(TypeError) as e:
                    address(t, pointee)
                assert "ss_fn" in str(e.value) and "'p'" in str(e.value) and f"{pointee}*" in str(e.value) and str(dt) in str(e.value)
    for dt in every:   # void*: any dtype, still a device tensor
        with pytest.raises(L.StyleSingerHipError):
            address(torch.zeros(4, dtype=dt), "void")
    assert issubclass(L.StyleSingerHipError, RuntimeError) and not issubclass(L.StyleSingerHipError, TypeError)
    # host arrays follow the same table
    for pointee, names in (("uint16_t", ("float16", "int16", "uint16")), ("uint64_t", ("int64", "uint64")), ("double", ("float64",)), ("uint8_t", ("uint8",))):
        for n in ("float16", "int16", "uint16", "int64", "uint64", "float64", "float32", "uint8", "int32"):
            a = np.zeros(4, n)
            if n in names:
                assert address(a, pointee) == a.ctypes.data
            else:
                with pytest.raises(TypeError):
                    address(a, pointee)
    assert address(np.zeros(4, np.complex64), "void") != 0
    assert address(b"gate16", "char") == b"gate16"
    with pytest.raises(TypeError):
        address(b"gate16", "uint8_t")
    with pytest.raises(L.StyleSingerHipError) as e:
        L.ptr(torch.zeros(4))
    assert "device tensors" in str(e.value) and L.ptr(None) is None


def test_a_real_entry_point_reports_its_own_refusal_under_its_symbol():
    """ss_layernorm refuses null arguments before it touches a device (test_host_cpu.py): through ops that is the library's message under the symbol."""
    x = np.zeros(8, np.float32)
    with pytest.raises(L.StyleSingerHipError) as e:
        L.ops.ss_layernorm(x, None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0, None)
    assert str(e.value).startswith("ss_layernorm failed (") and L.load().ss_last_error().decode() in str(e.value)
    with pytest.raises(TypeError) as e:
        L.ops.ss_layernorm(x.astype(np.float64), None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0, None)
    assert "ss_layernorm" in str(e.value) and "'x'" in str(e.value)
    with pytest.raises(TypeError):
        L.ops.ss_layernorm(torch.zeros(8, dtype=torch.float64), None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0, None)
    with pytest.raises(L.StyleSingerHipError) as e:
        L.ops.ss_layernorm(torch.zeros(8), None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0, None)
    assert "needs device tensors" in str(e.value)
    with pytest.raises(L.StyleSingerHipError) as e:
        L.ops.ss_layer512(L.Layer512Args(), None)
    assert "ss_layer512 failed" in str(e.value) and "null Hin" in str(e.value)


def test_struct_members_are_checked_without_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the struct setter needs no library")
    monkeypatch.setattr(L, "load", no_load)
    kw = dict(B=1, T=4, Cin=32, N=32, Np=32, Kp=32)
    with pytest.raises(TypeError) as e:
        L._fill_args(torch.zeros(4, 32, dtype=torch.float64), None, None, **kw)
    assert "ss_conv_gemm_args" in str(e.value) and "'A'" in str(e.value) and "float*" in str(e.value) and "torch.float64" in str(e.value)
    with pytest.raises(TypeError) as e:
        L._fill_args(None, None, None, lens=torch.zeros(1, dtype=torch.int64), **kw)
    assert "'lens'" in str(e.value)
    with pytest.raises(L.StyleSingerHipError) as e:
        L._fill_args(torch.zeros(4, 32), None, None, **kw)
    assert "needs device tensors" in str(e.value)
    with pytest.raises(TypeError) as e:
        L.gemm_bf16(torch.zeros(1, 4, 32), None, B=1, T=4, K=32, taps=(0,), N=32, Np=32, epi=L.HEPI_STORE)
    assert "ss_gemm_bf16_args" in str(e.value) and "'A'" in str(e.value) and "uint16_t*" in str(e.value) and "torch.float32" in str(e.value)
    with pytest.raises(TypeError) as e:
        L.layer512(torch.zeros(8), None, None, None, B=1, T=4, d=1)
    assert "ss_layer512_args" in str(e.value) and "'Hin'" in str(e.value)
    a = L._fill_args(0x1000, 0x2000, 0x3000, bias=np.zeros(32, np.float32), **kw)   # raw addresses and NULL go through untouched
    assert (a.A, a.W, a.C, a.lens, a.E) == (0x1000, 0x2000, 0x3000, None, None) and a.bias != 0
    n = L.WaveNet()
    assert L.member_address(n, "w_dil_h", None) is None and L.member_address(n, "w_dil", 0x40) == 0x40
    with pytest.raises(TypeError):
        L.member_address(n, "w_dil_h", torch.zeros(4))
    with pytest.raises(KeyError):
        L.member_address(n, "steps", None)   # not a pointer member
