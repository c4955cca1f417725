"""ctypes binding of libstylesinger_hip.so (the C-ABI in include/stylesinger_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol cannot be resolved this
module raises, and every op raises `StyleSingerHipError` on a non-zero status.  PyTorch is used only
for device memory (`tensor.data_ptr()`) and streams.

Two paths lead to the library. `ops.ss_x(...)`, one callable per prototype that ends in the stream (everything that launches):
tensors, host arrays and argument structs are passed as they are and checked against the pointee the header declares, so a
wrong dtype, a host tensor or a wrong argument count is an exception naming function and parameter BEFORE any launch; the
current stream is supplied when left out; a plain int is a raw address and the one explicit way to reinterpret memory.
`load().ss_x(...)` is raw ctypes, for the functions that answer queries and launch nothing (`_ok` / `_pick` rules,
`*_workspace_bytes`, `ss_set_tuning`, host tables), and for tests and tools that pin the raw ABI.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import abi
from .abi import declarations, declared_symbols  # noqa: F401  (part of this module's surface)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SS_LIB_PATH") or os.path.join(HERE, "libstylesinger_hip.so")  # SS_LIB_PATH: debug builds (tools/reproduce.sh trace-layer512)

# The C-ABI is read from the header by abi.py: constants, enumerators, struct layouts and prototypes. Nothing below restates it.
SS_MAX_TAPS, SS_MAX_LAYERS, SS_HG_MAX_UPS, SS_HG_MAX_KERNELS = (abi.DEFINES[n] for n in ("SS_MAX_TAPS", "SS_MAX_LAYERS", "SS_HG_MAX_UPS", "SS_HG_MAX_KERNELS"))
ABI_VERSION = abi.DEFINES["SS_ABI_VERSION"]
ALIGN_MAX_T, ALIGN_MAX_LC = abi.DEFINES["SS_ALIGN_MAX_T"], abi.DEFINES["SS_ALIGN_MAX_LC"]   # size caps of ss_contour_align (pitch.contour_align_device)
PITCH_EDIT_TILE, PITCH_EDIT_MAX_W = abi.DEFINES["SS_PITCH_EDIT_TILE"], abi.DEFINES["SS_PITCH_EDIT_MAX_W"]   # frames per workgroup / widest half-window of ss_pitch_edit
EPI_STORE, EPI_GATE, EPI_RESSKIP, EPI_DDPM = (abi.ENUMS["SS_EPI_" + n] for n in ("STORE", "GATE", "RESSKIP", "DDPM"))
ACT_NONE, ACT_RELU, ACT_GELU, ACT_MISH, ACT_TANH, ACT_LRELU = (abi.ENUMS[f"SS_ACT_{n}_"] for n in ("NONE", "RELU", "GELU", "MISH", "TANH", "LRELU"))
HEPI_STORE, HEPI_GATE, HEPI_RESX = (abi.ENUMS["SS_HEPI_" + n] for n in ("STORE", "GATE", "RESX"))

# the C structs in the positional order of ss_struct_sizes (csrc/api.hip), and the names their ctypes classes have here
_STRUCT_SIZES_ORDER = ("ss_conv_gemm_args", "ss_wavenet", "ss_hifigan", "ss_gemm_bf16_args", "ss_f0track_params", "ss_layer512_args")
ConvGemmArgs, WaveNet, HifiGan, GemmBf16Args, F0TrackParams, Layer512Args = (abi.STRUCTURES[n] for n in _STRUCT_SIZES_ORDER)


class StyleSingerHipError(RuntimeError):
    pass


_lib = None


def load():
    """Load the shared library (once). Raises if it is missing: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StyleSingerHipError(
            f"{LIB_PATH} not found: build it with `python -m stylesinger_amd.build` (hipcc, gfx950). "
            "The StyleSinger HIP path has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in declarations().items():
        if not hasattr(lib, name):
            raise StyleSingerHipError(f"libstylesinger_hip.so does not export {name}")
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.ss_abi_version() != ABI_VERSION:
        raise StyleSingerHipError(f"libstylesinger_hip.so has ABI {lib.ss_abi_version()}, this binding expects {ABI_VERSION}: rebuild it")
    sizes = (C.c_int64 * len(_STRUCT_SIZES_ORDER))()
    if lib.ss_struct_sizes(sizes, len(sizes)) != 0:
        raise StyleSingerHipError("ss_struct_sizes failed")
    for name, c_size in zip(_STRUCT_SIZES_ORDER, sizes):
        if C.sizeof(abi.STRUCTURES[name]) != c_size:
            raise StyleSingerHipError(f"{name}: {C.sizeof(abi.STRUCTURES[name])} bytes as read from include/stylesinger_hip.h, {c_size} in libstylesinger_hip.so: rebuild it")
    _lib = lib
    for name, proto in abi.PROTOTYPES.items():
        if proto.launch:
            setattr(ops, name, _op(proto))
    for env, key in (("SS_GATE16", b"gate16"), ("SS_GATE16_KS", b"gate16_ks"), ("SS_GATE256", b"gate256"), ("SS_MEL_TAIL", b"mel_tail"), ("SS_GATE128", b"gate128"),
                     ("SS_Q4_FORCE", b"q4_force"), ("SS_SKIP_DENSE", b"skip_dense"), ("SS_LAYER512", b"layer512"), ("SS_LAYER512_TAIL", b"layer512_tail")):
        val = os.environ.get(env)
        if val is not None:   # validated by the library; an out-of-range value is an error, not a silent different tile
            check(lib.ss_set_tuning(key, int(val)), f"ss_set_tuning({env}={val})")
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().ss_last_error().decode(errors="replace")
        raise StyleSingerHipError(f"{what} failed ({rc}): {msg}")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a torch tensor (or None) as a plain int."""
    if t is None:
        return None
    if not t.is_cuda:
        raise StyleSingerHipError("HIP path needs device tensors")
    return t.data_ptr()


def hptr(a):
    """Host pointer of a contiguous numpy array."""
    return a.ctypes.data


# ---------------------------------------------------------------------------------------------
# checked marshalling: what a pointer of the header may be handed (ops.* and the pointer members of the argument structs)
# ---------------------------------------------------------------------------------------------
_ANY = None   # void*: every dtype
_TORCH_DTYPES = {"float": {torch.float32}, "double": {torch.float64}, "int32_t": {torch.int32}, "int": {torch.int32}, "int64_t": {torch.int64},
                 "int16_t": {torch.int16}, "uint8_t": {torch.uint8}, "char": {torch.uint8, torch.int8},
                 "uint16_t": {torch.bfloat16, torch.float16, torch.int16, torch.uint16},
                 "uint64_t": {torch.int64, torch.uint64},   # the plans' `seed` word is int64
                 "void": _ANY}
_NUMPY_DTYPES = {k: v if v is _ANY else {str(d).split(".")[1] for d in v} for k, v in _TORCH_DTYPES.items()}
_Tensor = torch.Tensor


def _refuse(fn, param, pointee, got):
    return TypeError(f"{fn}: parameter '{param}' is a `{pointee}*` and cannot take {got}")


def _address(a, pointee, fn, param):
    """What ctypes is handed for the `pointee*` parameter (or struct member) `param` of `fn`; everything the pointee rules out raises here."""
    if a is None or type(a) is int:   # NULL; a raw address (address arithmetic, deliberate reinterpretation) goes through untouched
        return a
    if type(a) is _Tensor or isinstance(a, _Tensor):
        ok = _TORCH_DTYPES.get(pointee, ())
        if ok is not _ANY and a.dtype not in ok:
            raise _refuse(fn, param, pointee, f"a {a.dtype} tensor")
        if not a.is_cuda:
            raise StyleSingerHipError(f"{fn}: parameter '{param}' needs device tensors")
        return a.data_ptr()
    if isinstance(a, np.ndarray):   # a host pointer
        ok = _NUMPY_DTYPES.get(pointee, ())
        if ok is not _ANY and a.dtype.name not in ok:
            raise _refuse(fn, param, pointee, f"a {a.dtype.name} array")
        if not a.flags.c_contiguous:
            raise _refuse(fn, param, pointee, "an array that is not C-contiguous")
        return a.ctypes.data
    if isinstance(a, C.Structure):
        if type(a) is not abi.STRUCTURES.get(pointee):
            raise _refuse(fn, param, pointee, f"a {type(a).__name__} struct")
        return C.byref(a)
    if type(a) is bytes and pointee == "char":
        return a
    raise _refuse(fn, param, pointee, f"{type(a).__name__} {a!r}")


def member_address(struct, field, v):
    """The checked address of tensor `v` for pointer member `field` of the ctypes struct `struct` (the caller keeps `v` alive)."""
    name = type(struct).__name__
    return _address(v, abi.STRUCT_POINTEES[name][field], name, field)


def set_members(struct, **members):
    """struct.field = tensor | None | raw address for pointer members, each checked against the member's declaration in the header."""
    for field, v in members.items():
        setattr(struct, field, member_address(struct, field, v))


def _op(proto, fn=None):
    """The checked callable of one launch prototype: pointers marshalled by _address, the stream supplied where it is left out, status raised.
    The entry point is looked up on load() at every call, like every other use of the library (fn: a stand-in, for tests)."""
    name, n = proto.name, len(proto.params)
    pointers = tuple((i, p.pointee, p.name) for i, p in enumerate(proto.params) if p.pointee)

    def op(*args):
        if not n - 1 <= len(args) <= n:
            raise TypeError(f"{name} takes {n - 1} arguments and, optionally, the stream ({len(args)} given): {proto.text}")
        a = list(args)
        if len(a) < n:   # None holds the stream's place until every other argument has passed
            a.append(None)
        for i, pointee, param in pointers:
            v = a[i]
            if v is not None:
                a[i] = _address(v, pointee, name, param)
        if len(args) < n:
            a[-1] = stream_ptr()
        rc = (fn or getattr(load(), name))(*a)
        if rc != 0:
            raise StyleSingerHipError(f"{name} failed ({rc}): {load().ss_last_error().decode(errors='replace')}")
    op.__name__ = op.__qualname__ = name
    op.__doc__ = proto.text
    return op


class _Ops:
    """One checked callable per prototype that ends in the stream; filled by load()."""

    def __getattr__(self, name):   # reached only for what load() has not put here
        if _lib is None:
            load()
            return getattr(self, name)
        if name in abi.PROTOTYPES:
            raise AttributeError(f"{name} takes no stream, so it launches nothing and is not in ops: call it as load().{name}(...)")
        raise AttributeError(f"include/stylesinger_hip.h declares no {name}")


ops = _Ops()


def round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------
# thin op wrappers (defaults and argument structs; the marshalling is ops' and set_members')
# ---------------------------------------------------------------------------------------------
def conv_gemm(A, W, out, **kw):
    a = _fill_args(A, W, out, **kw)
    ops.ss_conv_gemm(a)


def _fill_args(A, W, out, *, B, T, Cin, N, Np, Kp, lda=None, a_bs=None, taps=(0,), lens=None, a_bias=None, a_scale=1.0,
               a_lrelu=1.0, epi=EPI_STORE, bias=None, pre_scale=1.0, act=ACT_NONE, act_slope=0.0, E=None, lde=0, e_bs=0,
               gate_mode=0, R=None, ldr=0, r_bs=None, post_scale=1.0, accumulate=False, mask_rows=True, ldc=None, c_bs=None,
               C2=None, ldc2=0, c2_bs=0, Nh=0, tile=0, group_size=0, w_gs=0, bias_gs=0, a_bias_gs=0, bf16=False, e_tiled=False):
    a = ConvGemmArgs()
    set_members(a, A=A, lens=lens, a_bias=a_bias, W=W, bias=bias, E=E, R=R, C=out, C2=C2)
    a.lda = lda if lda is not None else Cin
    a.a_batch_stride = a_bs if a_bs is not None else T * a.lda
    a.Cin = Cin; a.ntaps = len(taps)
    for i, o in enumerate(taps):
        a.tap_off[i] = int(o)
    a.B = B; a.T = T; a.a_scale = a_scale; a.a_lrelu = a_lrelu
    a.N = N; a.Np = Np; a.Kp = Kp
    a.epi = epi; a.pre_scale = pre_scale; a.act = act; a.act_slope = act_slope
    a.lde = lde; a.e_batch_stride = e_bs; a.gate_mode = gate_mode
    a.ldr = ldr; a.r_batch_stride = r_bs if r_bs is not None else T * ldr
    a.post_scale = post_scale; a.accumulate = int(accumulate); a.mask_rows = int(mask_rows)
    a.ldc = ldc if ldc is not None else N
    a.c_batch_stride = c_bs if c_bs is not None else T * a.ldc
    a.ldc2 = ldc2; a.c2_batch_stride = c2_bs; a.Nh = Nh; a.tile = tile
    a.group_size = group_size; a.w_group_stride = w_gs; a.bias_group_stride = bias_gs; a.a_bias_group_stride = a_bias_gs
    a.mfma_bf16 = 1 if bf16 else 0
    a.e_tiled = 1 if e_tiled else 0
    return a


def gate16_tile_addend(E, *, B, T, Np, lde, e_bs, dilation, mt):
    """E (this layer's Np packed columns, row stride lde) -> the addend in the 16x16x4 gate kernel's fetch order (ss_gate16_tile_addend)."""
    n = load().ss_gate16_tiled_floats(B, T, Np, int(dilation), int(mt))
    out = torch.empty(n, device=E.device, dtype=torch.float32)
    ops.ss_gate16_tile_addend(E, lde, e_bs, out, B, T, Np, int(dilation), int(mt))
    return out


def wino_gate(A, Wt, out, *, dilation, **kw):
    """Winograd F(2,3) dilated conv + gate (ss_wino_gate); Wt = packed transformed weights (4 'taps')."""
    kw.setdefault("epi", EPI_GATE)
    a = _fill_args(A, Wt, out, **kw)
    ops.ss_wino_gate(a, int(dilation))


def wino43_gate(A, Wt, out, *, dilation, **kw):
    """Winograd F(4,3) dilated conv + gate (ss_wino43_gate); Wt = packed transformed weights (6 'taps')."""
    kw.setdefault("epi", EPI_GATE)
    a = _fill_args(A, Wt, out, **kw)
    ops.ss_wino43_gate(a, int(dilation))


def pack_gemm16_weights(Wp, Kp):
    """packed weight rows [Np][Kp] (Np % 64 == 0) -> the same floats in the fetch order of ss_gemm16_res (ss_pack_gemm16_weights)."""
    Wp = Wp.contiguous().float()
    out = torch.empty_like(Wp)
    ops.ss_pack_gemm16_weights(Wp, out, Wp.shape[0], Kp)
    return out


def pack_gate16_weights(Wp, Kp):
    """packed F(4,3) weights [Np][6 * Kp] -> the same floats in the fetch order of the 16x16x4 gate kernel (ss_pack_gate16_weights)."""
    Wp = Wp.contiguous().float()
    out = torch.empty_like(Wp)
    ops.ss_pack_gate16_weights(Wp, out, Wp.shape[0], Kp)
    return out


def wino43_gate16(A, Wt, out, *, dilation, mt=0, W16=None, **kw):
    """The F(4,3) gate on 16x16x4 MFMA tiles (ss_wino43_gate16); mt = 0 lets the library pick, 1 / 2 / 3 force the row-tile count (16 * mt
    quads per workgroup). mt = 1 exists only in the K-staged form: it needs Kp >= 64 and the gate16_ks knob on, and is refused otherwise.
    W16 = pack_gate16_weights(Wt): the weights in the kernel's fetch order (ss_wino43_gate16w). e_tiled=True (E from gate16_tile_addend
    with the same dilation and mt) needs an explicit mt."""
    kw.setdefault("epi", EPI_GATE)
    a = _fill_args(A, Wt, out, **kw)
    if W16 is not None:
        ops.ss_wino43_gate16w(a, W16, int(dilation), int(mt))
        return
    ops.ss_wino43_gate16(a, int(dilation), int(mt))


def gemm16_res(A, W, out, *, mt=0, W16=None, **kw):
    """Residual projection C = (R + A.W^T + bias) * post_scale on 16x16x4 tiles (ss_gemm16_res); same keyword arguments as conv_gemm.
    mt = 0 lets the library pick, 2 / 4 / 6 / 8 force 16 * mt rows per workgroup (the 32-row tile, mt = 2, exists for this kernel only).
    W16 = pack_gemm16_weights(first N rows of W): the weights in the kernel's fetch order (ss_gemm16_resw; N % 64 == 0)."""
    a = _fill_args(A, W, out, **kw)
    if W16 is not None:
        ops.ss_gemm16_resw(a, W16, int(mt))
        return
    ops.ss_gemm16_res(a, int(mt))


def gemm16_store(A, W, out, *, mt=0, **kw):
    """C = act(A.W^T + bias) on 16x16x4 tiles with both operands streamed by LDS-DMA (ss_gemm16_store)."""
    a = _fill_args(A, W, out, **kw)
    ops.ss_gemm16_store(a, int(mt))


def gemm16_store_splitk(A, W, out, *, ksplit, mt=0, **kw):
    """ss_gemm16_store_splitk: the long-K GEMM with K split over `ksplit` workgroup slices + a fixed-order reduction (small launches)."""
    a = _fill_args(A, W, out, **kw)
    part = torch.empty(max(1, ksplit) * a.B * a.T * a.N, device=out.device, dtype=torch.float32)
    ops.ss_gemm16_store_splitk(a, int(mt), int(ksplit), part)


def wino43_weight(w):
    """conv weight [Cout][Cin][3] (device) -> F(4,3)-transformed [Cout][Cin][6]."""
    w = w.contiguous().float()
    out = torch.empty(w.shape[0], w.shape[1], 6, device=w.device, dtype=torch.float32)
    ops.ss_wino43_weight_transform(w, out, w.shape[0], w.shape[1])
    return out


def wino43_group_weight(w):
    """conv weight [Cout][Cin][k] (device, k odd) -> [Cout][Cin][6 * ceil(k/3)]: the taps in groups of three (zero padded), every group
    F(4,3)-transformed - the B operand of ss_wino43_conv after ss_pack_conv_weight."""
    w = w.contiguous().float()
    Cout, Cin, k = w.shape
    G = (k + 2) // 3
    wp = torch.zeros(Cout, Cin, 3 * G, device=w.device, dtype=torch.float32)
    wp[..., :k] = w
    return torch.cat([wino43_weight(wp[..., 3 * g:3 * g + 3]) for g in range(G)], dim=-1).contiguous()


def wino43_conv(A, W, out, *, k, dilation, **kw):
    """Grouped Winograd F(4,3) conv (ss_wino43_conv); keyword arguments as conv_gemm (taps are implied by k and dilation)."""
    taps = [(j - (k - 1) // 2) * dilation for j in range(k)]
    a = _fill_args(A, W, out, taps=taps, **kw)
    ops.ss_wino43_conv(a, k, dilation)
    return out


# F(4,4) on the points {0, 1, -1, 2, -2, 1/2, inf}: the 7 x 4 filter matrix (row j = p_j^i / prod_{l != j} (p_j - p_l); last row = the point at
# infinity). Its partners are the input transform of csrc/wino44_conv.hip and the power-of-two output transform in its header comment.
WINO44_G = (
    (-1 / 2, 0.0, 0.0, 0.0),
    (-1 / 3, -1 / 3, -1 / 3, -1 / 3),
    (1 / 9, -1 / 9, 1 / 9, -1 / 9),
    (1 / 36, 1 / 18, 1 / 9, 2 / 9),
    (-1 / 60, 1 / 30, -1 / 15, 2 / 15),
    (32 / 45, 16 / 45, 8 / 45, 4 / 45),
    (0.0, 0.0, 0.0, 1.0),
)


def wino44_conv_ok(C, k, dilation):
    """1 where the square ResBlock conv (C, k, dilation) runs as F(4,4) tap groups (ss_wino44_conv_ok): the one rule of pack and forward."""
    return int(load().ss_wino44_conv_ok(int(C), int(k), int(dilation)))


def wino44_group_weight(w):
    """conv weight [Cout][Cin][k] (device) -> [Cout][Cin][7 * ceil(k/4)]: the taps in groups of four (zero padded at the end), every group
    F(4,4)-transformed in float64 and rounded once - the B operand of ss_wino44_conv after ss_pack_conv_weight."""
    Cout, Cin, k = w.shape
    G = (k + 3) // 4
    wp = torch.zeros(Cout, Cin, G, 4, device=w.device, dtype=torch.float64)
    wp.view(Cout, Cin, 4 * G)[..., :k] = w.double()
    g = torch.tensor(WINO44_G, device=w.device, dtype=torch.float64)
    return torch.einsum("jt,oigt->oigj", g, wp).reshape(Cout, Cin, 7 * G).float().contiguous()


def wino44_conv(A, W, out, *, k, dilation, **kw):
    """Grouped Winograd F(4,4) conv (ss_wino44_conv, k = 7 | 11); keyword arguments as conv_gemm (taps are implied by k and dilation)."""
    taps = [(j - (k - 1) // 2) * dilation for j in range(k)]
    a = _fill_args(A, W, out, taps=taps, **kw)
    ops.ss_wino44_conv(a, k, dilation)
    return out


def split3_weights(Wp, Kp):
    """packed F(4,3) weights [Np][6 * Kp] fp32 -> Np * 18 * Kp bf16: every element as its three bf16 terms, in the fetch order of
    ss_wino43_gate16x ([n tile][wave][K chunk][component][plane][lane][8])."""
    Wp = Wp.contiguous().float()
    Np = Wp.shape[0]
    out = torch.empty(Np, 3 * Wp.shape[1], device=Wp.device, dtype=torch.bfloat16)
    ops.ss_split3_weights(Wp, out, Np, Kp)
    return out


def split3_gemm16_weights(Wp, Kp):
    """packed weight rows [Np][Kp] fp32 -> their three bf16 terms in the fetch order of ss_gemm16x_store."""
    Wp = Wp.contiguous().float()
    Np = Wp.shape[0]
    out = torch.empty(int(load().ss_split3_gemm16_elems(Np, Kp)), device=Wp.device, dtype=torch.bfloat16)
    ops.ss_split3_gemm16_weights(Wp, out, Np, Kp)
    return out


def gemm16x_store(A, W, Wx, out, *, mt=0, **kw):
    """bf16x3 form of gemm16_store (ss_gemm16x_store); W only supplies Np / Kp for the argument struct."""
    a = _fill_args(A, W, out, **kw)
    ops.ss_gemm16x_store(a, Wx, int(mt))


def wino43_gate16x(A, Wx, out, *, dilation, mt=0, **kw):
    """bf16x3 form of the F(4,3) gate (ss_wino43_gate16x); Wx = split3_weights(packed F(4,3) weight); keyword arguments as wino43_gate16
    (w_gs, if given, in bf16 elements)."""
    kw.setdefault("epi", EPI_GATE)
    a = _fill_args(A, ptr(Wx), out, **kw)   # the bf16 terms also stand in the struct's `const float* W`, as before: reinterpreted on purpose, so by address
    ops.ss_wino43_gate16x(a, Wx, dilation, mt)
    return out


def wino_weight(w):
    """conv weight [Cout][Cin][3] (device) -> transformed [Cout][Cin][4]."""
    w = w.contiguous().float()
    out = torch.empty(w.shape[0], w.shape[1], 4, device=w.device, dtype=torch.float32)
    ops.ss_wino_weight_transform(w, out, w.shape[0], w.shape[1])
    return out


def pack_conv_weight(w, *, scale0=None, interleave_half=0, row_scale=1.0):
    """torch conv/linear weight [Cout, Cin(, k)] (device) -> packed [Np][k*Kp] device tensor."""
    if w.dim() == 2:
        w = w[:, :, None]
    w = w.contiguous().float()
    Cout, Cin, k = w.shape
    Kp = round_up(Cin, 32)
    Np = 2 * round_up(interleave_half, 32) if interleave_half else round_up(Cout, 32)
    dst = torch.empty(Np, k * Kp, device=w.device, dtype=torch.float32)
    ops.ss_pack_conv_weight(w, scale0, dst, Cout, Cin, k, Np, Kp, interleave_half, float(row_scale))
    return dst


def weight_norm_scale(v, g):
    v = v.contiguous().float()
    g = g.contiguous().float().reshape(-1)
    rows = v.shape[0]
    out = torch.empty(rows, device=v.device, dtype=torch.float32)
    ops.ss_weight_norm_scale(v, g, out, rows, v.numel() // rows)
    return out


def pack_convtr_weight(w, scale0, u, group):
    w = w.contiguous().float()
    Cin, Cout, k = w.shape
    pad = (k - u) // 2
    nph = (u - pad) if group == 0 else pad
    Np = round_up(nph * Cout, 32)
    Kp = round_up(Cin, 32)
    dst = torch.empty(Np, 2 * Kp, device=w.device, dtype=torch.float32)
    ops.ss_pack_convtr_weight(w, scale0, dst, Cin, Cout, k, u, group, Np, Kp)
    return dst


def pack_bias(b, *, b2=None, Np=None, interleave_half=0, repeat=1):
    b = b.contiguous().float()
    n = b.numel()
    if Np is None:
        Np = 2 * round_up(interleave_half, 32) if interleave_half else round_up(n * repeat, 32)
    dst = torch.empty(Np, device=b.device, dtype=torch.float32)
    ops.ss_pack_bias(b, b2, dst, n, Np, interleave_half, repeat)
    return dst


def to_bf16(x, bias=None, lens=None):
    """fp32 device tensor [..., C] -> bf16 bits (torch.bfloat16 tensor, RNE) through ss_to_bf16 (B*T rows)."""
    x = x.contiguous().float()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    ops.ss_to_bf16(x, bias, y, 1, rows, Cc, Cc, Cc, lens, 0, 0)
    return y


def split_bf16(x, bias=None, lens=None):
    """fp32 device tensor [..., C] -> [..., 2C] bf16 bits, pairs interleaved by 32: per 32-channel chunk the 32 hi = RNE(v) terms, then the 32
    mid = RNE(v - hi) terms (ss_split_bf16; the operand layout of ss_gemm_bf16_args.split)."""
    x = x.contiguous().float()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty(tuple(x.shape[:-1]) + (2 * Cc,), device=x.device, dtype=torch.bfloat16)
    ops.ss_split_bf16(x, bias, y, 1, rows, Cc, Cc, 2 * Cc, lens, 0, 0)
    return y


def split_f16(x, bias=None, lens=None, scale=1.0):
    """fp32 device tensor [..., C] -> [..., 2C] fp16 bits in the same pairs-interleaved-by-32 layout: hi = RNE16(v), lo = RNE16(v - hi) of
    v = (x + bias) * scale (ss_split_f16; the operand layout of ss_gemm_bf16_args.split = 2, scale = the weights' power-of-two shift)."""
    x = x.contiguous().float()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty(tuple(x.shape[:-1]) + (2 * Cc,), device=x.device, dtype=torch.float16)
    ops.ss_split_f16(x, bias, float(scale), y, 1, rows, Cc, Cc, 2 * Cc, lens, 0, 0)
    return y


_FP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def fp4_rne(v):
    """|v| <= 6 (float tensor) -> (code 0..7, value) of the nearest e2m1 magnitude, ties to the even mantissa (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
    1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4): what v_cvt_scalef32_pk_fp4_f16 does (profiles/r04_ubench_cvt_fp4_probe.log)."""
    grid = torch.tensor(_FP4_GRID, device=v.device, dtype=v.dtype)
    mid = (grid[1:] + grid[:-1]) / 2
    a = v.abs().clamp(max=6.0).contiguous()
    idx = torch.bucketize(a, mid) + ((a == 0.75) | (a == 1.75) | (a == 3.5)).long()
    return idx, grid[idx]


def gate128q_kindex():
    """[12 pairs][2 lane halves][32 elements] -> K index (tap * 256 + channel): the element order of the fp16q4 gate's block-scaled second
    product (csrc/gate128_layout.h, g128q::q_kindex - the same function the kernel's layout is checked against)."""
    out = (C.c_int32 * 768)()
    n = load().ss_gate128q_kindex(out, 768)
    if n != 768:
        raise StyleSingerHipError("ss_gate128q_kindex: " + load().ss_last_error().decode(errors="replace"))
    return torch.tensor(list(out), dtype=torch.long).view(12, 2, 32)


def tile256q_kindex(n_pairs):
    """[n_pairs][2][32] -> K index: the element order of the fp16q4 skip GEMM's block-scaled second product (csrc/gate128_layout.h t128q_kindex)."""
    out = (C.c_int32 * (n_pairs * 64))()
    if load().ss_tile256q_kindex(out, n_pairs) != n_pairs * 64:
        raise StyleSingerHipError("ss_tile256q_kindex: " + load().ss_last_error().decode(errors="replace"))
    return torch.tensor(list(out), dtype=torch.long).view(n_pairs, 2, 32)


def _pack_q4(Wp, tab, odd_lines, shift):
    """shared by pack_gate_q4 / pack_skip_q4: the ss_split_f16 pack of w * 2^shift with its lo plane replaced by block-scaled fp4 terms; tab
    [pairs][2][32] = K index of every element, odd_lines [pairs] = the 64-element weight line that carries pair p's terms"""
    Np, K = Wp.shape
    nl = K // 32
    dev = Wp.device
    ws = Wp.float() * float(2 ** shift)
    if Wp.is_cuda:
        pack = split_f16(Wp, scale=float(2 ** shift))
    else:   # host form of ss_split_f16 (pairs interleaved by 32), so that the packer can be checked without a GPU
        hi = ws.half()
        lo16 = (ws - hi.float()).half()
        pack = torch.stack([hi.view(Np, nl, 32), lo16.view(Np, nl, 32)], dim=2).reshape(Np, 2 * K).contiguous()
    lo = ws - ws.half().float()
    npairs = tab.shape[0]
    tab = tab.to(dev)
    blocks = lo[:, tab.reshape(-1)].view(Np, npairs, 2, 32)
    amax = blocks.abs().amax(dim=-1, keepdim=True)
    e = torch.floor(torch.log2(amax.clamp_min(2.0 ** -120))) - 2      # the block's largest element lands in [4, 8): the grid's top is 6
    e = torch.where(amax > 0, e, torch.full_like(e, -120.0))
    scale = torch.exp2(e)
    idx, mag = fp4_rne(blocks / scale)
    code = idx | ((blocks < 0).long() << 3)
    nib = code.view(Np, npairs, 2, 16, 2)
    qbytes = (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8)       # element e in nibble e & 1 of byte e >> 1
    sbyte = (e.squeeze(-1) + 127).clamp(0, 254).to(torch.uint8)       # [Np][pairs][2]
    wb = pack.view(torch.uint8).view(Np, nl, 128)
    wb[:, :, 64:] = 0                                                 # nothing in the second half of any line ...
    line = torch.as_tensor(odd_lines, device=dev, dtype=torch.long)   # ... except the line that closes every pair
    for h in range(2):
        wb[:, line, 64 + 16 * h:64 + 16 * h + 16] = qbytes[:, :, h]
        wb[:, line, 96 + h] = sbyte[:, :, h]
    lo_q = torch.zeros_like(lo)
    lo_q[:, tab.reshape(-1)] = (mag * torch.sign(blocks) * scale).view(Np, -1)
    return pack, lo_q


def pack_skip_q4(Wp, *, shift=8):
    """Packed fp32 1-tap weight [Np][K] (K a multiple of 64) -> the operand of ss_gemm_bf16_tile256q (split = 3): as pack_gate_q4, pairs =
    consecutive 32-channel chunks, the pair's fp4 terms in the line of its odd chunk. Returns (pack [Np][2 K] fp16 bits, lo_q [Np][K] fp32)."""
    Np, K = Wp.shape
    assert K % 64 == 0
    return _pack_q4(Wp, tile256q_kindex(K // 64), [2 * p + 1 for p in range(K // 64)], shift)


def pack_gate_q4(Wp, *, shift=8):
    """Packed fp32 gate weight [Np][3 * 256] (ss_pack_conv_weight, gate-interleaved rows, tap-major) -> the operand of ss_gemm_bf16_gate128q
    (ss_gemm_bf16_args.split = 3): the ss_split_f16 pack of w * 2^shift whose LO plane is replaced by the fp4 (e2m1) terms of
    lo = w * 2^shift - fp16(w * 2^shift) in the kernel's lane order with one E8M0 scale per 32-element block (block = lane half h of step pair p).
    Returns (pack [Np][2 * 768] fp16 bits, lo_q [Np][768] fp32 = the values the matrix cores will see for lo, in K order - for references)."""
    Np, K3 = Wp.shape
    assert K3 == 768, "the fp16q4 gate is built for K = 256, three taps"
    S_odd = [2 * p + 1 for p in range(12)]
    return _pack_q4(Wp, gate128q_kindex(), [(S % 3) * 8 + S // 3 for S in S_odd], shift)   # g128q::step_line of the pair's odd step


def unpack_skip_q4(pack):
    """the ss_gemm_bf16_tile256q view of a pack_skip_q4 pack: (hi [Np][K], lo_q [Np][K]) in K order"""
    Np, K = pack.shape[0], pack.shape[1] // 2
    nl = K // 32
    wb = pack.contiguous().view(torch.uint8).view(Np, nl, 128)
    hi = pack.view(Np, nl, 64)[:, :, :32].float().reshape(Np, K)
    tab = tile256q_kindex(K // 64).to(pack.device)
    grid = torch.tensor(_FP4_GRID, device=pack.device)
    lo_q = torch.zeros(Np, K, device=pack.device)
    for p in range(K // 64):
        for h in range(2):
            by = wb[:, 2 * p + 1, 64 + 16 * h:64 + 16 * h + 16].long()
            nib = torch.stack([by & 15, by >> 4], dim=-1).reshape(Np, 32)
            lo_q[:, tab[p, h]] = grid[nib & 7] * torch.where((nib & 8) != 0, -1.0, 1.0) * torch.exp2(wb[:, 2 * p + 1, 96 + h].float() - 127.0).unsqueeze(-1)
    return hi, lo_q


def unpack_gate_q4(pack):
    """What ss_gemm_bf16_gate128q reads from a pack_gate_q4 pack, decoded the way the kernel addresses it (csrc/gate128_layout.h): for packed
    column n, step pair p, lane half h the 16 bytes at logical slot 4 + h of the weight line of step 2 p + 1 are 32 e2m1 nibbles (element e in
    nibble e & 1 of byte e >> 1), byte h of slot 6 their E8M0 scale. Returns (hi [Np][768] fp32 in K order, lo_q [Np][768] fp32 in K order)."""
    Np = pack.shape[0]
    wb = pack.contiguous().view(torch.uint8).view(Np, 24, 128)
    hi = pack.view(Np, 24, 64)[:, :, :32].float().reshape(Np, 768)
    tab = gate128q_kindex().to(pack.device)
    grid = torch.tensor(_FP4_GRID, device=pack.device)
    lo_q = torch.zeros(Np, 768, device=pack.device)
    for p in range(12):
        S = 2 * p + 1
        line = (S % 3) * 8 + S // 3
        for h in range(2):
            by = wb[:, line, 64 + 16 * h:64 + 16 * h + 16].long()                  # [Np][16]
            nib = torch.stack([by & 15, by >> 4], dim=-1).reshape(Np, 32)             # element e = 2 * byte + nibble
            val = grid[nib & 7] * torch.where((nib & 8) != 0, -1.0, 1.0) * torch.exp2(wb[:, line, 96 + h].float() - 127.0).unsqueeze(-1)
            lo_q[:, tab[p, h]] = val
    return hi, lo_q


def split_planes(y):
    """[..., 2C] pairs-interleaved-by-32 bf16 / fp16 -> (hi [..., C], mid [..., C]) as float (host-side view for tests / debugging)."""
    v = y.float().reshape(*y.shape[:-1], y.shape[-1] // 64, 2, 32)
    return v[..., 0, :].reshape(*y.shape[:-1], -1), v[..., 1, :].reshape(*y.shape[:-1], -1)


def gemm_bf16(A, Wh, *, B, T, K, taps, N, Np, epi, lens=None, bias=None, act=ACT_NONE, E=None, lde=0, e_bs=None, X=None, post_scale=1.0,
              next_bias=None, Y=None, out=None, ldc=None, c_bs=None, lda=None, a_bs=None, mask_rows=True, gate_mode=0, gate256=False,
              split=0, cur_bias=None, out_scale=1.0, q_scale=0.0, one_product=False, a_compact=False, group_size=0, w_gs=0, bias_gs=0, next_bias_gs=0,
              cur_bias_gs=0):
    """ss_gemm_bf16: A, Wh = bf16 device tensors (A [B,T,lda], Wh packed [Np][len(taps)*K]); see include/stylesinger_hip.h."""
    a = GemmBf16Args()
    set_members(a, A=A, lens=lens, W=Wh, bias=bias, E=E, X=X, next_bias=next_bias, Y=Y, C=out, cur_bias=cur_bias)
    a.lda = lda if lda is not None else A.shape[-1]
    a.a_batch_stride = a_bs if a_bs is not None else T * a.lda
    a.K = K; a.ntaps = len(taps)
    for i, o in enumerate(taps):
        a.tap_off[i] = int(o)
    a.B = B; a.T = T; a.N = N; a.Np = Np; a.epi = epi; a.act = act
    a.lde = lde; a.e_batch_stride = e_bs if e_bs is not None else T * lde; a.gate_mode = gate_mode
    if X is not None:
        a.ldx = X.shape[-1]; a.x_batch_stride = T * a.ldx
    a.post_scale = post_scale
    if Y is not None:
        a.ldy = Y.shape[-1]; a.y_batch_stride = T * a.ldy
    a.ldc = ldc if ldc is not None else (out.shape[-1] if out is not None else 0)
    a.c_batch_stride = c_bs if c_bs is not None else T * a.ldc
    a.mask_rows = int(mask_rows)
    a.split = split
    a.out_scale = out_scale
    a.q_scale = q_scale
    a.one_product = int(one_product)
    a.a_compact = int(a_compact)
    a.group_size = group_size; a.w_group_stride = w_gs; a.bias_group_stride = bias_gs
    a.next_bias_group_stride = next_bias_gs; a.cur_bias_group_stride = cur_bias_gs
    if gate256 and epi == HEPI_STORE and split == 3:   # the fp16q4 skip GEMM
        ops.ss_gemm_bf16_tile256q(a)
        return
    if gate256 == 128 and epi == HEPI_GATE and split == 3:   # ... with the second product on the block-scaled fp4 instruction
        ops.ss_gemm_bf16_gate128q(a)
        return
    if gate256 == 128 and epi == HEPI_GATE:   # the fp16x2 gate on 256 x 128 tiles, two workgroups per CU
        ops.ss_gemm_bf16_gate128(a)
        return
    if gate256:   # the 256-row LDS-DMA kernels directly (ss_gemm_bf16 picks them by itself for many-round launches)
        if epi == HEPI_GATE:
            ops.ss_gemm_bf16_gate256(a)
        else:
            ops.ss_gemm_bf16_tile256(a)
        return
    ops.ss_gemm_bf16(a)


def layer512_pack_gate(w_pairs, n_products=2):
    """ss_split_f16 pack [512][3*256*2] of the gate-interleaved dilated-conv weights -> the fragment order ss_layer512 streams (fp16 [786432];
    n_products = 1: the hi terms only, [393216])."""
    assert w_pairs.dtype == torch.float16 and tuple(w_pairs.shape) == (512, 3 * 256 * 2) and w_pairs.is_contiguous(), tuple(w_pairs.shape)
    out = torch.empty(8 * 48 * 2 * n_products * 64 * 8, device=w_pairs.device, dtype=torch.float16)
    ops.ss_layer512_pack_gate(w_pairs, out, n_products)
    return out


def layer512_pack_res(w_pairs, n_products=2):
    """ss_split_f16 pack [>= 256][256*2] of the output projection (first 256 rows = residual half) -> fragment order (fp16 [131072]; n_products = 1: [65536])."""
    assert w_pairs.dtype == torch.float16 and w_pairs.shape[0] >= 256 and w_pairs.shape[1] == 512 and w_pairs.is_contiguous(), tuple(w_pairs.shape)
    out = torch.empty(8 * 16 * n_products * 64 * 8, device=w_pairs.device, dtype=torch.float16)
    ops.ss_layer512_pack_res(w_pairs, out, n_products)
    return out


def layer512_tile_addend(E, *, B, T, lde=None, e_bs=None, out=None):
    """E fp32 [B][T][lde] (the layer's 512 packed addend columns start at E) -> the tiled slab ss_layer512 reads."""
    lde = lde if lde is not None else E.shape[-1]
    n = load().ss_layer512_addend_floats(B, T)
    out = torch.empty(n, device=E.device, dtype=torch.float32) if out is None else out
    ops.ss_layer512_tile_addend(E, lde, e_bs if e_bs is not None else T * lde, out, B, T)
    return out


def layer512_tile_addend_f16(E, n_sets, *, B, T, lde=None, e_bs=None):
    """E fp32 [B][T][lde] -> fp16 [n_sets][ss_layer512_addend_halfs]: the addend slab as sigma-delta sets (ss_layer512 with e_f16 reads ONE of them per launch)."""
    lde = lde if lde is not None else E.shape[-1]
    n = load().ss_layer512_addend_halfs(B, T)
    out = torch.empty(n_sets, n, device=E.device, dtype=torch.float16)
    ops.ss_layer512_tile_addend_f16(E, lde, e_bs if e_bs is not None else T * lde, out, n_sets, n, B, T)
    return out


def layer512_addend_values(E512, *, B, T, f16=False):
    """a tiled addend slab (fp32 form, or ONE fp16 set) -> [B][T][512] in the packed column order, as the gate's exp2 arguments (test helper)"""
    nt = (T + 127) // 128
    if f16:
        v = E512.view(B * nt, 4, 4, 8, 2, 32, 2, 4).float()            # tile, m, q, wave, lh, l31, nb, e
        v = v.permute(0, 1, 5, 3, 6, 2, 4, 7)                          # tile, m, l31, wave, nb, q, lh, e
    else:
        v = E512.view(B * nt, 2, 4, 4, 8, 2, 32, 4)                    # tile, nb, m, q, wave, lh, l31, e
        v = v.permute(0, 2, 6, 4, 1, 3, 5, 7)                          # tile, m, l31, wave, nb, q, lh, e
    return v.reshape(B, nt * 128, 512)[:, :T]


def layer512_entry(X, bias=None, *, B, T, lens=None):
    """ss_layer512_entry: X fp32 [B][T][256] -> (H = fp16(X + bias) in slot-major tiles (fp16 [elems]), P = X in accumulator order (uint8 buffer of fp32))"""
    H = torch.empty(load().ss_layer512_h_elems(B, T), device=X.device, dtype=torch.float16)
    P = torch.empty(load().ss_layer512_stream_bytes(B, T), device=X.device, dtype=torch.uint8)
    ops.ss_layer512_entry(X, X.shape[-1], T * X.shape[-1], bias, lens, H, P, B, T)
    return H, P


def layer512_h_values(H, *, B, T):
    """H (slot-major tiles [tile][slot 32][row 128][8]) -> fp16 [B][T][256] (test helper)"""
    nt = (T + 127) // 128
    return H.view(B * nt, 32, 128, 8).permute(0, 2, 1, 3).reshape(B, nt * 128, 256)[:, :T]


def layer512_stream_values(P, H, bias=None, *, B, T, lens=None):
    """the stream x = (H - bias) + R from its two terms: H (slot-major tiles, = fp16(x + bias)) and P = R, the fp16 remainder in accumulator order
    -> fp32 [B][T][256], rows >= lens[b] zero (test helper: the index map and the arithmetic of include/stylesinger_hip.h)"""
    nt = (T + 127) // 128
    v = P.view(torch.float16).view(B * nt, 4, 4, 8, 2, 32, 4).float()  # tile, m, q, wave, lh, l31, e
    r = v.permute(0, 1, 5, 3, 2, 4, 6).reshape(B, nt * 128, 256)[:, :T]   # tile, (m, l31) = row, (wave, q, lh, e) = channel
    h = layer512_h_values(H, B=B, T=T).float()
    x = (h - bias) + r if bias is not None else h + r
    if lens is not None:
        x = x * (torch.arange(T, device=x.device)[None, :, None] < lens.to(x.device)[:, None, None])
    return x


def layer512(Hin, Wg, E512, G, *, B, T, d, lens=None, Hout=None, P=None, Wr=None, bias_r=None, next_bias=None, out_scale=1.0 / 256.0,
             post_scale=0.70710678118654752440, ldg=None, g_bs=None, mask_rows=True, n_products=2, g_compact=False, e_f16=False, cur_bias=None):
    """ss_layer512: one launch per residual layer (gate + residual projection) of the fp16x2 mel denoiser; see include/stylesinger_hip.h."""
    a = Layer512Args()
    if e_f16 and E512 is not None:   # the fp16 sigma-delta sets travel in the `const float* E512` member: reinterpreted on purpose, so by address
        E512 = ptr(E512)
    set_members(a, Hin=Hin, Hout=Hout, P=P, lens=lens, Wg=Wg, Wr=Wr, E512=E512, G=G, bias_r=bias_r, next_bias=next_bias, cur_bias=cur_bias)
    a.d = d; a.n_products = n_products; a.g_compact = int(g_compact); a.e_f16 = int(e_f16)
    a.B = B; a.T = T
    a.ldg = ldg if ldg is not None else G.shape[-1]; a.g_batch_stride = g_bs if g_bs is not None else T * a.ldg
    a.mask_rows = int(mask_rows)
    a.out_scale = out_scale; a.post_scale = post_scale
    ops.ss_layer512(a)


def layernorm(x, gamma, beta, *, B, T, C_, out=None, lens=None, mask_rows=False, eps=1e-5):
    out = x if out is None else out
    ops.ss_layernorm(x, out, gamma, beta, B, T, C_, C_, C_, T * C_, T * C_, float(eps), lens, int(mask_rows))
    return out


def attention(Q, K, V, O, *, B, H, D, Tq, Tk, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, qlens=None, klens=None, scale):
    ops.ss_attention(Q, K, V, O, B, H, D, Tq, Tk, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, qlens, klens, float(scale))


def attention_seg(Q, K, V, O, *, B, H, D, Tq, R, Ts, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, qlens=None, seg_lens, seg_logw, scale):
    """ss_attention_seg: the attention core over R key segments of Ts rows with per-segment lengths and log prior weights [B, R]."""
    ops.ss_attention_seg(Q, K, V, O, B, H, D, Tq, R, Ts, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, qlens, seg_lens, seg_logw, float(scale))
