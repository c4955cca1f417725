"""Launch contracts of the five many-round 16-bit LDS-DMA GEMM kernels (gemm_bf16_gate256 / gate128 / gate128q / tile256 / tile256q.hip), without
a GPU. Each kernel states its contract once (<kernel>_contract): its dispatch predicate ss_gemm_bf16_*_ok is "the contract holds and the launch has
enough rounds of tiles", its launcher refuses what the contract refuses - so a launch the dispatcher hands over is never refused afterwards, and one
that breaks a rule falls back to another kernel. Here: a valid production-size argument struct per kernel form gives _ok == 1; every single violation
of a rule gives _ok == 0 AND makes the launcher return the argument error that names the kernel. Predicates and refusals return before any HIP call
(pointers are never followed; without a device the CU count falls back to 256), and the launcher is never called with a valid struct."""
import ctypes as C

import pytest

from stylesinger_amd import lib as L

SS_ERR_ARG = -1
P = 1 << 20                      # a dummy non-null 16-byte-aligned pointer
B, T = 64, 8192                  # 64 x 32 row tiles of 256: every size rule holds on 256 CUs
BIG = 1 << 18                    # T * BIG * 2 bytes = 2^32: past 32-bit offsets (a multiple of 8, and >= every 2 K / 2 N here)


def _args(**kw):
    a = L.GemmBf16Args()
    taps = kw.pop("taps")
    a.ntaps = len(taps)
    for i, o in enumerate(taps):
        a.tap_off[i] = o
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _gate(split, **kw):
    """the fp16x2 / fp16q4 / bf16x2 GATE launch of the C4 mel stack (C = 256: K = N = 256, Np = 512), pair layout"""
    d = dict(A=P, W=P, C=P, E=P, B=B, T=T, K=256, N=256, Np=512, lda=512, a_batch_stride=T * 512, ldc=512, c_batch_stride=T * 512, lde=512,
             e_batch_stride=T * 512, taps=(-8, 0, 8), epi=L.HEPI_GATE, split=split, out_scale=2.0 ** -8, q_scale=0.25 if split == 3 else 0.0, mask_rows=1)
    d.update(kw)
    return d


def _gate_plain(**kw):
    """the plain bf16 GATE launch: rows of K / N single terms"""
    return _gate(0, lda=256, a_batch_stride=T * 256, ldc=128, c_batch_stride=T * 128, out_scale=1.0, **kw)


def _store(split, **kw):
    """the K = L * C skip GEMM (20 layers of 256 channels), fp32 output"""
    d = dict(A=P, W=P, C=P, B=B, T=T, K=5120, N=256, Np=256, lda=10240, a_batch_stride=T * 10240, ldc=256, c_batch_stride=T * 256, taps=(0,),
             epi=L.HEPI_STORE, act=L.ACT_NONE, split=split, out_scale=2.0 ** -8 if split >= 2 else 1.0, q_scale=0.25 if split == 3 else 0.0, mask_rows=1)
    d.update(kw)
    return d


def _resx(split, **kw):
    """the residual projection on the pair-only stream (X = NULL)"""
    d = dict(A=P, W=P, Y=P, cur_bias=P, B=B, T=T, K=256, N=256, Np=256, lda=512, a_batch_stride=T * 512, ldy=512, y_batch_stride=T * 512, taps=(0,),
             epi=L.HEPI_RESX, split=split, out_scale=2.0 ** -8 if split == 2 else 1.0, post_scale=1.0, mask_rows=1)
    d.update(kw)
    return d


# violations shared by the three gate kernels: (what, overrides)
_GATE_TAPS = [("epi STORE", dict(epi=L.HEPI_STORE)), ("one tap", dict(taps=(0,))), ("asymmetric taps", dict(taps=(-3, 0, 5))),
              ("centre tap off 0", dict(taps=(-4, 1, 4))), ("d = 9", dict(taps=(-9, 0, 9))), ("d = 0", dict(taps=(0, 0, 0))), ("mirrored taps", dict(taps=(8, 0, -8)))]
_GATE_PAIR = [("K = 192", dict(K=192)), ("Np not a tile multiple", dict(Np=576)), ("2 N > Np", dict(Np=256)), ("N % 32", dict(N=248)), ("lda < 2 K", dict(lda=504)),
              ("lda % 8", dict(lda=516)), ("ldc < 2 N", dict(ldc=504)), ("ldc % 8", dict(ldc=516)), ("C NULL", dict(C=None)), ("A NULL", dict(A=None)), ("W NULL", dict(W=None)),
              ("out_scale = 0", dict(out_scale=0.0)), ("out_scale = 2", dict(out_scale=2.0)), ("out_scale NaN", dict(out_scale=float("nan"))),
              ("T * lda over 2^31", dict(lda=BIG)), ("T * lde over 2^31", dict(lde=BIG // 2)), ("T * ldc over 2^31", dict(ldc=BIG)),
              ("weights over 2^31", dict(Np=699136))]
_GATE128 = _GATE_TAPS + _GATE_PAIR + [("lde % 4", dict(lde=510)), ("A off by 8 bytes", dict(A=P + 8)), ("W off by 8 bytes", dict(W=P + 8)), ("E off by 8 bytes", dict(E=P + 8)),
                                      ("a_batch_stride odd", dict(a_batch_stride=T * 512 + 1)), ("e_batch_stride % 4", dict(e_batch_stride=T * 512 + 2))]
_Q_SCALE = [("q_scale = 3.0", dict(q_scale=3.0)), ("q_scale = 0", dict(q_scale=0.0)), ("q_scale < 0", dict(q_scale=-0.25)), ("q_scale = 2^-30", dict(q_scale=2.0 ** -30)),
            ("q_scale = 2^30", dict(q_scale=2.0 ** 30)), ("q_scale NaN", dict(q_scale=float("nan")))]
_ONE_TAP = [("three taps", dict(taps=(-1, 0, 1))), ("tap off 0", dict(taps=(1,))), ("epi GATE", dict(epi=L.HEPI_GATE))]
_TILE = [("N = 0", dict(N=0)), ("N > 256", dict(N=260, Np=512)), ("Np < N", dict(Np=128)), ("A NULL", dict(A=None)), ("W NULL", dict(W=None)), ("A off by 8 bytes", dict(A=P + 8)),
         ("W off by 8 bytes", dict(W=P + 8)), ("T * lda over 2^31", dict(lda=BIG))]
_STORE = _TILE + [("K % 64", dict(K=5152)), ("lda < 2 K", dict(lda=10232)), ("lda % 8", dict(lda=10244)), ("a_batch_stride odd", dict(a_batch_stride=T * 10240 + 1)),
                  ("weights over 2^31", dict(Np=104858)), ("C NULL", dict(C=None)), ("N % 4", dict(N=254)), ("ldc % 4", dict(ldc=258)), ("T * ldc over 2^31", dict(ldc=1 << 16)),
                  ("act gelu", dict(act=L.ACT_GELU)), ("act tanh", dict(act=L.ACT_TANH)), ("out_scale = 0", dict(out_scale=0.0)), ("out_scale = 2", dict(out_scale=2.0))]
_RESX = _TILE + [("K % 64", dict(K=288, lda=576)), ("lda < 2 K", dict(lda=504)), ("lda % 8", dict(lda=516)), ("a_batch_stride odd", dict(a_batch_stride=T * 512 + 1)),
                 ("weights over 2^31", dict(Np=2097152)), ("X != NULL", dict(X=P)), ("Y NULL", dict(Y=None)), ("cur_bias NULL", dict(cur_bias=None)), ("N % 32", dict(N=248)),
                 ("ldy < 2 N", dict(ldy=504)), ("ldy % 8", dict(ldy=516)), ("T * ldy over 2^31", dict(ldy=BIG)), ("a_compact", dict(a_compact=1)), ("one_product = 2", dict(one_product=2))]

# kernel -> (valid structs, violations as (what, base struct, overrides))
KERNELS = {
    "gate128": ([_gate(2), _gate(2, E=None), _gate(2, taps=(-1, 0, 1))],
                [(w, _gate(2), o) for w, o in _GATE128 + [("split = 1", dict(split=1)), ("split = 3", dict(split=3)), ("split = 0", dict(split=0))]]),
    "gate128q": ([_gate(3), _gate(3, E=None), _gate(3, q_scale=2.0 ** -21), _gate(3, q_scale=2.0 ** 19)],
                 [(w, _gate(3), o) for w, o in _GATE128 + _Q_SCALE + [("split = 2", dict(split=2)), ("split = 1", dict(split=1))]]),
    "gate256": ([_gate(2), _gate(1), _gate_plain(), _gate_plain(N=120)],
                [(w, _gate(2), o) for w, o in _GATE_TAPS + _GATE_PAIR + [("split = 3", dict(split=3)), ("split = -1", dict(split=-1)), ("Np % 256", dict(Np=640))]] +
                [(w, _gate(1), o) for w, o in [("N % 32 (bf16x2)", dict(N=248)), ("lda < 2 K (bf16x2)", dict(lda=504)), ("ldc < 2 N (bf16x2)", dict(ldc=504))]] +
                [(w if w.endswith("(plain)") else w + " (plain)", _gate_plain(), o) for w, o in _GATE_TAPS + [("N % 8 (plain)", dict(N=252)), ("lda % 8 (plain)", dict(lda=260)), ("ldc % 8 (plain)", dict(ldc=132)),
                                                                 ("K = 192 (plain)", dict(K=192))]]),
    "tile256": ([_store(2), _store(1), _store(2, act=L.ACT_RELU), _store(2, one_product=1), _store(2, a_compact=1, lda=5120, a_batch_stride=T * 5120),
                 _store(2, a_compact=1, one_product=2, lda=5120, a_batch_stride=T * 5120), _resx(2), _resx(1), _resx(2, next_bias=P)],
                [(w, _store(2), o) for w, o in _ONE_TAP + _STORE + [("split = 0", dict(split=0)), ("split = 3", dict(split=3)), ("one_product = 3", dict(one_product=3)),
                                                                    ("one_product = -1", dict(one_product=-1)), ("lda < K (a_compact)", dict(a_compact=1, lda=5112))]] +
                [(w + " (bf16x2)", _store(1), o) for w, o in [("a_compact", dict(a_compact=1)), ("one_product = 2", dict(one_product=2))]] +
                [(w + " (RESX)", _resx(2), o) for w, o in _ONE_TAP[:2] + _RESX + [("split = 0", dict(split=0)), ("out_scale = 0", dict(out_scale=0.0))]]),
    "tile256q": ([_store(3), _store(3, act=L.ACT_RELU), _store(3, N=64, Np=64)],
                 [(w, _store(3), o) for w, o in _ONE_TAP[:2] + _STORE + _Q_SCALE + [("split = 2", dict(split=2)), ("split = 0", dict(split=0)), ("epi RESX", dict(epi=L.HEPI_RESX))]]),
}
VIOLATIONS = [pytest.param(k, base, over, id=f"{k}-{what}") for k, (_, bad) in KERNELS.items() for what, base, over in bad]


def _fns(kernel):
    l = L.load()
    return getattr(l, f"ss_gemm_bf16_{kernel}_ok"), getattr(l, f"ss_gemm_bf16_{kernel}"), l


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_a_valid_production_launch_is_taken(kernel):
    ok, _, l = _fns(kernel)
    assert l.ss_get_tuning(b"q4_force") == 0
    for i, d in enumerate(KERNELS[kernel][0]):
        assert ok(C.byref(_args(**d))) == 1, (kernel, i)
    assert ok(None) == 0
    # the size rule is the other half of the predicate: one short item breaks no rule of the contract, but is not worth a launch of 256-row tiles
    assert ok(C.byref(_args(**dict(KERNELS[kernel][0][0], B=1, T=300)))) == 0


@pytest.mark.parametrize("kernel, base, over", VIOLATIONS)
def test_one_broken_rule_is_refused_by_predicate_and_launcher_alike(kernel, base, over):
    ok, launch, l = _fns(kernel)
    a = _args(**dict(base, **over))
    assert ok(C.byref(a)) == 0
    assert launch(C.byref(a), None) == SS_ERR_ARG
    assert l.ss_last_error().startswith(f"ss_gemm_bf16_{kernel}: ".encode()), l.ss_last_error()


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_the_launcher_refuses_null_args(kernel):
    _, launch, l = _fns(kernel)
    assert launch(None, None) == SS_ERR_ARG and l.ss_last_error() == f"ss_gemm_bf16_{kernel}: null args".encode()
