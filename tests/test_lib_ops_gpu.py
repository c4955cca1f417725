"""The checked call path on the device: L.ops passes what the raw calls pass, and a refused argument launches nothing."""
import pytest
import torch

from stylesinger_amd import lib as L

pytestmark = pytest.mark.gpu

B, T, C = 2, 5, 80


def test_ops_is_bit_identical_to_the_raw_calls():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, C, generator=g).to(dev)
    gamma, beta = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    lens = torch.tensor([T, 3], dtype=torch.int32, device=dev)
    raw, chk = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    L.check(L.load().ss_layernorm(L.ptr(x), L.ptr(raw), L.ptr(gamma), L.ptr(beta), B, T, C, C, C, T * C, T * C, 1e-5, L.ptr(lens), 1, L.stream_ptr()), "ss_layernorm")
    L.ops.ss_layernorm(x, chk, gamma, beta, B, T, C, C, C, T * C, T * C, 1e-5, lens, 1)
    assert torch.equal(raw, chk) and torch.isfinite(raw).all() and not torch.equal(raw, torch.full_like(x, 7.0))
    n_table = 11
    idx = torch.randint(0, n_table, (B, T), generator=g).to(dev)
    table = torch.randn(n_table, C, generator=g).to(dev)
    raw, chk = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    L.check(L.load().ss_embedding(L.ptr(idx), L.ptr(table), L.ptr(raw), B * T, C, n_table, C ** 0.5, 0, L.stream_ptr()), "ss_embedding")
    L.ops.ss_embedding(idx, table, chk, B * T, C, n_table, C ** 0.5, 0, L.stream_ptr())   # the full-length form
    assert torch.equal(raw, chk) and not (raw == 7.0).any()
    L.ops.ss_embedding(idx, table, chk, B * T, C, n_table, C ** 0.5, 1)   # accumulate on a view of the same rows
    assert torch.equal(chk, raw + raw)


def test_a_refused_argument_launches_nothing():
    dev = torch.device("cuda:0")
    x = torch.randn(B, T, C, device=dev)
    y = torch.full_like(x, 7.0)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    with pytest.raises(TypeError) as e:
        L.ops.ss_layernorm(x.double(), y, gamma, beta, B, T, C, C, C, T * C, T * C, 1e-5, None, 0)
    assert "ss_layernorm" in str(e.value) and "'x'" in str(e.value) and "torch.float64" in str(e.value)
    with pytest.raises(TypeError) as e:
        L.ops.ss_layernorm(x, y, gamma, beta, B, T, C, C, C, T * C, T * C, 1e-5, torch.full((B,), T, device=dev), 0)   # int64 lens for `const int32_t*`
    assert "'lens'" in str(e.value) and "torch.int64" in str(e.value)
    with pytest.raises(L.StyleSingerHipError) as e:
        L.ops.ss_layernorm(x, y, gamma.cpu(), beta, B, T, C, C, C, T * C, T * C, 1e-5, None, 0)
    assert "needs device tensors" in str(e.value) and "'gamma'" in str(e.value)
    with pytest.raises(TypeError):
        L.ops.ss_layernorm(x, y, gamma, beta, B, T, C, C, C, T * C, T * C, 1e-5, None)
    torch.cuda.synchronize()
    assert (y == 7.0).all(), "the output buffer is as it was: nothing ran"
