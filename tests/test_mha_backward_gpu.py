"""aimet_attn_softmax_backward and the opt-in fused training route of QuantizableMultiheadAttention
against the literal chain restated in float64 on the CPU: QDQ on the score encoding's grid,
masked_fill(-inf), softmax and the two straight-through masks, differentiated by autograd.

Tolerance of the kernel tests: |dx - dx64| <= 2^-16 max|g|. p carries at most about 26 ulp (exp_r within
3, a sum of depth <= 22, one divide), d that plus its own depth, |p| <= 1: about 104 * 2^-24 max|g|,
rounded up to a power of two. A wrong mask index, a missing STE factor or a wrong d is off by the size
of the gradient itself."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available

import mha_oracle as O
from aimet_amd import _native
from aimet_amd import transformers as T
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES
from aimet_amd.quantsim import QuantizationSimModel

gpu = lambda f: pytest.mark.gpu(pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")(f))  # noqa: E731
DEV, F = "cuda", np.float32
B, H, L = 2, 3, 3
SCORE_ENC = (-6.3, 7.1, 8)
SENTINEL = -777.25


@functools.lru_cache(None)
def data(S):
    """The fixed inputs for rows of S: scores, the 3-D mask, g, the prob encoding, a padding mask."""
    rng = np.random.default_rng(1000 + S)
    scores = (3 * rng.standard_normal((B * H, L, S))).astype(F)
    mask = rng.random((B * H, L, S)) < 0.3
    mask[..., 0] = False
    g = rng.standard_normal((B * H, L, S)).astype(F)
    kpm = (np.arange(S)[None, :] + np.arange(B)[:, None]) % 5 == 2
    kpm[:, 0] = False
    return scores, mask, g, (0.0, float(F(min(0.3, 8 / S))), 8), kpm


def ste(x, value, enc):
    inside = (x >= float(F(enc[0]))) & (x <= float(F(enc[1])))
    return value.detach() + (x - x.detach()) * inside, inside


@functools.lru_cache(None)
def reference(S, masked, enc):
    """float64: (dx, positions that must be exactly zero). The quantized score is the float32 grid value
    (its value feeds the softmax; its gradient is the STE mask); the probability QDQ moves no gradient
    but through its STE mask."""
    scores, mask, g, prob_enc, kpm = data(S)
    x = torch.from_numpy(scores.astype(np.float64)).requires_grad_(True)
    zero = np.zeros(scores.shape, bool)
    xq = x
    if enc:
        xq, inside = ste(x, torch.from_numpy(O.qdq(scores, SCORE_ENC).astype(np.float64)), SCORE_ENC)
        zero |= ~inside.numpy()
    if masked:
        eff = mask | np.repeat(kpm, H, axis=0)[:, None, :]
        xq = xq.masked_fill(torch.from_numpy(eff), float("-inf"))
        zero |= eff
    p = torch.softmax(xq, dim=-1)
    if enc:
        pmax = prob_enc[1]
        assert float(((p.detach() - pmax).abs() / pmax).min()) > 1e-4   # the prob STE mask is unambiguous
        p, _ = ste(p, p, prob_enc)
    (p * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return x.grad.numpy(), zero


def run(S, masked, enc, out=None, scores=None, am=None, kpm=None, g=None):
    d = data(S)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    if masked and am is None:
        am, kpm = d[1], d[4]
    g = dev(d[2] if g is None else g)
    return T.attn_softmax_backward(dev(d[0] if scores is None else scores), g, B, H, dev(am), dev(kpm),
                                   SCORE_ENC if enc else None, d[3] if enc else None,
                                   out=g if out == "in place" else out)


def check(got, want, zero, g):
    got = got.cpu().numpy()
    assert np.all(got[zero] == 0)   # bitwise +0 or -0, never NaN
    err = float(np.abs(got - want).max())
    print("max |dx - dx64| = %.3g of the bound %.3g" % (err, 2.0 ** -16 * np.abs(g).max()))
    assert err <= 2.0 ** -16 * np.abs(g).max()


@gpu
@pytest.mark.parametrize("enc", [True, False], ids=["both_enc", "no_enc"])
@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "attn3d_padding"])
@pytest.mark.parametrize("S", [1, 2, 5, 63, 64, 65, 129, 257, 1024, 1025, 1030])
def test_kernel_against_the_float64_chain(S, masked, enc):
    want, zero = reference(S, masked, enc)
    n = T.attn_backward_launch_count()
    for out in (None, "in place"):
        check(run(S, masked, enc, out), want, zero, data(S)[2])
    assert T.attn_backward_launch_count() == n + 2


@gpu
def test_misaligned_output_between_guards_a_fully_masked_row_and_the_refusal():
    S = 1025
    want, zero = (a.copy() for a in reference(S, True, True))
    am = data(S)[1].copy()
    am[4, 1, :] = True
    want[4, 1], zero[4, 1] = 0.0, True
    buf = torch.full((9 + want.size + 8,), SENTINEL, device=DEV)   # 256-byte base: the view is one float off 16
    got = run(S, True, True, out=buf[9:9 + want.size].view(want.shape), am=am, kpm=data(S)[4])
    check(got, want, zero, data(S)[2])
    assert bool((buf[:9] == SENTINEL).all()) and bool((buf[9 + want.size:] == SENTINEL).all())
    S, n = T.attn_softmax_max_s() + 1, T.attn_backward_launch_count()
    out = torch.full((1, 1, S), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="not resident"):
        T.attn_softmax_backward(torch.zeros(1, 1, S, device=DEV), torch.zeros(1, 1, S, device=DEV), 1, 1, out=out)
    assert T.attn_backward_launch_count() == n and bool((out == SENTINEL).all())


@gpu
@pytest.mark.parametrize("S", [5, 1025])
def test_forward_identity_and_saved_scores(S):
    scores, mask, _, prob_enc, kpm = data(S)
    x = torch.from_numpy(scores).to(DEV).requires_grad_(True)
    args = (B, H, torch.from_numpy(mask).to(DEV), torch.from_numpy(kpm).to(DEV), SCORE_ENC, prob_enc)
    probs = T.AttnSoftmax.apply(x, *args)
    assert torch.equal(probs, T.attn_softmax(x.detach(), *args)) and probs.requires_grad
    assert torch.equal(x.detach().cpu(), torch.from_numpy(scores))


@gpu
@pytest.mark.parametrize("S,stride", [(2, 4 * 65536), (1025, 65536)], ids=["wave", "lds"])
def test_rows_of_the_second_grid_stride_trip(S, stride):
    """attn_softmax.hip caps the grid at 65536 workgroups of four rows (wave path) or one (LDS path)."""
    rows = stride + (8 if S == 2 else 2)
    want, zero = reference(S, True, True)
    scores, mask, g, _, kpm = data(S)
    tile = np.arange(rows) % (B * H * L)
    assert rows % (B * H) == 0 and stride % (B * H * L) != 0
    big = lambda a: a.reshape(-1, S)[tile].reshape(B * H, -1, S)  # noqa: E731
    eff = mask | np.repeat(kpm, H, axis=0)[:, None, :]
    got = run(S, True, True, scores=big(scores), am=big(eff), g=big(g)).view(-1, S)
    pick = np.r_[0:5, stride - 3:rows]
    check(got[torch.from_numpy(pick).to(DEV)], want.reshape(-1, S)[tile[pick]], zero.reshape(-1, S)[tile[pick]], g)


@gpu
def test_module_trains_through_one_launch_each_way():
    torch.manual_seed(5)
    was, torch.backends.cuda.matmul.allow_tf32 = torch.backends.cuda.matmul.allow_tf32, False
    attn = T.QuantizableMultiheadAttention(16, 4).to(DEV).eval()
    x = torch.randn(5, 3, 16, device=DEV)
    kpm = torch.tensor([[False] * 5, [False, False, False, True, True], [False, True, False, False, False]], device=DEV)
    sim = QuantizationSimModel(attn, dummy_input=(x, x, x), quant_scheme="tf", default_output_bw=16,
                               quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    sim.compute_encodings(lambda m, _: m(x, x, x, key_padding_mask=kpm))
    weight = torch.randn(5, 3, 16, device=DEV)
    grads, launches = {}, {}
    for route, (fused, fused_backward) in {"literal": (False, False), "default": (True, False),
                                           "fused": (True, True)}.items():
        sim.model.fused = fused
        assert T.set_fused_attention_backward(sim.model, fused_backward) == 1
        xg = x.clone().requires_grad_(True)
        sim.model.zero_grad()
        n = (T.attn_launch_count(), T.attn_backward_launch_count())
        (sim.model(xg, xg, xg, key_padding_mask=kpm)[0] * weight).sum().backward()
        launches[route] = (T.attn_launch_count() - n[0], T.attn_backward_launch_count() - n[1])
        grads[route] = {"x": xg.grad} | {k: p.grad.clone() for k, p in sim.model.named_parameters() if "weight" in k}
    torch.backends.cuda.matmul.allow_tf32 = was
    assert launches == {"literal": (0, 0), "default": (0, 0), "fused": (1, 1)}
    assert len(grads["literal"]) == 5
    for k, want in grads["literal"].items():
        assert float((grads["fused"][k] - want).abs().max()) <= 1e-3 * float(want.abs().max()), k


def test_c_abi_names_are_exported():
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        header = f.read()
    for name in ("aimet_attn_softmax_backward", "aimet_attn_backward_launch_count"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(_native.load(), name) and "int %s(" % name in header
