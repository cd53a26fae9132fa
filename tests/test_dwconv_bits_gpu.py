"""The depthwise AdaRound kernels give the bits that tests/golden/dwconv_bits.json records.

The one-pass step (aimet_adaround_dw_step) and the four-launch chain it replaces (gather -> forward
-> reconstruction gradient -> weight gradient) are instantiations of one slice body in dwconv.hip,
so comparing one with the other cannot see a mistake they share. The fixture was recorded from the
kernels as they stood before they were merged into that body (tests/golden/make_golden_dw.py): each
case's weight gradient and its [C][S][K K] slices, over iterations 0 and 2, as sha256. So that a
recorded hash cannot enshrine a wrong answer, every case also checks the forward against torch's
conv2d, the weight gradient against autograd (the tolerances of test_depthwise_conv_kernels_vs_torch)
and the step against the chain bit for bit.

The cases are the smallest shapes at which each path can go wrong: the quad form with several
slices and `per` rounded up to a quad, H != W, the generic form with odd sizes, dilation, padding
past the kernel, K = 5, OW % 4 != 0, the quad form refused because the target cache / grad_y is not
16-byte aligned, and batches past the 1024 rows whose table the step keeps in LDS."""
import collections
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwconv_bits.json")
ITERS = (0, 2)   # of a 3-row idx_all

# off: the target cache (step) and grad_y (chain) start `off` floats past a 16-byte boundary
Case = collections.namedtuple("Case", "name N C H W K stride pad dil act bias off quads")
CASES = [
    Case("quad_slices_per_rounded", 11, 5, 12, 12, 3, 1, 1, 1, 2, True, 0, True),
    Case("quad_nonsquare", 3, 4, 10, 16, 3, 1, 1, 1, 0, False, 0, True),
    Case("generic_nonsquare_odd", 5, 7, 9, 13, 3, 2, 0, 1, 0, True, 0, False),
    Case("generic_dilated_overpadded", 3, 12, 17, 17, 3, 1, 2, 2, 1, True, 0, False),
    Case("generic_k5", 4, 6, 19, 15, 5, 2, 2, 1, 1, False, 0, False),
    Case("generic_ow_not_quads", 3, 5, 7, 7, 3, 1, 1, 1, 2, False, 0, False),
    Case("quad_refused_by_alignment", 3, 4, 12, 12, 3, 1, 1, 1, 1, True, 1, False),
    Case("rows_in_global_quad", 1025, 2, 4, 4, 3, 1, 1, 1, 0, False, 0, True),
    Case("rows_in_global_generic", 1025, 2, 5, 5, 3, 1, 1, 1, 2, True, 0, False),
]


def out_size(n, c):
    return (n + 2 * c.pad - c.dil * (c.K - 1) - 1) // c.stride + 1


def plan(c, OH, OW):
    """The slice plan of the weight gradient, restated: 16 positions per lane, ~2048 workgroups of
    256 lanes, `per` rounded up to whole quads in the quad form. Returns (S, per)."""
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    npos = c.N * OH * OW
    S = cdiv(npos, 256 * 16)
    want = cdiv(2048, c.C)
    if S < want:
        S = min(want, cdiv(npos, 256))
    per = cdiv(npos, max(S, 1))
    if c.quads:
        per = cdiv(per, 4) * 4
    return cdiv(npos, per), per


def device(a, off=0):
    """`a` on the device, its first element `off` floats past a 16-byte boundary."""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return v


def sha(parts):
    h = hashlib.sha256()
    for t in parts:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(c, seed):
    """Every route of case `c`, checked against torch and against each other; returns
    {"S", "grad_w", "slices"}: the hashes are over iterations 0 and 2 in that order."""
    N, C, H, W, K = c.N, c.C, c.H, c.W, c.K
    OH, OW = out_size(H, c), out_size(W, c)
    rows = N + 5
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x_cache = device(rng.standard_normal((rows, C, H, W), dtype=f32))
    t_cache = device(rng.standard_normal((rows, C, OH, OW), dtype=f32) * f32(2) + f32(1), c.off)
    w = device(rng.standard_normal((C, 1, K, K), dtype=f32) * f32(0.3))
    b = device(rng.standard_normal(C, dtype=f32)) if c.bias else None
    idx = torch.from_numpy(np.stack([rng.permutation(rows)[:N] for _ in range(3)]).astype(np.int64)).to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    dims = (N, C, H, W, OH, OW, K, c.stride, c.pad, c.dil)

    n_ws, S = ctypes.c_int64(), ctypes.c_int64()
    _native.call("aimet_dwconv2d_grad_weight_workspace", N, C, OH, OW, K, ctypes.byref(n_ws))
    _native.call("aimet_adaround_dw_step_slices", P(t_cache), N, C, OH, OW, K, c.stride, c.dil, ctypes.byref(S))
    S = S.value
    assert S == plan(c, OH, OW)[0], "the form the case means (quads: %s)" % c.quads
    n_sl = C * S * K * K
    assert n_sl <= n_ws.value

    def workspace():
        return torch.full((n_ws.value,), float("nan"), device=DEV)

    routes = collections.defaultdict(list)   # route -> [tensor per iteration]
    for it in ITERS:
        # the chain
        ctr = torch.tensor([it, -1], dtype=torch.long, device=DEV)
        inp = torch.empty(N, C, H, W, device=DEV)
        _native.call("aimet_adaround_gather", P(x_cache), P(t_cache), P(inp), None, P(idx), ctr.data_ptr(),
                     ctr.data_ptr() + 8, N, C * H * W, C * OH * OW, s)
        q = torch.empty(N, C, OH, OW, device=DEV)
        _native.call("aimet_dwconv2d_forward", P(inp), P(w), P(b), P(q), *dims, s)
        gq = device(np.zeros((N, C, OH, OW), f32), c.off)
        _native.call("aimet_adaround_recon_grad_indexed", P(q), P(t_cache), P(idx), ctr.data_ptr(), P(gq), N, C,
                     OH * OW, None, c.act, s)
        ws = workspace()
        gw = torch.empty_like(w)
        _native.call("aimet_dwconv2d_grad_weight", P(inp), P(gq), P(gw), P(ws), *dims, s)
        routes["chain grad_w"].append(gw)
        routes["chain slices"].append(ws[:n_sl])
        gw = torch.empty_like(w)
        _native.call("aimet_dwconv2d_grad_weight", P(inp), P(gq), P(gw), None, *dims, s)
        routes["chain grad_w, no workspace"].append(gw)
        assert ctr.tolist() == [it, it + 1]

        # forward and weight gradient against torch
        prev = torch.backends.cudnn.enabled
        torch.backends.cudnn.enabled = False
        try:
            wr = w.clone().requires_grad_(True)
            ref = torch.nn.functional.conv2d(inp, wr, b, c.stride, c.pad, c.dil, C)
            ref.backward(gq)
        finally:
            torch.backends.cudnn.enabled = prev
        assert ref.shape == q.shape
        torch.testing.assert_close(q, ref.detach(), rtol=1e-6, atol=1e-5)
        scale = float((gq.abs().sum() * inp.abs().max()) / (N * OH * OW) ** 0.5)
        torch.testing.assert_close(routes["chain grad_w"][-1], wr.grad, rtol=2e-5, atol=1e-6 * scale)
        assert bool(gw.abs().sum() > 0)

        # the step: workspace and grad_w; no workspace; workspace only (the slices the Adam step folds)
        for route, with_ws, with_gw in (("step", True, True), ("step, no workspace", False, True),
                                        ("step, slices only", True, False)):
            ctr2 = torch.tensor([it, -1], dtype=torch.long, device=DEV)
            ws = workspace() if with_ws else None
            gw = torch.empty_like(w) if with_gw else None
            _native.call("aimet_adaround_dw_step", P(x_cache), P(t_cache), P(idx), ctr2.data_ptr(),
                         ctr2.data_ptr() + 8, P(w), P(b), P(gw), P(ws), *dims, c.act, s)
            assert ctr2.tolist() == [it, it + 1], route
            if with_gw:
                routes[route + " grad_w"].append(gw)
            if with_ws:
                routes[route + " slices"].append(ws[:n_sl])

    out = {"S": S, "grad_w": sha(routes["chain grad_w"]), "slices": sha(routes["chain slices"])}
    for route, tensors in routes.items():   # step == chain, with and without a workspace, bit for bit
        kind = "slices" if route.endswith("slices") else "grad_w"
        assert not any(bool(torch.isnan(t).any()) for t in tensors), route
        assert sha(tensors) == out[kind], (c.name, route)
    return out


def seed_of(c):
    return 2200 + CASES.index(c)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_dwconv_bits(c):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(k.name for k in CASES)
    assert run_case(c, seed_of(c)) == golden[c.name]
