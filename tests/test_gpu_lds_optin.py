"""The dynamic-LDS opt-in (csrc/optim.hip mts_dyn_lds) on a real MI355X: the limit above 64 KiB belongs to (kernel, device), so a
kernel whose need grows between two launches, and the first launch of a kernel on a second device, must both be opted in again.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R  # noqa: E402

DEV = 'cuda'


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def test_band_attention_lds_need_grows_on_one_kernel():
    """Generic fp32 band forward, one instantiation (MAXU = 8), twice in one process: head dim 192 needs 95 * 784 + 32 * 33 * 4 =
    78 704 bytes of LDS, head dim 256 then needs 95 * 1040 + 4 224 = 103 024.  Both against the fp64 oracle at the fp32 tolerance of
    test_gpu_kernels.py::test_band_attention_fwd_bwd."""
    from multimodaltopicsegmentation_amd import _lib as L
    from multimodaltopicsegmentation_amd import ops
    B, Lq, heads, radius = 1, 40, 1, 4
    slots = ops.band_slots(radius)
    try:
        L.check(L.lib.mts_set_option(b'band_mfma', 0))
        for hd in (192, 256):
            D = heads * hd
            qkv = _rnd(B * Lq, 3 * D, seed=30 + hd, scale=0.7)
            ctx = torch.full((B * Lq, D), float('nan'), device=DEV)
            probs = torch.full((B * Lq, heads * slots), float('nan'), device=DEV)
            ops.band_attn_fwd(qkv.to(DEV), None, B, Lq, D, heads, radius, ctx, probs)
            torch.cuda.synchronize()
            x64 = qkv.double().view(B, Lq, 3, heads, hd)
            ref = R.band_attention(x64[:, :, 0], x64[:, :, 1], x64[:, :, 2], torch.tensor([Lq] * B), radius).reshape(B * Lq, D)
            err = (ctx.cpu().double() - ref).abs()
            lim = 2e-5 + 2e-5 * ref.abs()
            print(f'hd {hd}: max err {float(err.max()):.3e}, ref max {float(ref.abs().max()):.3e}')
            assert not (err > lim).any(), f'hd {hd}: {int((err > lim).sum())}/{err.numel()} off, max err {float(err.max()):.3e}'
    finally:
        L.check(L.lib.mts_set_option(b'band_mfma', 1))


def test_gemm_224_first_launch_on_a_second_device():
    """One 256x224-tile GEMM (bf16, NT, bias) on device 0, then the same as the first thing run on device 1: same kernel, same bits."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two visible devices')
    from multimodaltopicsegmentation_amd import _lib as L
    from multimodaltopicsegmentation_amd import ops
    M, N, K = 256, 224, 256
    a = _rnd(M, K, seed=61).to(torch.bfloat16)
    b = _rnd(N, K, seed=62).to(torch.bfloat16)
    bias = _rnd(N, seed=63)
    outs, tiles = [], []
    try:
        L.check(L.lib.mts_set_option(b'gemm_tile', 224))
        for d in (0, 1):
            torch.cuda.set_device(d)
            dev = torch.device('cuda', d)
            out = torch.full((M, N), float('nan'), dtype=torch.bfloat16, device=dev)
            ops.gemm(L.NT, a.to(dev), b.to(dev), out, M=M, N=N, K=K, bias=bias.to(dev))
            torch.cuda.synchronize(dev)
            tile = ctypes.c_int(0)
            L.check(L.lib.mts_gemm_last_plan(ctypes.byref(tile), None))
            outs.append(out.cpu())
            tiles.append(tile.value)
    finally:
        torch.cuda.set_device(0)
        L.check(L.lib.mts_set_option(b'gemm_tile', 0))
    assert tiles[0] == tiles[1] and tiles[0] in (224, 225, 226), tiles
    assert not torch.isnan(outs[0].float()).any()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
