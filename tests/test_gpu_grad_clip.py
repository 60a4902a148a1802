"""Gradient clipping on the native training step (train_fit.py:288,295,779 --gradient_clipping -> Trainer(gradient_clip_val) ->
torch.nn.utils.clip_grad_norm_ before optimizer.step()):

  * mts_grad_norm against fp64, bit-reproducible, NaN / Inf as ordinary arithmetic;
  * mts_adam_step_clipped / mts_sgd_step_clipped against clip_grad_norm_ / clip_grad_value_ + torch.optim on the CPU, and bit for bit
    against the unclipped entry points when the coefficient clamps to 1;
  * trainer.NativeTrainer(gradient_clip_val=...) against the same step with the coefficient applied by hand, alone and with two
    ranks on cuda:0 over gloo (the pattern of test_gpu_dp_step.py).
"""
import functools
import os

import pytest
import torch

from tests.test_gpu_dp_step import _batches, _build, _free_port, _to_dev

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LR = {'Adam': 1e-3, 'SGD': 1e-2}


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


def _rnd(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _norm(ops, g_dev, spans, scale):
    """two calls into a NaN-filled workspace: the result, after checking that the second call gave the same bits"""
    ws = ops.grad_norm_workspace(DEV).fill_(float('nan'))          # partials the launch does not write are never read
    a, b = torch.full((), -1.0, device=DEV), torch.full((), -2.0, device=DEV)
    ops.grad_norm(g_dev, spans, scale, ws, a)
    ops.grad_norm(g_dev, spans, scale, ws, b)
    assert torch.equal(_bits(a), _bits(b))
    return float(a)


# ---- the reduction ------------------------------------------------------------------------------------------------------------------
# 2 097 159 = 2048 * 256 * 4 + 7: the grid-stride loop wraps and the scalar tail runs
@pytest.mark.parametrize('scale', [1.0, 0.125])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 1025, 2097159])
def test_grad_norm_matches_fp64(ops, n, scale):
    g = _rnd(n, seed=n)
    ref = float(g.double().mul(scale).square().sum().sqrt())
    got = _norm(ops, g.to(DEV), [(0, n)], scale)
    rel = abs(got - ref) / ref
    print(f'n {n} scale {scale}: got {got!r} ref {ref!r} rel {rel:.3e}')
    # a lane adds at most a few tens of non-negative terms in sequence, the trees add about 20 levels: ~4e-6 on the sum, half on the root
    assert rel <= 1e-5, (got, ref, rel)


@pytest.mark.parametrize('scale', [1.0, 0.125])
def test_grad_norm_two_spans_skip_the_gap(ops, scale):
    n = 8192
    g = _rnd(n, seed=7)
    spans = [(0, 1027), (2048, 2048 + 4101)]                         # aligned begins, ragged ends
    live = torch.cat([g[a:b] for a, b in spans])
    ref = float(live.double().mul(scale).square().sum().sqrt())
    g[1027:2048] = float('nan')                                      # garbage between and behind the spans: must not be read
    g[2048 + 4101:] = float('inf')
    got = _norm(ops, g.to(DEV), spans, scale)
    rel = abs(got - ref) / ref
    print(f'two spans scale {scale}: got {got!r} ref {ref!r} rel {rel:.3e}')
    assert rel <= 1e-5, (got, ref, rel)


def test_grad_norm_of_nothing_is_zero(ops):
    out = torch.full((), 5.0, device=DEV)
    ops.grad_norm(torch.ones(16, device=DEV), [(4, 4)], 1.0, ops.grad_norm_workspace(DEV), out)
    assert float(out) == 0.0


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('at', [0, 1000, 1024])                     # vector part, and the scalar tail of 1025
def test_grad_norm_propagates_nonfinite(ops, bad, at):
    g = _rnd(1025, seed=3)
    g[at] = bad
    got = _norm(ops, g.to(DEV), [(0, 1025)], 1.0)
    assert (got != got) if bad != bad else (got == float('inf')), got


# ---- the clipped optimizer kernels ----------------------------------------------------------------------------------------------------
N = 10007                                                            # several workgroups and a scalar tail, as test_adam_and_sgd_match_torch


def _close(got, ref, rtol, atol, msg):
    err = (got.detach().cpu().double() - ref.detach().double()).abs()
    bad = err > atol + rtol * ref.detach().double().abs()
    print(f'{msg}: max err {float(err.max()):.3e}')
    assert not bad.any(), f'{msg}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e}'


def test_coefficient_of_one_leaves_the_bits_of_the_unclipped_steps(ops):
    p0, g = _rnd(N, 41), _rnd(N, 42, 0.1).to(DEV)
    ws, norm, coef = ops.grad_norm_workspace(DEV), torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    st = {k: [p0.to(DEV).clone(), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), torch.empty(N, dtype=torch.bfloat16, device=DEV)]
          for k in ('plain', 'clipped')}
    for step in range(1, 4):
        gs = g * step
        ops.grad_norm(gs, [(0, N)], 0.25, ws, norm)
        p, m, v, mir = st['plain']
        ops.adam_step(p, gs, m, v, 1e-3, 0.9, 0.999, 1e-7, step, grad_scale=0.25, bf16_copy=mir)
        p, m, v, mir = st['clipped']
        ops.adam_step_clipped(p, gs, m, v, 1e-3, 0.9, 0.999, 1e-7, step, grad_scale=0.25, bf16_copy=mir, total_norm=norm,
                              max_norm=1e30, clip_coef_out=coef)
        assert float(coef) == 1.0 and float(norm) > 1.0
    for a, b in zip(st['plain'], st['clipped']):
        assert torch.equal(_bits(a.float()), _bits(b.float()))
    st = {k: [p0.to(DEV).clone(), torch.zeros(N, device=DEV), torch.empty(N, dtype=torch.bfloat16, device=DEV)] for k in ('plain', 'clipped')}
    for step in range(1, 4):
        ops.grad_norm(g, [(0, N)], 0.5, ws, norm)
        p, buf, mir = st['plain']
        ops.sgd_step(p, g, buf, 0.01, 0.9, 1e-4, step == 1, 0.5, mir)
        p, buf, mir = st['clipped']
        coef.fill_(-1.0)
        ops.sgd_step_clipped(p, g, buf, 0.01, 0.9, 1e-4, step == 1, 0.5, mir, total_norm=norm, max_norm=1e30, clip_coef_out=coef)
        assert float(coef) == 1.0
    for a, b in zip(st['plain'], st['clipped']):
        assert torch.equal(_bits(a.float()), _bits(b.float()))


def test_clipped_adam_and_sgd_match_clip_grad_norm(ops):
    """max_norm = a quarter of the gradient's fp64 norm: the coefficient is about 0.25.  Bars of test_adam_and_sgd_match_torch."""
    p0, g = _rnd(N, 41), _rnd(N, 42, 0.1)
    max_norm = 0.25 * float(g.double().norm())
    ws, norm, coef = ops.grad_norm_workspace(DEV), torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=1e-3, eps=1e-7)
    p, m, v = p0.to(DEV).clone(), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    mirror = torch.empty(N, dtype=torch.bfloat16, device=DEV)
    g4 = (g * 4).to(DEV)                                             # the device gradient is a SUM over 4 ranks: grad_scale 1/4 restores g exactly
    for step in range(1, 4):
        pt.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        ops.grad_norm(g4, [(0, N)], 0.25, ws, norm)
        ops.adam_step_clipped(p, g4, m, v, 1e-3, 0.9, 0.999, 1e-7, step, grad_scale=0.25, bf16_copy=mirror, total_norm=norm,
                              max_norm=max_norm, clip_coef_out=coef)
        assert abs(float(norm) - float(total)) <= 1e-5 * float(total)
        assert abs(float(coef) - 0.25) <= 1e-4                       # clipping demonstrably acts
    _close(p, pt, 1e-6, 1e-7, 'adam, norm mode')
    assert torch.equal(mirror.cpu(), p.cpu().to(torch.bfloat16))
    ps = torch.nn.Parameter(p0.clone())
    sgd = torch.optim.SGD([ps], lr=0.01, weight_decay=1e-4, momentum=0.9)
    p2, buf = p0.to(DEV).clone(), torch.zeros(N, device=DEV)
    gd = g.to(DEV)
    for step in range(1, 4):
        ps.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ps], max_norm)
        sgd.step()
        ops.grad_norm(gd, [(0, N)], 1.0, ws, norm)
        ops.sgd_step_clipped(p2, gd, buf, 0.01, 0.9, 1e-4, step == 1, 1.0, None, total_norm=norm, max_norm=max_norm, clip_coef_out=coef)
        assert abs(float(coef) - 0.25) <= 1e-4
    _close(p2, ps, 1e-6, 1e-7, 'sgd, norm mode')


def test_clipped_adam_and_sgd_match_clip_grad_value(ops):
    p0, g = _rnd(N, 41), _rnd(N, 42, 0.1)
    clip_value = 0.1                                                 # one standard deviation: about a third of the elements
    share = float((g.abs() > clip_value).float().mean())
    assert 0.1 <= share <= 0.9, share
    g[17] = float('nan')                                             # a NaN is not clamped away (clip_grad_value_ keeps it too)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=1e-3, eps=1e-7)
    ps = torch.nn.Parameter(p0.clone())
    sgd = torch.optim.SGD([ps], lr=0.01, weight_decay=1e-4, momentum=0.9)
    p, m, v = p0.to(DEV).clone(), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    p2, buf = p0.to(DEV).clone(), torch.zeros(N, device=DEV)
    mirror = torch.empty(N, dtype=torch.bfloat16, device=DEV)
    g4, gd = (g * 4).to(DEV), g.to(DEV)
    for step in range(1, 4):
        for prm, o in ((pt, opt), (ps, sgd)):
            prm.grad = g.clone()
            torch.nn.utils.clip_grad_value_([prm], clip_value)
            o.step()
        ops.adam_step_clipped(p, g4, m, v, 1e-3, 0.9, 0.999, 1e-7, step, grad_scale=0.25, bf16_copy=mirror, clip_value=clip_value)
        ops.sgd_step_clipped(p2, gd, buf, 0.01, 0.9, 1e-4, step == 1, 1.0, None, clip_value=clip_value)
    keep = torch.ones(N, dtype=torch.bool)
    keep[17] = False
    for got, ref, name in ((p, pt, 'adam'), (p2, ps, 'sgd')):
        assert torch.isnan(got[17]) and torch.isnan(ref[17])
        _close(got.cpu()[keep], ref.detach()[keep], 1e-6, 1e-7, f'{name}, value mode')
    assert torch.equal(mirror.cpu()[keep], p.cpu().to(torch.bfloat16)[keep])


# ---- NativeTrainer ----------------------------------------------------------------------------------------------------------------------
def _backward(tr, batch):
    """what NativeTrainer._step does in front of apply_optimizer() in one process"""
    m = tr.model
    tr._last_L = batch['src_tokens'].shape[1]
    m.loss_grad_scale, m._grad_hook = 1.0, None
    if batch.get('src_tokens2') is not None and hasattr(m, '_rnn2'):
        m.loss_and_grad(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'], batch['tgt_tokens'], True)
    else:
        m.loss_and_grad(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'], True)


def _train(kind, opt, by_hand=None, **clip):
    """Two steps on the global batch -> parameters, per-step fp64 norm of the raw gradient, last_grad_norm / last_clip_coef per step.
    by_hand = max_norm: the reference of the issue -- backward, coefficient in fp64 on the host, grad_flat().mul_(coef), UNCLIPPED optimizer."""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    model = _build(kind).to(DEV)
    tr = NativeTrainer(model, lr=LR[opt], optimizer=opt, **clip)
    out = {'raw': [], 'norm': [], 'coef': []}
    for batch in _batches(kind, False):
        batch = _to_dev(batch)
        if by_hand is None:
            tr.step(batch)
        else:
            _backward(tr, batch)
        out['raw'].append(float(model.grad_flat().double().norm()))
        if by_hand is not None:
            model.grad_flat().mul_(min(1.0, by_hand / (out['raw'][-1] + 1e-6)))
            tr.apply_optimizer()
        if tr.last_grad_norm is not None:
            out['norm'].append(tr.last_grad_norm.clone())
            out['coef'].append(float(tr.last_clip_coef))
    torch.cuda.synchronize()
    out['flat'] = model.flat.detach().cpu().clone()
    out['trainer'] = tr
    return out


@functools.lru_cache(maxsize=None)
def _unclipped(kind, opt):
    return _train(kind, opt)


@functools.lru_cache(maxsize=None)
def _clipped(kind, opt):
    return _train(kind, opt, gradient_clip_val=0.25 * _unclipped(kind, opt)['raw'][0])


CASES = [(k, o) for k in ('transformer', 'latefusion') for o in ('Adam', 'SGD')]


@pytest.mark.parametrize('kind,opt', CASES)
def test_huge_max_norm_is_the_unclipped_step_bit_for_bit(kind, opt):
    plain = _unclipped(kind, opt)
    assert plain['trainer'].last_grad_norm is None and plain['trainer'].last_clip_coef is None
    huge = _train(kind, opt, gradient_clip_val=1e30)
    assert huge['coef'] == [1.0, 1.0]
    assert torch.equal(_bits(huge['flat']), _bits(plain['flat']))
    for got, raw in zip(huge['norm'], plain['raw']):                 # last_grad_norm is the norm BEFORE clipping
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
        assert abs(float(got) - raw) <= 1e-5 * raw


@pytest.mark.parametrize('kind,opt', CASES)
def test_active_clipping_equals_the_coefficient_applied_by_hand(kind, opt):
    plain, got = _unclipped(kind, opt), _clipped(kind, opt)
    max_norm = 0.25 * plain['raw'][0]
    print(f'{kind} {opt}: raw norms {plain["raw"]}, max_norm {max_norm}, coefficients {got["coef"]}')
    assert len(got['coef']) == 2 and all(c < 1.0 for c in got['coef']), got['coef']
    assert abs(got['coef'][0] - max_norm / (plain['raw'][0] + 1e-6)) <= 1e-5          # about a quarter: clipping demonstrably acts
    assert got['coef'][0] < 0.26
    ref = _train(kind, opt, by_hand=max_norm)
    init = _build(kind).flat.detach().clone()
    moved = float((got['flat'] - init).abs().max())
    diff = (got['flat'] - ref['flat']).abs()
    print(f'{kind} {opt}: moved {moved:.3e}, diff max {float(diff.max()):.3e} mean {float(diff.mean()):.3e}')
    assert not torch.equal(got['flat'], plain['flat'])
    if opt == 'Adam':
        # the bars of test_gpu_dp_step.py for fp32 summation-order noise through Adam's quotient
        assert moved > 1e-3
        assert float(diff.max()) <= 2e-5, (float(diff.max()), int(diff.argmax()))
        assert float(diff.mean()) <= 1e-7, float(diff.mean())
    else:
        assert moved > 0.0
        assert float(diff.max()) <= 1e-5 * moved, (float(diff.max()), moved)     # SGD's update is linear in g


@pytest.mark.parametrize('opt', ['Adam', 'SGD'])
def test_value_mode_equals_the_gradient_clamped_by_hand(opt):
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    kind = 'transformer'
    probe = NativeTrainer(_build(kind).to(DEV))
    _backward(probe, _to_dev(_batches(kind, False)[0]))
    clip_value = 0.1 * float(probe.model.grad_flat().abs().max())          # a tenth of the first gradient's largest element: some are clamped
    flats = {}
    for mode in ('kernel', 'hand'):
        model = _build(kind).to(DEV)
        clip = dict(gradient_clip_val=clip_value, gradient_clip_algorithm='value') if mode == 'kernel' else {}
        tr = NativeTrainer(model, lr=LR[opt], optimizer=opt, **clip)
        for batch in _batches(kind, False):
            _backward(tr, _to_dev(batch))
            g = model.grad_flat()
            assert int((g.abs() > clip_value).sum()) > 0
            if mode == 'hand':
                g.clamp_(-clip_value, clip_value)
            tr.apply_optimizer()
        assert tr.last_grad_norm is None and tr.last_clip_coef is None      # no norm is taken by value, as in Lightning
        flats[mode] = model.flat.detach().cpu().clone()
    assert torch.equal(_bits(flats['kernel']), _bits(flats['hand']))       # one process: grad_scale is 1, so the clamp is the same arithmetic


@pytest.mark.parametrize('opt', ['Adam', 'SGD'])
def test_error_if_nonfinite(opt):
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    kind = 'transformer'
    batch = _to_dev(_batches(kind, False)[0])
    model = _build(kind).to(DEV)
    tr = NativeTrainer(model, lr=LR[opt], optimizer=opt, gradient_clip_val=1.0, error_if_nonfinite=True)
    tr.step(batch)                                                   # a finite step passes
    before, count = model.flat.detach().clone(), tr.step_count
    assert count == 1
    _backward(tr, batch)
    model.grad_flat()[5] = float('nan')
    with pytest.raises(RuntimeError):
        tr.apply_optimizer()
    torch.cuda.synchronize()
    assert tr.step_count == count and torch.equal(_bits(model.flat), _bits(before))
    tr.error_if_nonfinite = False                                    # the same gradient, torch's default: it propagates
    tr.apply_optimizer()
    assert torch.isnan(tr.last_grad_norm) and torch.isnan(tr.last_clip_coef)
    assert tr.step_count == count + 1 and bool(torch.isnan(model.flat).any())


# ---- two ranks on cuda:0 over gloo ------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_dir, max_norm, schedule):
    import torch.distributed as dist
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer, shard_batch
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    model = _build('transformer').to(DEV)
    tr = NativeTrainer(model, lr=1e-3, optimizer='Adam', exchange_schedule=schedule, gradient_clip_val=max_norm)
    norms, coefs = [], []
    for batch in _batches('transformer', False):
        tr.step(_to_dev(shard_batch(batch, rank, world)))
        norms.append(tr.last_grad_norm.clone())
        coefs.append(tr.last_clip_coef.clone())
    torch.cuda.synchronize()
    assert tr.world == world and tr.exchange_schedule == schedule and tr.model._grad_hook is not None
    torch.save({'flat': model.flat.detach().cpu(), 'norms': torch.stack(norms).cpu(), 'coefs': torch.stack(coefs).cpu()},
               os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('schedule', ['allreduce', 'rs_ag'])
def test_two_ranks_clip_alike_and_equal_the_single_process_step(tmp_path, schedule):
    import torch.multiprocessing as mp
    single = _clipped('transformer', 'Adam')
    max_norm = 0.25 * _unclipped('transformer', 'Adam')['raw'][0]
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), max_norm, schedule), nprocs=2, join=True)
    r0, r1 = torch.load(os.path.join(tmp_path, 'r0.pt')), torch.load(os.path.join(tmp_path, 'r1.pt'))
    assert torch.equal(_bits(r0['norms']), _bits(r1['norms']))       # no collective for the norm: the same buffer, the same order
    assert torch.equal(_bits(r0['flat']), _bits(r1['flat']))
    assert bool((r0['coefs'] < 1.0).all()), r0['coefs']
    diff = (r0['flat'] - single['flat']).abs()
    print(f'{schedule}: norms {r0["norms"].tolist()} single {[float(x) for x in single["norm"]]} diff max {float(diff.max()):.3e} '
          f'mean {float(diff.mean()):.3e}')
    assert float(diff.max()) <= 2e-5, (float(diff.max()), int(diff.argmax()))
    assert float(diff.mean()) <= 1e-7, float(diff.mean())
