"""CPU pins of tests/norm_oracle.py, the fp64 reference that tests/test_gpu_norm_regimes.py compares the kernels of csrc/norm.hip with: against
torch's own layer_norm under autograd and oracle.restatement, the packed and two-part embedding sums against a per-row loop, the width table
against the dispatch ladder, and the tolerances against what fp32 arithmetic itself costs on every case."""
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests import norm_oracle as O

ACTS = [torch.float32, torch.bfloat16]


def test_layer_norm_against_torch_autograd():
    D, rows, eps = 52, 23, 1e-5
    i = O.ln_inputs(D, rows, torch.float32)
    got_f = O.ln_fwd_reference(i['x'], i['gamma'], i['beta'], eps)
    got_b = O.ln_bwd_reference(i['x'], i['gamma'], i['beta'], eps, dy=i['dy'], dlogit=i['dlogit'][:, :3], head_w=i['head_w'][:3])
    x, g, b = (t.double().requires_grad_(True) for t in (i['x'], i['gamma'], i['beta']))
    y = F.layer_norm(x, (D,), g, b, eps)
    sc = F.linear(y, i['head_w'][:3].double())
    want = torch.autograd.grad((y * i['dy'].double()).sum() + (sc * i['dlogit'][:, :3].double()).sum(), [x, g, b])
    assert torch.allclose(got_f['y'], y.detach(), rtol=0, atol=1e-13)
    assert torch.allclose(got_f['y'], R.layer_norm(i['x'].double(), i['gamma'].double(), i['beta'].double(), eps), rtol=0, atol=1e-14)
    assert torch.allclose(got_f['mean'], i['x'].double().mean(-1), rtol=0, atol=1e-15)
    assert torch.allclose(got_f['rstd'], 1 / torch.sqrt(i['x'].double().var(-1, unbiased=False) + eps), rtol=1e-13, atol=0)
    for name, w in zip(('dx', 'dgamma', 'dbeta'), want):
        assert float(w.abs().max()) > 0
        assert float((got_b[name] - w).abs().max()) <= 1e-12 * float(w.abs().max()), name
    # either term alone, and the head against a matrix product
    only_dy = O.ln_bwd_reference(i['x'], i['gamma'], i['beta'], eps, dy=i['dy'])
    only_h = O.ln_bwd_reference(i['x'], i['gamma'], i['beta'], eps, dlogit=i['dlogit'][:, :3], head_w=i['head_w'][:3])
    for name in ('dx', 'dgamma', 'dbeta'):
        assert float((only_dy[name] + only_h[name] - got_b[name]).abs().max()) <= 1e-12 * float(got_b[name].abs().max()), name
    hr = O.head_reference(i['x'], i['head_w'], i['head_b'], i['dlogit'])
    assert torch.allclose(hr['scores'], i['x'].double() @ i['head_w'].double().t() + i['head_b'].double(), rtol=0, atol=1e-13)
    assert torch.allclose(hr['dw'], i['dlogit'].double().t() @ i['x'].double(), rtol=0, atol=1e-12)
    assert torch.allclose(hr['dx'], i['dlogit'].double() @ i['head_w'].double(), rtol=0, atol=1e-13)
    assert torch.allclose(hr['dx'], O.head_transposed(i['dlogit'].double(), i['head_w'].double()), rtol=0, atol=1e-13)
    assert torch.allclose(hr['db'], i['dlogit'].double().sum(0), rtol=0, atol=1e-13)


@pytest.mark.parametrize('pos_offset', [0, 2])
def test_embedding_sum_against_a_row_loop(pos_offset):
    B, L, D1, D2 = 3, 5, 4, 8
    g = torch.Generator().manual_seed(1)
    x, x2 = torch.randn(B, L, D1, generator=g, dtype=torch.float64), torch.randn(B, L, D2, generator=g, dtype=torch.float64)
    pos, typ = torch.randn(L + 3, D1 + D2, generator=g, dtype=torch.float64), torch.randn(D1 + D2, generator=g, dtype=torch.float64)
    lengths = [5, 1, 3]
    rs = O.pack_rows(lengths, L)
    assert rs.tolist() == [0, 1, 2, 3, 4, 5, 10, 11, 12]
    want = []
    for b, n in enumerate(lengths):
        for i in range(n):
            row = torch.tensor(x[b, i].tolist() + x2[b, i].tolist(), dtype=torch.float64)
            want.append((row + pos[pos_offset + i]) + typ)
    got = O.embed_sum(x, pos, pos_offset, typ, row_src=rs, x2=x2)
    assert torch.equal(got, torch.stack(want))
    padded = O.embed_sum(x, pos, pos_offset, typ, x2=x2)
    assert padded.shape == (B * L, D1 + D2) and torch.equal(padded[rs.long()], got)
    one = O.embed_sum(torch.cat([x, x2], -1), pos, pos_offset, typ)
    assert torch.equal(one, padded)
    # the position-table accumulation, packed against padded with zero rows past each length
    dpre = torch.randn(B * L, D1, generator=g, dtype=torch.float64)
    valid = torch.zeros(B * L, dtype=torch.bool)
    valid[rs.long()] = True
    dpos0 = torch.randn(L + 3, D1, generator=g, dtype=torch.float64)
    row0 = torch.tensor([0, 5, 6])
    a = O.embed_bwd_reference(dpre[valid], B, L, dpos0, pos_offset, row0=row0, lengths=torch.tensor(lengths))
    b = O.embed_bwd_reference(dpre * valid[:, None], B, L, dpos0, pos_offset)
    assert torch.allclose(a, b, rtol=0, atol=1e-14) and not torch.equal(a, dpos0)
    assert torch.equal(a[:pos_offset], dpos0[:pos_offset]) and torch.equal(a[pos_offset + L:], dpos0[pos_offset + L:])


def test_width_table_reaches_every_dispatch_regime():
    """if the dispatch ladder of norm.hip changes, update norm_oracle.pick_nv and give WIDTHS a width for every new regime"""
    seen = {O.regime(D)[:2] for D in O.WIDTHS}
    for nv in (1, 2, 4, 7, 8, 16):
        assert (nv, True) in seen, f'WIDTHS needs D = {nv * 256} (NV = {nv}, FULL)'
        assert (nv, False) in seen, f'WIDTHS needs a width of NV = {nv} that is no multiple of 256'
    assert all(nv in (1, 2, 4, 7, 8, 16) for nv, _ in seen), 'a new NV: the table needs a width for it'
    # every width up to 4096 lands on a listed NV, and the ladder is the smallest listed NV that holds the row (7 only for seven slots)
    for D in range(4, 4097, 4):
        nv, need = O.pick_nv(D), -(-D // 256)
        assert nv == (7 if need == 7 else min(v for v in (1, 2, 4, 8, 16) if v >= need)), D
    wide = [D for D in O.WIDTHS if O.regime(D)[2]]
    assert any(D % 2048 and D < 4096 for D in wide) and 4096 in wide, 'both WIDE shapes: a ragged second chunk and two full chunks'
    assert any(D % 256 and D - (D // 256) * 256 <= 4 and O.pick_nv(D) > -(-D // 256) for D in O.WIDTHS), 'a width with a wholly idle last slot'
    assert 768 in O.WIDTHS and 4 in O.WIDTHS
    assert all(O.pick_nv(D) == 0 or D % 4 for D in O.REFUSED_WIDTHS)
    assert all(O.pick_nv(D) > 8 for D in O.EMBED_BWD_REFUSED_WIDTHS)
    cases = O.ln_cases()
    assert len(cases) == len(set(cases)) == 2 * len(O.WIDTHS) + 2 * len(O.EDGE_WIDTHS)
    assert all(set(O.EDGE_WIDTHS) <= set(w) for w in (O.WIDTHS, O.STALE_WIDTHS))
    assert max(r * D * 4 for D, r in cases) <= 34e6
    assert all(d1 % 4 == 0 and d2 % 4 == 0 for d1, d2 in O.EMBED_SPLITS)
    assert len(O.pack_rows(O.EMBED_LENGTHS, O.EMBED_L)) % 4 != 0


HALF = 0.5


@pytest.mark.parametrize('act', ACTS, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('D,rows', O.ln_cases())
def test_fp32_restatement_of_layernorm_within_half_the_tolerance(D, rows, act):
    """the formulas in fp32 on the CPU against fp64: forward with the widest head, backward with dy + the widest head and with a 3-tag head alone"""
    i = O.ln_inputs(D, rows, act)
    ref, r32 = (O.ln_fwd_reference(i['x'], i['gamma'], i['beta'], O.EPS, dt) for dt in (torch.float64, torch.float32))
    for k in ('y', 'mean', 'rstd'):
        assert O.excess32(r32[k], ref[k]) <= HALF, (k, O.excess32(r32[k], ref[k]))
    ys = O.stored(ref['y'], act)                                     # the head reads what was stored
    sc = O.head(ys, i['head_w'].double(), i['head_b'].double())
    sc32 = O.head(ys.float(), i['head_w'], i['head_b'])
    assert O.excess32(sc32, sc) <= HALF, ('scores', O.excess32(sc32, sc))
    for dy, n in ((i['dy'], 4), (None, 3)):
        kw = dict(dy=dy, dlogit=i['dlogit'][:, :n], head_w=i['head_w'][:n])
        ref, r32 = (O.ln_bwd_reference(i['x'], i['gamma'], i['beta'], O.EPS, dtype=dt, **kw) for dt in (torch.float64, torch.float32))
        for k in ('dx', 'dgamma', 'dbeta'):
            assert O.excess32(r32[k], ref[k]) <= HALF, (k, n, O.excess32(r32[k], ref[k]))
        dxs = O.stored(ref['dx'], act)                               # dxsum: the column sum of what was stored
        assert O.excess32(dxs.float().sum(0), dxs.sum(0)) <= HALF, 'dxsum'


@pytest.mark.parametrize('act', ACTS, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('D,D1', [(D, None) for D in O.EMBED_WIDTHS] + [(a + b, a) for a, b in O.EMBED_SPLITS])
def test_fp32_restatement_of_the_embedding_block_within_half_the_tolerance(D, D1, act):
    i = O.embed_inputs(D, act, D1)
    for pos_offset in O.EMBED_POS_OFFSETS:
        for rs in (None, i['row_src']):
            args = (i['x'], i['pos'], pos_offset, i['type0'], i['gamma'], i['beta'], O.EPS, act)
            ref = O.embed_fwd_reference(*args, row_src=rs, x2=i.get('x2'))
            r32 = O.embed_fwd_reference(*args, row_src=rs, x2=i.get('x2'), dtype=torch.float32)
            assert O.excess32(r32['pre'], ref['pre']) <= HALF
            # statistics and y of the SAME stored pre (see the module's header)
            same = O.ln_fwd_reference(O.stored(ref['pre'], act), i['gamma'], i['beta'], O.EPS, torch.float32)
            for k in ('y', 'mean', 'rstd'):
                assert O.excess32(same[k], ref[k]) <= HALF, k


@pytest.mark.parametrize('act', ACTS, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('rows', O.HEAD_ROWS)
@pytest.mark.parametrize('D', O.HEAD_WIDTHS)
def test_fp32_restatement_of_the_head_within_half_the_tolerance(D, rows, act):
    i = O.head_inputs(D, rows, act)
    ref, r32 = (O.head_reference(i['x'], i['w'], i['b'], i['ds'], dt) for dt in (torch.float64, torch.float32))
    for k in ('scores', 'dx', 'dw', 'db'):
        assert O.excess32(r32[k], ref[k]) <= HALF, k
    acc = i['dx_old'].double() + ref['dx']
    assert O.excess32(i['dx_old'].float() + r32['dx'], acc) <= HALF


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('B', O.EMBED_BWD_BS)
def test_fp32_restatement_of_the_position_sum_within_half_the_tolerance(B, packed):
    for D in O.EMBED_BWD_WIDTHS:
        for act in ACTS:
            i = O.embed_bwd_inputs(B, D, act, packed)
            args = (i['dpre'], B, O.EMBED_BWD_L, i['dpos0'], 2)
            ref = O.embed_bwd_reference(*args, row0=i['row0'], lengths=i['lengths'])
            r32 = O.embed_bwd_reference(*args, row0=i['row0'], lengths=i['lengths'], dtype=torch.float32)
            assert O.excess32(r32, ref) <= HALF
            if packed:
                assert int(i['lengths'][0]) == O.EMBED_BWD_L and (B == 1 or int(i['lengths'][1]) == 1)
