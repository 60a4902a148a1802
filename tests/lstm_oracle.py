"""fp64 reference, per-form restatement, case table and bounds of the LSTM recurrence kernels (csrc/lstm.hip, lstm_pair.hip, lstm_mfma.hip) behind
mts_lstm_fwd / mts_lstm_bwd.  Plain torch on the CPU; it never calls the library.  tests/test_lstm_oracle_cpu.py pins what is here,
tests/test_gpu_lstm_forms.py runs the table on the kernels.

Five recurrence forms sit behind the two entry points (expected_form restates the dispatch):
    generic      lstm_fwd_kernel<T> / lstm_bwd_kernel<T>: fp32 and bf16 activations, W_hh in fp32; H != 256, fp32 at H = 256 under lstm_parts = 2
    quad_bf16    CU-quad kernels, bf16, H = 256, the default; W_hh in bf16; partner partials of dh travel as bf16
    quad_fp32    CU-quad kernels, fp32, H = 256, the default; W_hh in fp32
    pair_bf16    CU-pair kernels, bf16, H = 256, lstm_parts = 2; W_hh in bf16; the partner's partial of dh travels as bf16
    mfma_bf16    persistent MFMA kernels, bf16, H = 256, only with MTS_LSTM_PAIR=0; W_hh in bf16

reference(case)     the exact recurrence in fp64: `out` and, by autograd, dxproj and dW_hh from oracle.restatement.lstm_direction (the per-document
                    statement of the semantics); the post-activation gates and the cells from a batched recurrence of its own (states64), which the
                    CPU test holds against the per-document one.  Lengths are clamped to 0..L first: that is the contract of mts.h.
restatement(...)    what a form is SUPPOSED to compute, from the comments and contracts of its kernels: fp64 arithmetic with a rounding at every place
                    the kernels store a value -- W_hh to bf16 for the three bf16 matrix-core forms; h to the activation dtype at every step; the gates
                    in the activation dtype, re-read by the backward; the cells in fp32; dxproj to the activation dtype before it propagates; the
                    partials of dh that the pair / quad bf16 backward hands to its partner workgroups in bf16; dW_hh as an fp32 value of the sum over
                    the rounded operands.  It models neither the v_exp / v_rcp activations nor an fp32 order of accumulation.
                    `mutant` plants one subtle error (MUTANTS).
saved_state_index   where each form keeps the gates and cells of a valid row: row-major as mts.h documents it for the generic and MFMA kernels (the
                    CU-pair and fp32 CU-quad kernels write the same layout), step-major blocks for the bf16 CU-quad kernels.  The GPU test reads the
                    saved state of every form through it.  That proves which kernels ran (a run of the bf16 CU-quad kernels cannot pass as the MFMA
                    form, nor the reverse), and it is the only place where cells rounded to bf16 show: through out, dxproj and dW_hh that error is
                    of the size of the bf16 storage roundings themselves (1 to 4 t on documents of 32 to 128 sentences, forget bias up to +4), so
                    no margin that leaves room for the kernels separates it there.

Bounds.
    fp32 cases      the bounds the suite already holds these kernels to, rtol / atol against fp64: out 1e-5 / 1e-5, dxproj 1e-4 / 2e-5, dW_hh
                    1e-4 / 1e-4.  gates and cells (both O(1) like out, one step of the same arithmetic) take out's.
    bf16 cases      nothing chosen in advance.  T[case id][quantity] is the largest error of the mutant-free restatement against the fp64 reference,
                    measured on the CPU (never against the kernels); a quantity stored in bf16 (out, dxproj, gates) is held, element by element, to
                    rule (ii) of norm_oracle.py, |got - ref| <= M t + 2^-8 (|ref| + M t); a quantity stored in fp32 (cells, dW_hh) has no storage
                    rounding of its own to allow for and is held to |got - ref| <= M t.
    margin          M = 4: the restatement leaves out the fast activations and the accumulation order, both far below one bf16 ulp but able to flip
                    a rounding that later steps amplify.  tests/test_lstm_oracle_cpu.py accepts M only because every mutant lies OUTSIDE the bound on
                    at least one case of every form it applies to.  b_hh is drawn at scale 0.5 (not the 0.1 of the older tests) so that a bias
                    dropped on one gate stands clear of the bound.
    RAISED          (case id, quantity) -> (measured t, chosen bound) for a case that needed a bound of its own; none did.
"""
import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from oracle import restatement as R

FORMS = ('generic', 'quad_bf16', 'quad_fp32', 'pair_bf16', 'mfma_bf16')
MATRIX_CORE_BF16 = ('quad_bf16', 'pair_bf16', 'mfma_bf16')
GROUP = {'generic': 8, 'quad_bf16': 16, 'quad_fp32': 16, 'pair_bf16': 16, 'mfma_bf16': 16}    # documents per workgroup (set)
M = 4.0
FP32_BOUNDS = {'out': (1e-5, 1e-5), 'dxproj': (1e-4, 2e-5), 'dw_hh': (1e-4, 1e-4), 'gates': (1e-5, 1e-5), 'cells': (1e-5, 1e-5)}
QUANTITIES = ('out', 'gates', 'cells', 'dxproj', 'dw_hh')
STORED_IN_ACT = ('out', 'gates', 'dxproj')
RAISED: Dict[Tuple[str, str], Tuple[float, float]] = {}

MUTANTS = ('drop_b_i', 'drop_b_f', 'drop_b_g', 'drop_b_o', 'swap_f_g', 'reverse_from_L', 'carry_state', 'ct_for_cprev', 'cells_bf16',
           'hprev_first_from_out', 'padded_dxproj')


def expected_form(dtype: torch.dtype, H: int, lstm_parts: int = 4, pair_env: bool = True) -> str:
    """the dispatch of mts_lstm_fwd restated; pair_env False = MTS_LSTM_PAIR=0 in the environment of the calling thread"""
    bf = dtype == torch.bfloat16
    if pair_env and H == 256 and (bf or lstm_parts == 4):          # mts_lstm_pair_supported
        return ('pair_bf16' if lstm_parts == 2 else 'quad_bf16') if bf else 'quad_fp32'
    if bf and H == 256:                                            # mts_lstm_mfma_supported
        return 'mfma_bf16'
    return 'generic'


class Case(NamedTuple):
    id: str
    dtype: torch.dtype
    H: int
    B: int
    L: int
    lengths: Optional[Tuple[int, ...]]      # None: the lengths pointer is NULL
    bias: bool = True                       # False: the b_hh pointer is NULL
    ndir: int = 2
    lstm_parts: int = 4
    pair_env: bool = True
    two_call: bool = False                  # also run mts_lstm_bwd_recurrence + mts_lstm_bwd_whh
    repeat: bool = False                    # also run everything a second time and compare the bits
    refused_bwd: bool = False               # the backward must return MTS_ERR_UNSUPPORTED

    @property
    def form(self) -> str:
        return expected_form(self.dtype, self.H, self.lstm_parts, self.pair_env)

    @property
    def eff_lengths(self) -> List[int]:
        return [self.L] * self.B if self.lengths is None else [max(0, min(int(n), self.L)) for n in self.lengths]


BF, FP = torch.bfloat16, torch.float32
_DT = {BF: 'bf16', FP: 'fp32'}
# 17 documents: two groups of 16, the last with one document; the first group's longest document is odd (9), the second's even (8)
_L17 = (9, 1, 8, 2, 5, 3, 7, 4, 6, 9, 1, 2, 3, 4, 5, 6, 8)
_H256_SETTINGS = [(BF, 4, True), (FP, 4, True), (BF, 2, True), (BF, 4, False), (FP, 2, True)]


def _h256_cases() -> List[Case]:
    out = []
    for dt, parts, env in _H256_SETTINGS:
        f = expected_form(dt, 256, parts, env)
        f = f if f != 'generic' else 'generic_h256'
        kw = dict(dtype=dt, H=256, lstm_parts=parts, pair_env=env)
        out += [Case(f'{f}-B17L9', B=17, L=9, lengths=_L17, two_call=True, **kw),
                Case(f'{f}-B3L8', B=3, L=8, lengths=(8, 7, 2), repeat=True, **kw),
                Case(f'{f}-B16L5-nolengths', B=16, L=5, lengths=None, **kw),
                Case(f'{f}-B5L6-nobias', B=5, L=6, lengths=(6, 3, 1, 5, 2), bias=False, **kw),
                Case(f'{f}-B5L6-ndir1', B=5, L=6, lengths=(6, 3, 1, 5, 2), ndir=1, **kw),
                Case(f'{f}-B6L7-len0', B=6, L=7, lengths=(7, 0, 3, 10, 0, 1), **kw)]
    return out


_L9 = (7, 1, 4, 6, 2, 7, 3, 5, 4)          # LSTM_DG = 8: a full group and a last group of one


def _generic_cases() -> List[Case]:
    out = []
    # H = 25 (odd): the forward runs in both dtypes; the backward's dW_hh GEMM needs rows of 4 fp32 / 8 bf16 elements and is refused.  H = 28 is
    # the smallest neighbour whose fp32 backward runs (a multiple of 4, none of 8).
    for H, dts in ((24, (FP, BF)), (25, (FP,)), (28, (FP,)), (104, (FP, BF)), (1024, (FP,))):
        for dt in dts:
            tag = f'generic-{_DT[dt]}-H{H}'
            if H == 1024:
                out.append(Case(f'{tag}-B9L3', dt, H, 9, 3, (3, 1, 2, 3, 2, 1, 3, 2, 2), two_call=True))
                continue
            sfx = '-refused' if H == 25 else ''
            out += [Case(f'{tag}-B1L7{sfx}', dt, H, 1, 7, (5,), repeat=(H == 24), refused_bwd=(H == 25)),
                    Case(f'{tag}-B9L7{sfx}', dt, H, 9, 7, _L9, two_call=(H not in (25, 104)), refused_bwd=(H == 25))]
    out.append(Case('generic-bf16-H25-B9L7-refused', BF, 25, 9, 7, _L9, refused_bwd=True))
    for dt in (FP, BF):
        tag = f'generic-{_DT[dt]}-H24'
        out += [Case(f'{tag}-B9L7-nolengths', dt, 24, 9, 7, None),
                Case(f'{tag}-B5L6-nobias', dt, 24, 5, 6, (6, 3, 1, 5, 2), bias=False),
                Case(f'{tag}-B5L6-ndir1', dt, 24, 5, 6, (6, 3, 1, 5, 2), ndir=1),
                Case(f'{tag}-B6L7-len0', dt, 24, 6, 7, (7, 0, 3, 10, 0, 1))]
    return out


CASES: List[Case] = _h256_cases() + _generic_cases()
BY_ID = {c.id: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------- inputs
def _shape_key(case: Case):
    return (case.H, case.B, case.L, case.lengths, case.bias, case.ndir)


@functools.lru_cache(maxsize=None)
def _inputs(key) -> Dict[str, Optional[Tensor]]:
    H, B, L, lengths, bias, ndir = key
    g = torch.Generator().manual_seed(1000 * H + 10 * B + L + (0 if bias else 3) + ndir)
    r = lambda *s: torch.randn(*s, generator=g)
    # xproj and dout hold bf16 values in every case, so that the fp32 and the bf16 cases of a shape share one reference
    return dict(xproj=r(B * L, ndir * 4 * H).bfloat16().float(), w_hh=r(ndir, 4 * H, H) / H ** 0.5, b_hh=(0.5 * r(ndir, 4 * H)) if bias else None,
                dout=r(B * L, ndir * H).bfloat16().float())


def inputs(case: Case) -> Dict[str, Optional[Tensor]]:
    """CPU fp32 tensors (xproj and dout exactly representable in bf16); treat them as read-only"""
    return _inputs(_shape_key(case))


# ---------------------------------------------------------------------------------------------------------------- reference
def _positions(lens: Tensor, L: int, s: int, reverse: bool):
    t = (lens - 1 - s) if reverse else torch.full_like(lens, s)
    return t.clamp(0, L - 1), s < lens


def states64(xp: Tensor, lens: Tensor, w: Tensor, b: Tensor, reverse: bool):
    """one direction, batched over the documents, fp64: out [B, L, H], gates [B, L, 4H] (post-activation i, f, g, o), cells [B, L, H]"""
    B, L, _ = xp.shape
    H = w.shape[1]
    out, gates, cells = xp.new_zeros(B, L, H), xp.new_zeros(B, L, 4 * H), xp.new_zeros(B, L, H)
    h, c = xp.new_zeros(B, H), xp.new_zeros(B, H)
    idx = torch.arange(B)
    for s in range(int(lens.max()) if B else 0):
        t, act = _positions(lens, L, s, reverse)
        pre = xp[idx, t] + b + h @ w.t()
        gi, gf, gg, go = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        cn = gf * c + gi * gg
        hn = go * torch.tanh(cn)
        m = act.unsqueeze(1)
        c, h = torch.where(m, cn, c), torch.where(m, hn, h)
        out[idx[act], t[act]], cells[idx[act], t[act]] = hn[act], cn[act]
        gates[idx[act], t[act]] = torch.cat([gi, gf, gg, go], 1)[act]
    return out, gates, cells


@functools.lru_cache(maxsize=None)
def _reference(key) -> Dict[str, Tensor]:
    H, B, L, lengths, bias, ndir = key
    inp = _inputs(key)
    lens = torch.tensor([L] * B if lengths is None else [max(0, min(int(n), L)) for n in lengths])
    xp = inp['xproj'].double().view(B, L, ndir * 4 * H).requires_grad_(True)
    whh = inp['w_hh'].double().requires_grad_(True)
    bhh = inp['b_hh'].double() if bias else torch.zeros(ndir, 4 * H, dtype=torch.float64)
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
    out = torch.cat([R.lstm_direction(xp[:, :, d * 4 * H:(d + 1) * 4 * H], lens, eye, whh[d], zero, bhh[d], d == 1) for d in range(ndir)], dim=2)
    dx, dw = torch.autograd.grad((out * inp['dout'].double().view(B, L, ndir * H)).sum(), [xp, whh])
    st = [states64(xp.detach()[:, :, d * 4 * H:(d + 1) * 4 * H], lens, whh.detach()[d], bhh[d], d == 1) for d in range(ndir)]
    return dict(out=out.detach().reshape(B * L, ndir * H), dxproj=dx.reshape(B * L, ndir * 4 * H), dw_hh=dw,
                gates=torch.cat([s[1] for s in st], 2).reshape(B * L, ndir * 4 * H), cells=torch.cat([s[2] for s in st], 2).reshape(B * L, ndir * H),
                out_batched=torch.cat([s[0] for s in st], 2).reshape(B * L, ndir * H))


def reference(case: Case) -> Dict[str, Tensor]:
    """fp64: out [B*L, ndir*H], gates [B*L, ndir*4H], cells [B*L, ndir*H], dxproj [B*L, ndir*4H], dw_hh [ndir, 4H, H]; shared, read-only"""
    return _reference(_shape_key(case))


def valid_rows(case: Case) -> Tensor:
    """bool [B*L]: row b*L + t with t < len_b"""
    return (torch.arange(case.L).view(1, -1) < torch.tensor(case.eff_lengths).view(-1, 1)).reshape(-1)


def saved_state_index(case: Case) -> Tuple[Tensor, Tensor]:
    """Where the form keeps the saved gates / cells of a valid row: flat element indices, gates [B*L, ndir*4H] and cells [B*L, ndir*H] (entries of
    rows past a document's end are -1).  The generic, persistent-MFMA, CU-pair and fp32 CU-quad kernels store row b*L + t, column d*4H + gate*H + unit
    (cells: d*H + unit).  The bf16 CU-quad kernels keep STEP-MAJOR blocks (lstm_fwd_quad_kernel): the region of a group of 16 documents is the rows of
    its documents, laid out [direction][part of 64 units][step][document < ndg][gate][64 units], ndg = documents present in the group; step s of the
    reverse direction is position len - 1 - s."""
    H, B, L, ndir = case.H, case.B, case.L, case.ndir
    lens = case.eff_lengths
    gi = torch.full((B, L, ndir, 4, H), -1, dtype=torch.long)
    ci = torch.full((B, L, ndir, H), -1, dtype=torch.long)
    unit = torch.arange(H)
    for b in range(B):
        n = lens[b]
        if n == 0:
            continue
        t = torch.arange(n)
        for d in range(ndir):
            if case.form != 'quad_bf16':
                row = (b * L + t).view(n, 1, 1)
                gi[b, :n, d] = row * (ndir * 4 * H) + d * 4 * H + torch.arange(4).view(1, 4, 1) * H + unit.view(1, 1, H)
                ci[b, :n, d] = row.view(n, 1) * (ndir * H) + d * H + unit.view(1, H)
                continue
            hq = H // 4
            gx, doc = divmod(b, 16)
            ndg = min(16, B - gx * 16)
            s = (t if d == 0 else n - 1 - t).view(n, 1, 1)
            p, ul = (unit // hq).view(1, 1, H), (unit % hq).view(1, 1, H)
            blk = (d * 4 + p) * L + s
            gi[b, :n, d] = gx * 16 * L * ndir * 4 * H + blk * (ndg * 4 * hq) + doc * 4 * hq + torch.arange(4).view(1, 4, 1) * hq + ul
            ci[b, :n, d] = (gx * 16 * L * ndir * H + blk * (ndg * hq) + doc * hq + ul).view(n, H)
    return gi.view(B * L, ndir * 4 * H), ci.view(B * L, ndir * H)


def canonical_state(case: Case, gates: Tensor, cells: Tensor) -> Tuple[Tensor, Tensor]:
    """the saved state of a run as [B*L, ndir*4H] / [B*L, ndir*H]; rows past a document's end come back as 0"""
    gi, ci = saved_state_index(case)
    g, c = gates.reshape(-1)[gi.clamp(min=0)], cells.reshape(-1)[ci.clamp(min=0)]
    return torch.where(gi >= 0, g, torch.zeros_like(g)), torch.where(ci >= 0, c, torch.zeros_like(c))


# ---------------------------------------------------------------------------------------------------------------- restatement
def _bf(x: Tensor) -> Tensor:
    return x.bfloat16().double()


def _f32(x: Tensor) -> Tensor:
    return x.float().double()


def _direction(form: str, act_dt, xp, dout, lens, w_hh, b, reverse: bool, mutant: Optional[str], start=None):
    B, L, _ = xp.shape
    H = w_hh.shape[1]
    ra = _bf if act_dt == torch.bfloat16 else _f32
    w = _bf(w_hh) if form in MATRIX_CORE_BF16 else w_hh
    idx = torch.arange(B)
    z = lambda *s: xp.new_zeros(*s)
    run = torch.full_like(lens, L) if (mutant == 'reverse_from_L' and reverse) else lens
    steps = int(run.max()) if B else 0
    # ---- forward
    out, gates, cells = z(B, L, H), z(B, L, 4 * H), z(B, L, H)
    h, c = (z(B, H), z(B, H)) if start is None else start
    for s in range(steps):
        t, act = _positions(run, L, s, reverse)
        pre = (xp[idx, t] + b) + h @ w.t()
        pi, pf, pg, po = pre[:, :H], pre[:, H:2 * H], pre[:, 2 * H:3 * H], pre[:, 3 * H:]
        if mutant == 'swap_f_g':
            pf, pg = pg, pf
        gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
        cn = _f32(gf * c + gi * gg)
        if mutant == 'cells_bf16':
            cn = _bf(cn)
        hn = ra(go * torch.tanh(cn))
        m = act.unsqueeze(1)
        c, h = torch.where(m, cn, c), torch.where(m, hn, h)
        out[idx[act], t[act]], cells[idx[act], t[act]] = hn[act], cn[act]
        gates[idx[act], t[act]] = ra(torch.cat([gi, gf, gg, go], 1))[act]
    final = (h, c)
    # ---- backward
    parts = {'quad_bf16': 4, 'pair_bf16': 2}.get(form, 1)
    dx, hprev = z(B, L, 4 * H), z(B, L, H)
    dh, dc = z(B, H), z(B, H)
    for s in range(steps - 1, -1, -1):
        t, act = _positions(run, L, s, reverse)
        tp = ((t + 1) if reverse else (t - 1)).clamp(0, L - 1)
        g = gates[idx, t]
        gi, gf, gg, go = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        ct = cells[idx, t]
        cp = cells[idx, tp] if s > 0 else z(B, H)
        if mutant == 'ct_for_cprev':
            cp = ct
        tc = torch.tanh(ct)
        dht = dout[idx, t] + dh
        dct = dc + dht * go * (1 - tc * tc)
        da = ra(torch.cat([dct * gg * gi * (1 - gi), dct * cp * gf * (1 - gf), dct * gi * (1 - gg * gg), dht * tc * go * (1 - go)], 1))
        m = act.unsqueeze(1)
        da = torch.where(m, da, z(B, 4 * H))
        dx[idx[act], t[act]] = da[act]
        if s > 0:
            hprev[idx[act], t[act]] = out[idx[act], tp[act]]
        if parts == 1:
            dh_new = da @ w
        else:       # every part reduces over the gate columns of its own units; what it computes for the other parts' units travels as bf16
            hp = H // parts
            dh_new = z(B, H)
            for p in range(parts):
                cols = torch.cat([torch.arange(gt * H + p * hp, gt * H + (p + 1) * hp) for gt in range(4)])
                part = da[:, cols] @ w[cols, :]
                sent = _bf(part)
                sent[:, p * hp:(p + 1) * hp] = part[:, p * hp:(p + 1) * hp]
                dh_new = dh_new + sent
        dh, dc = torch.where(m, dh_new, dh), torch.where(m, dct * gf, dc)
    if run is not lens:                                   # reverse_from_L: the rows past a document's end are still written as zeros
        pad = torch.arange(L).view(1, L) >= lens.view(B, 1)
        out[pad], dx[pad], hprev[pad], gates[pad], cells[pad] = 0, 0, 0, 0, 0
    return out, gates, cells, dx, hprev, final


def restatement(case: Case, form: Optional[str] = None, mutant: Optional[str] = None) -> Dict[str, Tensor]:
    """-> the quantities of reference(), as fp64 tensors holding what the form's buffers are supposed to hold"""
    form = form or case.form
    assert mutant is None or mutant in MUTANTS, mutant
    H, B, L, ndir = case.H, case.B, case.L, case.ndir
    inp = inputs(case)
    lens = torch.tensor(case.eff_lengths)
    xp = inp['xproj'].double().view(B, L, ndir * 4 * H)
    dout = inp['dout'].double().view(B, L, ndir * H)
    res = []
    for d in range(ndir):
        b = inp['b_hh'][d].double().clone() if case.bias else torch.zeros(4 * H, dtype=torch.float64)
        if mutant and mutant.startswith('drop_b_'):
            gt = 'ifgo'.index(mutant[-1])
            b[gt * H:(gt + 1) * H] = 0
        args = (form, case.dtype, xp[:, :, d * 4 * H:(d + 1) * 4 * H], dout[:, :, d * H:(d + 1) * H], lens, inp['w_hh'][d].double(), b, d == 1)
        start = None
        if mutant == 'carry_state':                       # a document starts from the final state of the document before it in its group
            h, c = _direction(*args, None)[5]
            first = (torch.arange(B) % GROUP[form] == 0).unsqueeze(1)
            start = tuple(torch.where(first, torch.zeros_like(v), torch.roll(v, 1, 0)) for v in (h, c))
        res.append(_direction(*args, mutant, start))
    cat = lambda i, wd: torch.cat([r[i] for r in res], 2).reshape(B * L, ndir * wd)
    out, gates, cells, dx, hprev = cat(0, H), cat(1, 4 * H), cat(2, H), cat(3, 4 * H), cat(4, H)
    if mutant == 'hprev_first_from_out':                  # has_prev ignored: the neighbouring ROW of `out`, whatever document it belongs to
        lo = torch.zeros(1, ndir * H, dtype=torch.float64)
        shifted = [torch.cat([lo, out[:-1]]), torch.cat([out[1:], lo])]
        hprev = torch.cat([shifted[d][:, d * H:(d + 1) * H] for d in range(ndir)], 1) * valid_rows(case).unsqueeze(1)
    dw = torch.stack([_f32(dx[:, d * 4 * H:(d + 1) * 4 * H].t() @ hprev[:, d * H:(d + 1) * H]) for d in range(ndir)])
    if mutant == 'padded_dxproj':                         # the rows past a document's end keep what its last step wrote
        d3 = dx.view(B, L, -1)
        for bb, n in enumerate(case.eff_lengths):
            if 0 < n < L:
                d3[bb, n:] = d3[bb, n - 1]
    return dict(out=out, gates=gates, cells=cells, dxproj=dx, dw_hh=dw)


def applies(mutant: str, case: Case) -> bool:
    """whether the planted error can change anything on this case"""
    lens, L = case.eff_lengths, case.L
    if mutant.startswith('drop_b_'):
        return case.bias
    if mutant == 'reverse_from_L':
        return case.ndir == 2 and any(0 < n < L for n in lens)
    if mutant == 'carry_state':
        return any(lens[b] > 0 and lens[b - 1] > 0 for b in range(1, case.B) if b % GROUP[case.form] != 0)
    if mutant == 'padded_dxproj':
        return any(0 < n < L for n in lens)
    if mutant == 'hprev_first_from_out':
        return case.B * L > 1
    return max(lens) > 1 if mutant == 'ct_for_cprev' else True


# ---------------------------------------------------------------------------------------------------------------- bounds
# largest |mutant-free restatement - fp64 reference| of every bf16 case, measured on the CPU with measure_t() and rounded up in the fourth digit;
# tests/test_lstm_oracle_cpu.py measures again and holds the table to it
T: Dict[str, Dict[str, float]] = {
    'quad_bf16-B17L9': dict(out=2.421e-03, gates=3.064e-03, cells=2.213e-03, dxproj=8.654e-03, dw_hh=1.143e-02),
    'quad_bf16-B3L8': dict(out=2.123e-03, gates=2.662e-03, cells=1.546e-03, dxproj=6.716e-03, dw_hh=7.259e-03),
    'quad_bf16-B16L5-nolengths': dict(out=2.328e-03, gates=3.004e-03, cells=1.781e-03, dxproj=9.249e-03, dw_hh=1.492e-02),
    'quad_bf16-B5L6-nobias': dict(out=1.856e-03, gates=2.759e-03, cells=1.382e-03, dxproj=6.986e-03, dw_hh=6.891e-03),
    'quad_bf16-B5L6-ndir1': dict(out=1.999e-03, gates=2.648e-03, cells=1.709e-03, dxproj=7.152e-03, dw_hh=8.367e-03),
    'quad_bf16-B6L7-len0': dict(out=2.116e-03, gates=2.734e-03, cells=1.414e-03, dxproj=8.623e-03, dw_hh=1.034e-02),
    'pair_bf16-B17L9': dict(out=2.421e-03, gates=3.064e-03, cells=2.213e-03, dxproj=8.654e-03, dw_hh=1.270e-02),
    'pair_bf16-B3L8': dict(out=2.123e-03, gates=2.662e-03, cells=1.546e-03, dxproj=6.716e-03, dw_hh=7.121e-03),
    'pair_bf16-B16L5-nolengths': dict(out=2.328e-03, gates=3.004e-03, cells=1.781e-03, dxproj=9.249e-03, dw_hh=1.495e-02),
    'pair_bf16-B5L6-nobias': dict(out=1.856e-03, gates=2.759e-03, cells=1.382e-03, dxproj=7.414e-03, dw_hh=6.891e-03),
    'pair_bf16-B5L6-ndir1': dict(out=1.999e-03, gates=2.648e-03, cells=1.709e-03, dxproj=7.152e-03, dw_hh=8.367e-03),
    'pair_bf16-B6L7-len0': dict(out=2.116e-03, gates=2.734e-03, cells=1.414e-03, dxproj=8.623e-03, dw_hh=1.034e-02),
    'mfma_bf16-B17L9': dict(out=2.421e-03, gates=3.064e-03, cells=2.213e-03, dxproj=8.654e-03, dw_hh=1.275e-02),
    'mfma_bf16-B3L8': dict(out=2.123e-03, gates=2.662e-03, cells=1.546e-03, dxproj=6.716e-03, dw_hh=7.259e-03),
    'mfma_bf16-B16L5-nolengths': dict(out=2.328e-03, gates=3.004e-03, cells=1.781e-03, dxproj=9.249e-03, dw_hh=1.452e-02),
    'mfma_bf16-B5L6-nobias': dict(out=1.856e-03, gates=2.759e-03, cells=1.382e-03, dxproj=7.414e-03, dw_hh=6.998e-03),
    'mfma_bf16-B5L6-ndir1': dict(out=1.999e-03, gates=2.648e-03, cells=1.709e-03, dxproj=7.152e-03, dw_hh=8.367e-03),
    'mfma_bf16-B6L7-len0': dict(out=2.116e-03, gates=2.734e-03, cells=1.414e-03, dxproj=8.623e-03, dw_hh=1.074e-02),
    'generic-bf16-H24-B1L7': dict(out=1.688e-03, gates=2.111e-03, cells=1.022e-03, dxproj=6.491e-03, dw_hh=2.941e-03),
    'generic-bf16-H24-B9L7': dict(out=2.069e-03, gates=2.607e-03, cells=9.586e-04, dxproj=4.460e-03, dw_hh=4.820e-03),
    'generic-bf16-H104-B1L7': dict(out=1.920e-03, gates=2.097e-03, cells=6.667e-04, dxproj=4.745e-03, dw_hh=4.369e-03),
    'generic-bf16-H104-B9L7': dict(out=1.976e-03, gates=2.282e-03, cells=9.513e-04, dxproj=7.668e-03, dw_hh=7.488e-03),
    'generic-bf16-H25-B9L7-refused': dict(out=1.941e-03, gates=2.650e-03, cells=1.301e-03, dxproj=5.403e-03, dw_hh=6.677e-03),
    'generic-bf16-H24-B9L7-nolengths': dict(out=2.069e-03, gates=2.607e-03, cells=1.004e-03, dxproj=6.129e-03, dw_hh=9.042e-03),
    'generic-bf16-H24-B5L6-nobias': dict(out=1.611e-03, gates=2.228e-03, cells=7.446e-04, dxproj=7.260e-03, dw_hh=4.957e-03),
    'generic-bf16-H24-B5L6-ndir1': dict(out=2.005e-03, gates=2.524e-03, cells=5.639e-04, dxproj=4.607e-03, dw_hh=2.453e-03),
    'generic-bf16-H24-B6L7-len0': dict(out=2.052e-03, gates=2.110e-03, cells=1.030e-03, dxproj=5.035e-03, dw_hh=5.626e-03),
}


def measure_t(case: Case) -> Dict[str, float]:
    ref, got = reference(case), restatement(case)
    return {q: float((got[q] - ref[q]).abs().max()) for q in QUANTITIES}


def excess(case: Case, quantity: str, got: Tensor, ref: Optional[Tensor] = None, rows: Optional[Tensor] = None) -> float:
    """largest error of `got` as a fraction of its element's bound (NaN counts as infinite); rows: bool mask of the rows to look at"""
    ref = reference(case)[quantity] if ref is None else ref
    got = got.detach().cpu().double().reshape(ref.shape)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if got.numel() == 0:
        return 0.0
    err = torch.nan_to_num((got - ref).abs(), nan=float('inf'))
    if case.dtype == torch.float32:
        rtol, atol = FP32_BOUNDS[quantity]
        return float((err / (atol + rtol * ref.abs())).max())
    if (case.id, quantity) in RAISED:
        mt = RAISED[(case.id, quantity)][1]
    else:
        mt = M * T[case.id][quantity]
    bound = mt + 2.0 ** -8 * (ref.abs() + mt) if quantity in STORED_IN_ACT else torch.full_like(ref, mt)
    return float((err / bound).max())
