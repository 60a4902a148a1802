"""fp64 reference of the row-wise kernels of csrc/norm.hip (embedding sum + LayerNorm, LayerNorm forward / backward with the fused tagger head,
the stand-alone head, the position-table accumulation) and the case tables that tests/test_gpu_norm_regimes.py runs them at.  Plain torch, written
from the operations themselves; it never calls the library, and the backward is autograd.  Every function works on whatever device its
arguments live on and uses elementwise operations and reductions only.

    LayerNorm       y = (x - mean) / sqrt(var + eps) * gamma + beta, biased variance over the last dim; rstd = 1 / sqrt(var + eps)
    embedding sum   pre[r] = (x[src] + pos[pos_offset + src % L]) + type0, src = r (padded) or row_src[r] (packed); x | x2 is an explicit cat
    head            scores = y @ w.T + b
    storage         with bf16 activations the kernels normalise the `pre` they STORED and feed the fused head the `y` they STORE.  One fp32
                    rounding next to a bf16 rounding boundary moves a stored element by a whole bf16 ulp (2^-8 relative), and at D = 64 one such
                    element moves the row mean by 1e-4: so in bf16 the statistics / y reference is computed from the stored `pre`, and the score
                    reference from the stored `y`, while `pre` and `y` themselves are compared with fp64 under rule (ii) below.

Tolerances (fixed before any kernel was run against them; tests/test_norm_oracle_cpu.py checks that the same formulas evaluated in fp32 on the
CPU stay within HALF of them on every case, so none is tighter than fp32 arithmetic allows):
    rule (i)   computed and stored in fp32:  max|got - ref| <= TOL * max(1, max|ref|), TOL = 2e-5 (the bound of tests/test_gpu_norm_fused.py)
    rule (ii)  stored in bf16: the kernel stores the bf16 rounding of an fp32 value v with |v - ref| <= t, t from rule (i), so element by
               element |got - ref| <= t + 2^-8 * (|ref| + t)  (half a bf16 ulp of any value within t of ref)
No case needed a raised bound: RAISED stays empty.
"""
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

EPS = 1e-12
TOL = 2e-5
RAISED: Dict[tuple, Tuple[float, float]] = {}          # (entry point, quantity, D, rows) -> (fp32 restatement error, chosen bound); none needed

# ---------------------------------------------------------------------------------------------------------------- case tables
# every NV of the dispatch ladder with and without FULL, widths whose last 256-column slot is wholly idle (768, 1028, 1540), one live lane (4),
# both WIDE shapes (ragged second chunk: 2052, 2304; two full chunks: 4096)
WIDTHS = [4, 64, 252, 256, 260, 512, 768, 1024, 1028, 1540, 1792, 1796, 2048, 2052, 2304, 4096]
REFUSED_WIDTHS = [66, 4100]                          # no multiple of 4; wider than 16 slots
EMBED_BWD_REFUSED_WIDTHS = [2052]                    # the embedding backward has no two-chunk form
# fewer rows than the 4 waves of a workgroup; a ragged last workgroup; past the 512 x 4 rows of one grid pass, so that SOME waves loop twice;
# past two passes, so that a few loop three times
ROWS_EVERY_WIDTH = [5, 2053]
ROWS_EDGE = [1, 4101]
EDGE_WIDTHS = [64, 1792, 2052]
N_OUTS = [1, 2, 3, 4]

EMBED_B, EMBED_L = 3, 37
EMBED_LENGTHS = [37, 1, 20]                          # packed: n_rows = 58, no multiple of 4
EMBED_POS_OFFSETS = [0, 2]
EMBED_WIDTHS = [64, 516, 768, 1792, 2052]
# (D1, D2) of x | x2: the switch of pointer in the first 16-byte chunk, in the last one, in the middle of a 256-column slot, on a slot boundary
EMBED_SPLITS = [(4, 60), (60, 4), (260, 256), (768, 1024), (1024, 768), (4, 2048)]

EMBED_BWD_BS = [1, 7, 8, 9, 17]                      # either side of the 8-document unrolled loop
EMBED_BWD_L = 19
EMBED_BWD_WIDTHS = [4, 96]

HEAD_WIDTHS = [4, 72, 256, 1792, 2052, 4096]
HEAD_ROWS = [1, 5, 2053]

STALE_WIDTHS = [64, 1792, 2052]
STALE_ROWS = (2053, 5)
STALE_EMBED_SHAPES = ((9, 300), (2, 5))


def ln_cases() -> List[Tuple[int, int]]:
    """(D, rows) of the LayerNorm forward / backward table: no cross product"""
    return [(D, r) for D in WIDTHS for r in ROWS_EVERY_WIDTH] + [(D, r) for D in EDGE_WIDTHS for r in ROWS_EDGE]


def pick_nv(D: int) -> int:
    # mirror of norm.hip:pick_nv; update both
    need = -(-D // 256)
    if need <= 1:
        return 1
    if need <= 2:
        return 2
    if need <= 4:
        return 4
    if need == 7:
        return 7
    if need <= 8:
        return 8
    if need <= 16:
        return 16
    return 0


def regime(D: int) -> Tuple[int, bool, bool]:
    """-> (NV, FULL, WIDE) of the LayerNorm kernels at width D (NV = 16 runs the backward as two chunks of NV = 8)"""
    nv = pick_nv(D)
    return nv, D == nv * 256, 2048 < D <= 4096


# ---------------------------------------------------------------------------------------------------------------- the operations
def row_stats(x: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    mean = x.mean(-1)
    var = ((x - mean.unsqueeze(-1)) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + eps)


def layer_norm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float) -> Tensor:
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def head(y: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """y @ w.T + b, one output column at a time"""
    return torch.stack([(y * w[c]).sum(-1) for c in range(w.shape[0])], dim=1) + b


def head_transposed(ds: Tensor, w: Tensor) -> Tensor:
    """ds @ w"""
    out = ds[:, 0:1] * w[0]
    for c in range(1, w.shape[0]):
        out = out + ds[:, c:c + 1] * w[c]
    return out


def embed_sum(x: Tensor, pos: Tensor, pos_offset: int, type0: Tensor, row_src: Optional[Tensor] = None, x2: Optional[Tensor] = None) -> Tensor:
    """x [B, L, D] (| x2 [B, L, D2]) -> pre [rows, D]"""
    B, L = x.shape[:2]
    if x2 is not None:
        x = torch.cat([x, x2], dim=-1)
    flat = x.reshape(B * L, -1)
    src = torch.arange(B * L, device=x.device) if row_src is None else row_src.long()
    return (flat[src] + pos[pos_offset + src % L]) + type0


def stored(t: Tensor, act: torch.dtype) -> Tensor:
    """what a buffer of dtype `act` holds of t, in t's own dtype"""
    return t.to(act).to(t.dtype)


def pack_rows(lengths, L: int) -> Tensor:
    """row_src of the packed form: the valid sentences, document after document"""
    return torch.cat([b * L + torch.arange(int(n)) for b, n in enumerate(lengths)]).to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- references
def ln_fwd_reference(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, dtype=torch.float64) -> Dict[str, Tensor]:
    xv = x.to(dtype)
    mean, rstd = row_stats(xv, eps)
    return dict(y=layer_norm(xv, gamma.to(dtype), beta.to(dtype), eps), mean=mean, rstd=rstd)


def ln_bwd_reference(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, dy: Optional[Tensor] = None, dlogit: Optional[Tensor] = None,
                     head_w: Optional[Tensor] = None, dtype=torch.float64) -> Dict[str, Tensor]:
    """gradients of sum(y * dy) + sum(head(y) * dlogit) wrt x, gamma, beta by autograd; either term may be absent"""
    xv, gv, bv = (t.detach().to(dtype).requires_grad_(True) for t in (x, gamma, beta))
    y = layer_norm(xv, gv, bv, eps)
    obj = y.new_zeros(())
    if dy is not None:
        obj = obj + (y * dy.to(dtype)).sum()
    if head_w is not None:
        w = head_w.to(dtype)
        obj = obj + (head(y, w, w.new_zeros(w.shape[0])) * dlogit.to(dtype)).sum()
    dx, dg, db = torch.autograd.grad(obj, [xv, gv, bv])
    return dict(dx=dx, dgamma=dg, dbeta=db)


def embed_fwd_reference(x, pos, pos_offset, type0, gamma, beta, eps, act, row_src=None, x2=None, dtype=torch.float64) -> Dict[str, Tensor]:
    """`pre` before storage, and y / mean / rstd of the storage rounding of that `pre` (identity for fp32 activations)"""
    pre = embed_sum(x.to(dtype), pos.to(dtype), pos_offset, type0.to(dtype), row_src, None if x2 is None else x2.to(dtype))
    out = ln_fwd_reference(stored(pre, act), gamma, beta, eps, dtype)
    out['pre'] = pre
    return out


def embed_bwd_reference(dpre: Tensor, B: int, L: int, dpos0: Tensor, pos_offset: int, row0=None, lengths=None, dtype=torch.float64) -> Tensor:
    """dpos0 with sum_b dpre[b, i] added to row pos_offset + i.  padded: dpre [B * L, D]; packed: document b owns rows row0[b] .. + lengths[b] - 1"""
    out = dpos0.to(dtype).clone()
    d = dpre.to(dtype)
    for b in range(B):
        n, r0 = (L, b * L) if row0 is None else (int(lengths[b]), int(row0[b]))
        out[pos_offset:pos_offset + n] += d[r0:r0 + n]
    return out


def embed_ln_bwd_reference(pre: Tensor, dh: Tensor, gamma: Tensor, eps: float, B: int, L: int, dtype=torch.float64) -> Dict[str, Tensor]:
    """backward of the embedding block on a padded batch: the LayerNorm's parameter gradients, and its input gradient summed over every row
    (token-type row) and over the documents of each position (position table)"""
    r = ln_bwd_reference(pre, gamma, torch.zeros_like(gamma), eps, dy=dh, dtype=dtype)
    dpre = r['dx']
    return dict(dgamma=r['dgamma'], dbeta=r['dbeta'], dtype0=dpre.sum(0), dpos=dpre.view(B, L, -1).sum(0))


def head_reference(x: Tensor, w: Tensor, b: Tensor, ds: Tensor, dtype=torch.float64) -> Dict[str, Tensor]:
    """scores and the gradients of sum(scores * ds) by autograd"""
    xv, wv, bv = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    scores = head(xv, wv, bv)
    dx, dw, db = torch.autograd.grad((scores * ds.to(dtype)).sum(), [xv, wv, bv])
    return dict(scores=scores.detach(), dx=dx, dw=dw, db=db)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 10007 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


def ln_inputs(D: int, rows: int, act: torch.dtype, salt: int = 0) -> Dict[str, Tensor]:
    """CPU tensors; x and dy in the activation dtype, everything else fp32"""
    g = _gen(D, rows, salt)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=(r(rows, D) * 1.7 + 0.3).to(act), gamma=1 + 0.1 * r(D), beta=0.1 * r(D), dy=r(rows, D).to(act), head_w=r(4, D) / D ** 0.5, head_b=r(4),
                dlogit=r(rows, 4))


def embed_inputs(D: int, act: torch.dtype, D1: Optional[int] = None) -> Dict[str, Tensor]:
    g = _gen(D, 77, D1 or 0)
    r = lambda *s: torch.randn(*s, generator=g)
    B, L = EMBED_B, EMBED_L
    x = r(B, L, D)
    d = dict(pos=0.5 * r(L + 5, D), type0=0.5 * r(D), gamma=1 + 0.1 * r(D), beta=0.1 * r(D), row_src=pack_rows(EMBED_LENGTHS, L))
    if D1 is None:
        d['x'] = x
    else:
        d['x'], d['x2'] = x[..., :D1].contiguous(), x[..., D1:].contiguous()
    return d


def head_inputs(D: int, rows: int, act: torch.dtype, salt: int = 0) -> Dict[str, Tensor]:
    g = _gen(D, rows, 5, salt)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(rows, D).to(act), w=r(4, D) / D ** 0.5, b=r(4), ds=r(rows, 4), dx_old=r(rows, D).to(act))


def embed_bwd_inputs(B: int, D: int, act: torch.dtype, packed: bool) -> Dict[str, object]:
    """packed: lengths with one document of length L (the first) and, from two documents on, one of length 1 (the second)"""
    g = _gen(B, D, 9, int(packed))
    L = EMBED_BWD_L
    d: Dict[str, object] = dict(dpos0=torch.randn(L + 5, D, generator=g) + 3.0)
    if packed:
        lengths = torch.randint(1, L + 1, (B,), generator=g)
        lengths[0] = L
        if B > 1:
            lengths[1] = 1
        row0 = torch.zeros(B, dtype=torch.int64)
        row0[1:] = torch.cumsum(lengths, 0)[:-1]
        d.update(lengths=lengths, row0=row0, n=int(lengths.sum()))
    else:
        d.update(lengths=None, row0=None, n=B * L)
    d['dpre'] = torch.randn(d['n'], D, generator=g).to(act)
    return d


# ---------------------------------------------------------------------------------------------------------------- tolerances
def bound32(ref: Tensor, key: Optional[tuple] = None) -> float:
    """rule (i)"""
    if key is not None and key in RAISED:
        return RAISED[key][1]
    return TOL * max(1.0, float(ref.abs().max()))


def excess32(got: Tensor, ref: Tensor, key: Optional[tuple] = None) -> float:
    """largest error as a fraction of the rule (i) bound (NaN counts as infinite)"""
    err = (got.double() - ref.double()).abs()
    err = torch.nan_to_num(err, nan=float('inf'))
    return float(err.max()) / bound32(ref, key)


def excess16(got: Tensor, ref: Tensor, key: Optional[tuple] = None) -> float:
    """rule (ii): largest error as a fraction of its element's bound"""
    ref = ref.double()
    t = bound32(ref, key)
    err = torch.nan_to_num((got.double() - ref).abs(), nan=float('inf'))
    return float((err / (t + 2.0 ** -8 * (ref.abs() + t))).max())


def excess(got: Tensor, ref: Tensor, key: Optional[tuple] = None) -> float:
    """by the dtype the result is stored in"""
    return excess16(got, ref, key) if got.dtype == torch.bfloat16 else excess32(got, ref, key)
