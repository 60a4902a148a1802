"""References and case tables of the flat streaming kernels (csrc/optim.hip: Adam, SGD, their clipped forms, mts_scale, mts_grad_norm; csrc/dropout.hip)
that tests/test_gpu_stream_regimes.py runs them against.  Nothing here touches the GPU or the library; tests/test_stream_oracle_cpu.py pins it.

The library is built with -ffp-contract=off and without fast-math, and HIP's fp32 divide and square root are correctly rounded, so every one of these
kernels except the norm reduction has a reference it must match BIT FOR BIT: the same float32 operations in the same order, in numpy.

    Adam      gr = clip(g * gscale);  m = m + (1 - b1) * (gr - m);  v = b2 * v + ((1 - b2) * gr) * gr;  denom = sqrt(v) / bc2_sqrt + eps;
              p = p - (lr / bc1) * (m / denom);  bc1 = 1 - b1^t and bc2_sqrt = sqrt(1 - b2^t) in double from the float32 betas, then narrowed
    SGD       gr = clip(g * gscale) + wd * p;  b = first ? gr : mom * b + gr;  p = p - lr * b
    clip      norm mode: gr * coef, coef = max_norm / (norm + 1e-6) clamped at 1 with NaN kept;  value mode: clamp to +-c, a NaN stays
    dropout   keep = hash32(seed, index) >= threshold, threshold = uint32(min(2^32 - 1, double(float32(p)) * 2^32));
              y = (keep ? x * scale : 0) + r, scale = float32(1) / (float32(1) - float32(p)), r = 0 without a residual; dx = keep ? dy * scale : 0.
              bf16: widened to float32, the same arithmetic, narrowed ONCE (torch's .to(bfloat16): round to nearest even)
The fp64 references (adam_f64 / sgd_f64) are torch's own optimizers on float64 copies: the bitwise replica and they cannot both drift.
"""
import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- launch constants
THREADS = 256                                        # every kernel here: __launch_bounds__(256)
ADAM_BLOCKS, ADAM_VEC = 2048, 4                      # optim.hip mts_adam_step: blocks = min(2048, (n / 4 + 255) / 256 + 1); adam_loop: 4 per lane
SGD_BLOCKS = 2048                                    # optim.hip mts_sgd_step: blocks = min(2048, (n + 255) / 256)
SCALE_BLOCKS = 1024                                  # optim.hip mts_scale: blocks = min(1024, (n + 255) / 256)
DROPOUT_BLOCKS, DROPOUT_VEC = 4096, 4                # dropout.hip mts_dropout_fwd / _bwd: blocks = min(4096, (n / 4 + 255) / 256)
NORM_BLOCKS, NORM_VEC, NORM_MAX_SPANS = 2048, 4, 4   # optim.hip NORM_MAX_BLOCKS, grad_sumsq_kernel's load4, NORM_MAX_SPANS

# elements of one full grid pass
P_ADAM = ADAM_BLOCKS * THREADS * ADAM_VEC            # 2 097 152
P_SGD = SGD_BLOCKS * THREADS                         # 524 288
P_SCALE = SCALE_BLOCKS * THREADS                     # 262 144
P_DROPOUT = DROPOUT_BLOCKS * THREADS * DROPOUT_VEC   # 4 194 304
P_NORM = NORM_BLOCKS * THREADS * NORM_VEC            # 2 097 152

# ---------------------------------------------------------------------------------------------------------------- size ladders
# scalar tail alone (< one vector), one vector, vector + tail, either side of one workgroup's 1024, the size of the older tests, one grid pass
# exactly, one element into the second trip (tail only), one vector + tail into it, three trips with a tail of 3
ADAM_NS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 10007, P_ADAM, P_ADAM + 1, P_ADAM + 7, 2 * P_ADAM + 4099]
ADAM_CLIP_NS = [10007, P_ADAM + 7, 2 * P_ADAM + 4099]
ADAM_F64_NS = [10007, P_ADAM + 7]
SGD_NS = [1, 255, 256, 257, P_SGD, P_SGD + 1, 2 * P_SGD + 151555]
SGD_F64_NS = [257, P_SGD + 1]
SCALE_NS = [1, 257, P_SCALE, P_SCALE + 1, 2 * P_SCALE + 175713]
DROPOUT_NS = [4, 8, 1020, 1024, 1028, 40960, P_DROPOUT, P_DROPOUT + 4, 2 * P_DROPOUT + 1048580]
DROPOUT_EDGE_NS = [1028, P_DROPOUT + 4, 2 * P_DROPOUT + 1048580]
DROPOUT_EDGE_PS = [0.0, 0.1, 0.5, 0.999]
# grad_sumsq_kernel keeps two loads in flight: three trips = pair + single (lane 0 alone, then with the n % 4 tail), four trips = pair + pair
# (lane 0 alone; 257 lanes and a tail of 1)
NORM_NS = [2 * P_NORM + 4, 2 * P_NORM + 7, 3 * P_NORM + 4, 3 * P_NORM + 1029]
NORM_SPAN_LENGTHS = [2 * P_NORM + 7, 0, 1027, 5]     # three trips with a tail, an empty span among live ones, one short of 257 vectors, vector + 1

NARROW_N = 1031                                      # 257 vectors + a scalar tail of 3


def trips(n: int, per_pass: int) -> int:
    """grid-stride trips of the busiest lane (lane 0) over n elements"""
    return -(-n // per_pass) if n else 0


def span_layout(lengths: Sequence[int], gap: int = 12) -> Tuple[List[Tuple[int, int]], int]:
    """spans of the given lengths in one flat buffer, every begin on a multiple of 4 elements, at least `gap` elements between them -> (spans, total)"""
    spans, at = [], 4
    for n in lengths:
        spans.append((at, at + n))
        at = (at + n + gap + 3) // 4 * 4
    return spans, at


# ---------------------------------------------------------------------------------------------------------------- inputs
def rnd(n: int, seed: int, scale: float = 1.0) -> torch.Tensor:
    """the _rnd of tests/test_gpu_kernels.py"""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def narrowing_values(n: int = NARROW_N) -> np.ndarray:
    """float32 values whose bf16 rounding is decided by the rule, cycled over n elements so that both the vector body and the scalar tail hold each:
    ties to even (up and down), just past / short of a tie, the largest finite float (-> inf), subnormals, -0.0"""
    bits = np.array([0x3F808000,      # 1 + 2^-8: a tie, the even neighbour is below  -> 0x3F80
                     0x3F818000,      # a tie, the even neighbour is above            -> 0x3F82
                     0x3F808001,      # just past the tie                             -> 0x3F81
                     0x3F817FFF,      # just short of it                              -> 0x3F81
                     0xBF808000, 0xBF818000,
                     0x7F7FFFFF,      # FLT_MAX -> +inf
                     0xFF7FFFFF,      # -> -inf
                     0x7F7F7FFF,      # stays finite: the largest bf16
                     0x00000001,      # the smallest subnormal -> 0
                     0x00008000,      # a subnormal tie -> 0 (even)
                     0x00018000,      # a subnormal tie -> 0x0002
                     0x007FFFFF,      # the largest subnormal -> the smallest normal
                     0x80000001, 0x80018000,
                     0x80000000,      # -0.0
                     0x00000000,
                     0x3EAAAAAB,      # 1/3
                     0x4048F5C3], dtype=np.uint32)
    return np.resize(bits, n).view(np.float32).copy()


# ---------------------------------------------------------------------------------------------------------------- clipping
def clip_coef(total_norm, max_norm) -> np.float32:
    """optim.hip clip_coef: max_norm / (norm + 1e-6) clamped to at most 1; a NaN norm gives NaN (c > 1 is false for it)"""
    with np.errstate(all='ignore'):
        c = f32(max_norm) / (f32(total_norm) + f32(1e-6))
    return f32(1.0) if c > f32(1.0) else c


def _clip(gr: np.ndarray, clip) -> np.ndarray:
    """optim.hip clip_grad.  clip: None | ('norm', coef) | ('value', c)"""
    if clip is None:
        return gr
    mode, c = clip
    c = f32(c)
    if mode == 'norm':
        return gr * c
    assert mode == 'value'
    return np.where(gr > c, c, np.where(gr < -c, -c, gr)).astype(np.float32)      # a NaN fails both comparisons and stays


def _np32(t) -> np.ndarray:
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    assert t.dtype == np.float32
    return t


# ---------------------------------------------------------------------------------------------------------------- Adam / SGD in float32
def adam_bias(b1, b2, step: int) -> Tuple[np.float32, np.float32]:
    """(bc1, bc2_sqrt) as mts_adam_step forms them: in double from the float32 betas, then narrowed"""
    bc1 = 1.0 - float(f32(b1)) ** step
    bc2 = 1.0 - float(f32(b2)) ** step
    return f32(bc1), f32(np.sqrt(bc2))


def adam_f32(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, clip=None):
    """one step of optim.hip adam_loop, operation by operation in float32 -> (p, m, v), new arrays"""
    p, g, m, v = _np32(p), _np32(g), _np32(m), _np32(v)
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(grad_scale)
    bc1, bc2_sqrt = adam_bias(b1, b2, step)
    one = f32(1.0)
    with np.errstate(all='ignore'):
        step_size = lr / bc1
        gr = _clip(g * gs, clip)
        m = m + (one - b1) * (gr - m)
        v = b2 * v + ((one - b2) * gr) * gr
        denom = np.sqrt(v) / bc2_sqrt + eps
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def sgd_f32(p, g, buf, lr, mom, wd, first, grad_scale=1.0, clip=None):
    """one step of optim.hip sgd_loop in float32 -> (p, buf), new arrays"""
    p, g, buf = _np32(p), _np32(g), _np32(buf)
    lr, mom, wd, gs = f32(lr), f32(mom), f32(wd), f32(grad_scale)
    with np.errstate(all='ignore'):
        gr = _clip(g * gs, clip) + wd * p                # the weight decay is added to the CLIPPED gradient
        b = gr if first else mom * buf + gr
        p = p - lr * b
    assert p.dtype == b.dtype == np.float32
    return p, b


def to_bf16(x) -> torch.Tensor:
    """the one narrowing: torch's round-to-nearest-even conversion"""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- Adam / SGD in fp64
def _clip_torch(prm, clip):
    if clip is None:
        return
    mode, c = clip
    if mode == 'norm':
        torch.nn.utils.clip_grad_norm_([prm], c)
    else:
        torch.nn.utils.clip_grad_value_([prm], c)


def adam_f64(p0, grads, lr, clip=None) -> torch.Tensor:
    """torch.optim.Adam(eps=1e-7) on float64 copies, one step per gradient.  clip: None | ('norm', max_norm) | ('value', c)"""
    prm = torch.nn.Parameter(p0.detach().double().clone())
    opt = torch.optim.Adam([prm], lr=lr, eps=1e-7)
    for g in grads:
        prm.grad = g.detach().double().clone()
        _clip_torch(prm, clip)
        opt.step()
    return prm.detach()


def sgd_f64(p0, grads, lr, momentum, weight_decay, clip=None) -> torch.Tensor:
    prm = torch.nn.Parameter(p0.detach().double().clone())
    opt = torch.optim.SGD([prm], lr=lr, momentum=momentum, weight_decay=weight_decay)
    for g in grads:
        prm.grad = g.detach().double().clone()
        _clip_torch(prm, clip)
        opt.step()
    return prm.detach()


def within_bar(got, ref, rtol=1e-6, atol=1e-7) -> float:
    """max of |got - ref| / (atol + rtol |ref|): the bar of test_adam_and_sgd_match_torch holds where this is <= 1"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


# ---------------------------------------------------------------------------------------------------------------- dropout
_C0, _C1, _C2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


@functools.lru_cache(maxsize=6)
def hash32(n: int, seed: int, first: int = 0) -> np.ndarray:
    """common.h mts_hash32(seed, i) for i = first .. first + n - 1 (the splitmix64 finaliser, arithmetic modulo 2^64); read-only"""
    out = np.empty(n, dtype=np.uint32)
    seed64 = np.uint64(seed % (1 << 64))
    with np.errstate(over='ignore'):
        for a in range(0, n, 1 << 20):
            b = min(n, a + (1 << 20))
            idx = np.arange(a, b, dtype=np.uint64) + np.uint64((first + 1) % (1 << 64))
            z = seed64 + _C0 * idx
            z = (z ^ (z >> np.uint64(30))) * _C1
            z = (z ^ (z >> np.uint64(27))) * _C2
            z = z ^ (z >> np.uint64(31))
            out[a:b] = (z >> np.uint64(32)).astype(np.uint32)
    out.setflags(write=False)
    return out


def threshold(p) -> int:
    """mts_dropout_fwd: (uint32_t)min(4294967295.0, (double)p * 4294967296.0) with p the float32 the C ABI receives"""
    return int(min(4294967295.0, float(f32(p)) * 4294967296.0))


def keep(n: int, p, seed: int, first: int = 0) -> np.ndarray:
    """bool [n]: element first + i is kept"""
    return hash32(n, seed, first) >= np.uint32(threshold(p))


def dropout_scale(p) -> np.float32:
    return f32(1.0) / (f32(1.0) - f32(p))


def _widen(x: torch.Tensor) -> np.ndarray:
    assert x.dtype in (torch.float32, torch.bfloat16)
    return x.detach().cpu().float().numpy()


def _narrow(y: np.ndarray, dtype) -> torch.Tensor:
    t = torch.from_numpy(y)
    return t if dtype == torch.float32 else t.to(torch.bfloat16)


def dropout_fwd_f32(x: torch.Tensor, kept: np.ndarray, p, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = (keep ? x * scale : 0) + r in float32, in x's dtype"""
    xv = _widen(x)
    r = _widen(residual) if residual is not None else np.zeros_like(xv)
    y = np.where(kept, xv * dropout_scale(p), f32(0.0)).astype(np.float32) + r
    return _narrow(y, x.dtype)


def dropout_bwd_f32(dy: torch.Tensor, kept: np.ndarray, p) -> torch.Tensor:
    """dx = keep ? dy * scale : 0"""
    d = _widen(dy)
    return _narrow(np.where(kept, d * dropout_scale(p), f32(0.0)).astype(np.float32), dy.dtype)


def bits(t: torch.Tensor) -> torch.Tensor:
    """the bit pattern of every element as an integer tensor"""
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])
