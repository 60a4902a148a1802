"""fp64 restatement of BiLSTMLateFusion(merge='gate') (DESIGN.md "Gated late-fusion merge"; the reference has no gate, so the definition is
the project's own) on top of oracle.restatement's LSTM and loss elements and tests/cosine_oracle.py.  Gradients come from autograd.

    h1, h2 = the two encoders' outputs [B, Lm, 2H] (Lm = max(lengths); rows at or past a document's length are 0), dropout 0
    a = [h1 ; h2] W_g^T + b_g          W_g [2H, 4H], b_g [2H]
    z = sigmoid(a)
    m = h2 + z (h1 - h2)
    scores = m W_c^T + b_c             W_c [n_out, 2H]
    loss: oracle.restatement.tagger_loss; with segments: 0.1 * cosine loss over m + the unmasked main loss (tests/cosine_oracle.py)
"""
from typing import Dict

import torch
from torch import Tensor

from oracle import restatement as R
from tests import cosine_oracle as C
from tests.helpers import bilstm_param_shapes


def param_shapes(D, H, NL, n_out):
    s = bilstm_param_shapes(D[0], H, NL, n_out, prefix='model1.')
    s.update(bilstm_param_shapes(D[1], H, NL, n_out, prefix='model2.'))
    s['classification.weight'], s['classification.bias'] = (n_out, 2 * H), (n_out,)
    s['gate.weight'], s['gate.bias'] = (2 * H, 4 * H), (2 * H,)
    return s


def num_layers(p: Dict[str, Tensor]) -> int:
    return sum(1 for k in p if k.startswith('model1.rnn.weight_hh_l') and not k.endswith('_reverse'))


def gate(h1: Tensor, h2: Tensor, w_g: Tensor, b_g: Tensor):
    """-> (m, z, a)"""
    a = torch.cat((h1, h2), dim=-1) @ w_g.t() + b_g
    z = torch.sigmoid(a)
    return h2 + z * (h1 - h2), z, a


def gate_backward(h1: Tensor, h2: Tensor, w_g: Tensor, z: Tensor, dm: Tensor):
    """The backward as the definition writes it out (what the kernels and GEMMs compute) -> (dh1, dh2, da, dW_g, db_g); 2-d operands."""
    W = h1.shape[-1]
    da = dm * (h1 - h2) * z * (1 - z)
    dh1 = dm * z + da @ w_g[:, :W]
    dh2 = dm * (1 - z) + da @ w_g[:, W:]
    return dh1, dh2, da, da.t() @ torch.cat((h1, h2), dim=-1), da.sum(0)


def merged(x1: Tensor, x2: Tensor, lengths: Tensor, p: Dict[str, Tensor], batched: bool = True):
    """-> (m [B, Lm, 2H], z)"""
    NL = num_layers(p)
    h1 = R.rnn_forward(x1, lengths, p, 'model1.', NL, True, batched)
    h2 = R.rnn_forward(x2, lengths, p, 'model2.', NL, True, batched)
    m, z, _ = gate(h1, h2, p['gate.weight'], p['gate.bias'])
    return m, z


def scores(x1: Tensor, x2: Tensor, lengths: Tensor, p: Dict[str, Tensor], batched: bool = True, return_gate: bool = False):
    m, z = merged(x1, x2, lengths, p, batched)
    s = m @ p['classification.weight'].t() + p['classification.bias']
    return (s, z) if return_gate else s


def loss(x1, x2, lengths: Tensor, tags: Tensor, p: Dict[str, Tensor], loss_fn: str, segments=None, batched: bool = True):
    """-> (loss, scores [B, Lm, n_out], z)"""
    m, z = merged(x1, x2, lengths, p, batched)
    s = m @ p['classification.weight'].t() + p['classification.bias']
    if segments is None:
        return R.tagger_loss(s, lengths, tags, loss_fn), s, z
    cl, _, _ = C.cosine_loss(m, lengths.tolist(), segments)
    return C.WEIGHT * cl + C.main_loss(s, tags, loss_fn), s, z


def valid_gates(z: Tensor, lengths) -> Tensor:
    """the gates of the rows inside each document, flattened"""
    return torch.cat([z[b, :int(n)].reshape(-1) for b, n in enumerate(lengths)])


def decided_fraction(z: Tensor, lengths) -> float:
    """share of the gates over valid rows outside [0.25, 0.75]: the tests require >= 1 / 5, so that a merge that ignored the gate fails"""
    v = valid_gates(z.detach(), lengths)
    return float(((v < 0.25) | (v > 0.75)).double().mean())


# ---- the cases tests/test_gated_fusion_cpu.py and tests/test_gpu_gated_fusion.py share ------------------------------------------------
GATE_SCALE = 48.0          # seeded gate.weight times this: |a| is then O(1) and the gates spread over (0, 1): 0.39 (H = 32) and 0.47 (H = 25)
                           # of the valid gates outside [0.25, 0.75] (tests/test_gated_fusion_cpu.py asserts >= 0.2)


def seeded_case_params(D, H, NL, n_out, seed, gate_scale=GATE_SCALE, dtype=torch.float32):
    from tests.helpers import seeded_param
    p = {}
    for n, s in param_shapes(D, H, NL, n_out).items():
        w = seeded_param(n, s, seed)
        if n == 'gate.weight':
            w = w * gate_scale
        p[n] = torch.from_numpy(w).to(dtype)
    return p


def small_case(H=32, n_out=1, seed=11):
    """D1 = 40, D2 = 24, 2 layers, B = 4, input L = 33, lengths [30, 12, 1, 22] (max 30 < 33: the input is trimmed); fp32 tensors."""
    D, NL, B, L = (40, 24), 2, 4, 33
    g = torch.Generator().manual_seed(100 + seed)
    lengths = torch.tensor([30, 12, 1, 22])
    x1, x2 = torch.randn(B, L, D[0], generator=g), torch.randn(B, L, D[1], generator=g)
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths.tolist()):
        x1[b, n:], x2[b, n:] = 0.0, 0.0
        tags[b, :n] = (torch.rand(n, generator=g) < 0.3).float()
        tags[b, n - 1] = 0
    return dict(D=D, H=H, NL=NL, B=B, L=L, lengths=lengths, x1=x1, x2=x2, tags=tags, p=seeded_case_params(D, H, NL, n_out, seed),
                segments=[[4, 9, 30], [12], [], [1, 2, 11, 20]])


def mid_case(seed=7):
    """bf16 at the production width: D1 = 128, D2 = 96, H = 256, 2 layers, B = 8, L = 96, ragged; bf16-exact inputs."""
    import numpy as np
    B, L, D, H, NL = 8, 96, (128, 96), 256, 2
    rng = np.random.default_rng(seed)
    lengths = [96, 1, 2, 57, 96, 33, 80, 14]
    x1 = torch.from_numpy(rng.standard_normal((B, L, D[0])).astype(np.float32)).to(torch.bfloat16).float()
    x2 = torch.from_numpy(rng.standard_normal((B, L, D[1])).astype(np.float32)).to(torch.bfloat16).float()
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths):
        x1[b, n:], x2[b, n:] = 0.0, 0.0
        t = (rng.random(n) < 0.25).astype(np.float32)
        t[-1] = 0
        tags[b, :n] = torch.from_numpy(t)
    return dict(D=D, H=H, NL=NL, B=B, L=L, lengths=torch.tensor(lengths), x1=x1, x2=x2, tags=tags, p=seeded_case_params(D, H, NL, 1, seed))
