"""PCA projection of the resident corpus (reference: ``--pca_reduce`` / ``--pca_value 167``, EncoderDataset.py:49-70: sklearn's
``PCA(n_components)`` fitted on the training split's sentence embeddings and applied to the validation and test splits).

The O(N D^2) and O(N D k) parts run on the device, on the corpus as it lies in HBM (csrc/pca.hip): ``ops.pca_colsum`` and
``ops.pca_gram`` give the fit's moments in fp64, ``ops.pca_project`` is the transform.  The one host step is ``pca_from_moments``: the
order-D symmetric eigenproblem in NumPy fp64, once per fit, from the 8 D^2 bytes read back.

  * ``ResidentCorpus.fit_pca(n_components)`` -> ``PcaReducer`` (resident.py);
  * ``PcaReducer.transform(x)``: device tensor [..., D] -> [..., k], same dtype;
  * ``ResidentCorpus.projected(reducer)`` -> a ResidentCorpus of width k that shares everything but the matrix;
  * ``project_folds(folds, n_components)``: per fold, fit on train and apply to train, val and test -- the reference's rule, and the rule
    that keeps the test split out of the fit.

The kernels are reproducible, so every rank that holds the corpus gets the same reducer bit for bit without a collective.
Deviations from upstream are listed in DESIGN.md ("PCA projection of the resident corpus")."""
import numpy as np
import torch

_STATE_ARRAYS = ('mean_', 'components_', 'explained_variance_', 'explained_variance_ratio_', 'singular_values_')
_STATE_INTS = ('n_components_', 'n_samples_', 'n_features_in_')


class PcaReducer:
    """A fitted PCA: sklearn's attribute names, fp64 NumPy.  ``mean_`` [D], ``components_`` [k, D] (rows of unit length, each with its
    coefficient of largest magnitude positive), ``explained_variance_`` [k] (descending), ``explained_variance_ratio_``,
    ``singular_values_``, ``n_components_``, ``n_samples_``, ``n_features_in_``."""

    def __init__(self, mean, components, explained_variance, explained_variance_ratio, singular_values, n_samples):
        self.mean_ = np.ascontiguousarray(mean, dtype=np.float64)
        self.components_ = np.ascontiguousarray(components, dtype=np.float64)
        self.explained_variance_ = np.ascontiguousarray(explained_variance, dtype=np.float64)
        self.explained_variance_ratio_ = np.ascontiguousarray(explained_variance_ratio, dtype=np.float64)
        self.singular_values_ = np.ascontiguousarray(singular_values, dtype=np.float64)
        if self.components_.ndim != 2 or self.mean_.shape != (self.components_.shape[1],):
            raise ValueError('PcaReducer: components_ is [k, D] and mean_ [D]')
        self.n_components_, self.n_features_in_ = int(self.components_.shape[0]), int(self.components_.shape[1])
        self.n_samples_ = int(n_samples)
        self._device_cache = {}

    def _on_device(self, device):
        """(center, w) = fp32(mean_), fp32(components_) on ``device``, uploaded once"""
        got = self._device_cache.get(device)
        if got is None:
            got = (torch.from_numpy(self.mean_.astype(np.float32)).to(device),
                   torch.from_numpy(self.components_.astype(np.float32)).contiguous().to(device))
            self._device_cache[device] = got
        return got

    def transform(self, x):
        """x: contiguous fp32 / bf16 device tensor [..., D] -> [..., k] of the same dtype: (x - fp32(mean_)) fp32(components_)^T by
        ``ops.pca_project`` on the current stream.  RuntimeError for a host tensor (there is no CPU fallback); ValueError for another
        dtype, width or a non-contiguous tensor."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError('PcaReducer.transform projects on the GPU (there is no CPU fallback): a device tensor is expected')
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'PcaReducer.transform: fp32 or bf16 is expected, not {x.dtype}')
        if x.dim() < 1 or int(x.shape[-1]) != self.n_features_in_:
            raise ValueError(f'PcaReducer.transform: the last dimension is {tuple(x.shape)[-1:]}, the reducer was fitted on width {self.n_features_in_}')
        if not x.is_contiguous():
            raise ValueError('PcaReducer.transform: a contiguous tensor is expected')
        from . import ops
        shape = tuple(x.shape[:-1]) + (self.n_components_,)
        y = torch.empty(shape, dtype=x.dtype, device=x.device)
        if y.numel():
            with torch.cuda.device(x.device):
                center, w = self._on_device(x.device)
                ops.pca_project(x.view(-1, self.n_features_in_), center, w, y.view(-1, self.n_components_))
        return y

    def state_dict(self):
        """-> a dict of NumPy arrays and ints (copies): what ``from_state_dict`` needs.  A model trained on projected inputs is useless
        without its reducer: save it next to the checkpoint."""
        out = {k: getattr(self, k).copy() for k in _STATE_ARRAYS}
        out.update({k: int(getattr(self, k)) for k in _STATE_INTS})
        return out

    @classmethod
    def from_state_dict(cls, d):
        r = cls(d['mean_'], d['components_'], d['explained_variance_'], d['explained_variance_ratio_'], d['singular_values_'], d['n_samples_'])
        if (r.n_components_, r.n_features_in_) != (int(d['n_components_']), int(d['n_features_in_'])):
            raise ValueError('PcaReducer.from_state_dict: n_components_ / n_features_in_ do not match components_')
        return r


def check_n_components(n_components, n, D, who):
    """sklearn's rule for an integer n_components with the full solver: 1 .. min(n, D); a float fraction and 'mle' are refused"""
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)):
        raise ValueError(f'{who}: n_components is an integer number of components (a float fraction and \'mle\' are not offered), not {n_components!r}')
    if n < 2:
        raise ValueError(f'{who}: a PCA needs at least 2 rows, the corpus has {n}')
    if not 1 <= int(n_components) <= min(n, D):
        raise ValueError(f'{who}: n_components = {int(n_components)} is outside 1 .. min(rows, width) = {min(n, D)}')
    return int(n_components)


def pca_from_moments(n, colsum, center, gram, n_components):
    """The host step of the fit, NumPy fp64.  n rows; colsum [D] their column sums; gram [D, D] = sum_r (x_r - center)(x_r - center)^T about
    any centre [D].  mu = colsum / n, delta = mu - center, S = gram - n delta delta^T is the scatter about the mean whatever the centre
    was (the centre is a numerical choice: near the mean, nothing cancels); eigh(S / (n - 1)), the n_components largest eigenpairs in
    descending order, every component with its coefficient of largest magnitude (lowest index on ties) positive -- sklearn >= 1.5's
    svd_flip(u_based_decision=False).  -> PcaReducer"""
    colsum = np.asarray(colsum, dtype=np.float64).reshape(-1)
    D = int(colsum.size)
    center = np.asarray(center, dtype=np.float64).reshape(-1)
    gram = np.asarray(gram, dtype=np.float64)
    if center.size != D or gram.shape != (D, D):
        raise ValueError(f'pca_from_moments: colsum has {D} columns, center {center.size}, gram is {gram.shape}')
    n = int(n)
    k = check_n_components(n_components, n, D, 'pca_from_moments')
    mu = colsum / n
    delta = mu - center
    S = gram - n * np.outer(delta, delta)
    lam, vec = np.linalg.eigh(S / (n - 1))
    lam, vec = lam[::-1][:k], vec[:, ::-1][:, :k].T
    top = np.argmax(np.abs(vec), axis=1)
    sign = np.sign(vec[np.arange(k), top])
    sign[sign == 0] = 1.0
    vec = vec * sign[:, None]
    total = float(np.trace(S)) / (n - 1)
    return PcaReducer(mu, vec, lam, lam / total if total > 0 else np.zeros_like(lam), np.sqrt(np.maximum(lam, 0.0) * (n - 1)), n)


def project_folds(folds, n_components=167):
    """folds: a list of (train, val, test) ``ResidentCorpus`` triples, ``val`` may be None.  Per fold the reducer is fitted on ``train``
    ALONE and applied to all three.  -> (the projected triples, ready for ``cross_validate``; the folds' reducers)"""
    out, reducers = [], []
    for train, val, test in folds:
        r = train.fit_pca(n_components)
        out.append((train.projected(r), None if val is None else val.projected(r), test.projected(r)))
        reducers.append(r)
    return out, reducers
