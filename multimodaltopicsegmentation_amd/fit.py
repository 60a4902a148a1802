"""The fit loop around sampler and step: epochs, validation on the device, the learning-rate schedule, early stopping and the best state
(reference: what ``pytorch_lightning.Trainer.fit`` does around ``TextSegmenter`` in train_fit.py:205-335 -- ModelCheckpoint(monitor, mode),
EarlyStopping(min_delta=0), and ``configure_optimizers``' ReduceLROnPlateau, lightning_model.py:759-781).

    fit(trainer, train, val, batch_size=8, max_epochs=100, search_threshold=True, metric='Pk')

``trainer`` is a ``NativeTrainer``; ``train`` / ``val`` are ``ResidentCorpus`` objects.  An epoch is ``DocumentShardSampler`` over ``train``
(rank and world from the trainer's process group) and ``trainer.step(train.batch(*item))`` per item -- the hand-written loop, launch for
launch: the step losses stay device scalars and are read once, when the epoch is over.  Validation runs in eval mode on documents
``rank::world`` of ``val`` in index order, no document dropped; a rank without documents skips the forward and still joins the
collectives.  What is monitored:

  * ``search_threshold=False``: ``val_loss = sum_b loss_b * docs_b / sum_b docs_b`` over the no-gradient ``loss`` of every batch, both sums
    all-reduced in float64; mode 'min';
  * ``search_threshold=True``: the scores go to a ``ThresholdSweep(metric=...)`` keyed by corpus index, ``gather()`` merges the ranks and
    ``best(metric)`` picks the threshold, which becomes ``trainer.model.th``; its 'valid_loss' is monitored, mode 'min' for Pk / WD and 'max'
    otherwise (train_fit.py:209-213);
  * no ``val``: the epoch's mean training loss (monitor='training_loss', train_fit.py:215), mode 'min'.

The schedule IS torch's ``ReduceLROnPlateau`` (on a one-parameter dummy optimizer; its lr is copied into ``trainer.lr`` after every
epoch), not a restatement of it.  Early stopping follows Lightning's ``EarlyStopping`` with ``min_delta = 0``: an epoch that is not strictly
better than the best so far counts, a better one resets the count, and training stops once ``patience`` consecutive epochs counted -- so
``patience=0`` and ``patience=1`` both stop at the first epoch without improvement, as in Lightning.  On improvement the loop keeps a device
clone of ``model.flat`` with the epoch's threshold; ``restore_best`` copies it back at the end.  Nothing is written to disk.
"""
import torch
import torch.distributed as dist

from .rnn_taggers import SheikhBiLSTM
from .taggers import decodes_by_viterbi
from .threshold_search import ThresholdSweep


class PlateauLR:
    """``configure_optimizers``' scheduler, driven without an optimizer of its own: torch's ReduceLROnPlateau on a dummy parameter."""

    def __init__(self, lr, mode, factor=0.8, patience=10):
        self._opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=float(lr))
        self._sched = torch.optim.lr_scheduler.ReduceLROnPlateau(self._opt, mode, factor=factor, patience=patience)

    def step(self, monitored):
        """-> the learning rate of the NEXT epoch"""
        self._sched.step(monitored)
        return float(self._opt.param_groups[0]['lr'])


class BestTracker:
    """Strict improvement (min_delta = 0) of the monitored value and Lightning's early-stopping count."""

    def __init__(self, mode, patience=None):
        if mode not in ('min', 'max'):
            raise ValueError("mode must be 'min' or 'max'")
        self.mode, self.patience = mode, patience
        self.best, self.best_epoch, self.wait = None, None, 0

    def step(self, epoch, monitored):
        """-> (improved, stop)"""
        improved = self.best is None or (monitored < self.best if self.mode == 'min' else monitored > self.best)
        if improved:
            self.best, self.best_epoch, self.wait = monitored, epoch, 0
            return True, False
        self.wait += 1
        return False, self.patience is not None and self.wait >= self.patience


def monitor_mode(search_threshold, metric):
    """lightning_model.py:774 / train_fit.py:209-213"""
    return 'min' if (not search_threshold or str(metric).lower() in ('pk', 'wd')) else 'max'


def _refusal(model, metric):
    """Why a threshold cannot be searched for this model and metric (TextSegmenter._sweep_refusal's reasons), or None."""
    if decodes_by_viterbi(model):
        return f"search_threshold: architecture '{model.crf_architecture}' decodes by Viterbi and has no decision threshold to search"
    if str(metric).lower() == 'b':
        return (f"search_threshold: metric '{metric}' (B-measure) needs the third-party package segeval and is not in the threshold-sweep "
                "kernels; use 'Pk', 'WD', 'F1' or 'scaiano'")
    return None


def _forward(model, batch):
    """scores of a batch, dispatched as TextSegmenter.validation_step does"""
    if getattr(model, 'takes_domains', False):
        return model(batch['src_tokens'], batch['src_lengths'], batch['domain'])[0]
    if batch.get('src_tokens2') is not None and hasattr(model, '_rnn2'):
        return model(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'])[0]
    return model(batch['src_tokens'], batch['src_lengths'])[0]


def _loss(model, batch):
    if getattr(model, 'takes_domains', False):
        return model.loss(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'], batch['domain'])
    if batch.get('src_tokens2') is not None and hasattr(model, '_rnn2'):
        return model.loss(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'], batch['tgt_tokens'])
    return model.loss(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'])


def _sum_over_ranks(values, trainer):
    """float64 sums over the trainer's ranks -> list of floats (one read)"""
    dev = trainer.model.flat.device
    t = values.to(torch.float64) if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=torch.float64, device=dev)
    if trainer.world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=trainer.pg)
    return t.tolist()


def fit(trainer, train, val=None, *, batch_size, max_epochs, search_threshold=False, metric='Pk', thresholds=None, end_boundary=False,
        patience=None, lr_factor=0.8, lr_patience=10, seed=0, shuffle=True, restore_best=True, on_epoch_end=None, augment=None, mask_inner=None):
    """-> {'epochs': [{'epoch', 'train_loss', 'monitored', 'lr' (the epoch's), 'threshold', + 'val_loss' or best(metric)'s row}, ...],
    'best_epoch', 'best_value', 'threshold' (the best epoch's), 'stopped_early'}; the same values on every rank.  ``on_epoch_end(record)``
    is called on every rank, after the epoch's threshold and learning rate are set and before the best state is restored.  ``augment``:
    None, or 'reverse' / 'shuffle' to train on ``train.augmented(augment, seed=seed)`` (resident.AugmentedCorpus: every document and a twin
    with its topic segments reordered, 'shuffle' anew every epoch); validation never augments.  ``mask_inner``: None, or the probability
    that a negative sentence is KEPT, to train on ``train.masked(mask_inner, seed=seed)`` (resident.MaskedCorpus: negative-sentence masking,
    drawn anew every epoch); validation never masks.  The two views do not compose: both at once is a ValueError."""
    if augment is not None and mask_inner is not None:
        raise ValueError('fit: augment= and mask_inner= cannot be combined (the two corpus views do not compose)')
    for name, c in (('training', train), ('validation', val)):
        if c is not None and not getattr(c, 'labelled', True):
            raise ValueError(f'fit: the {name} corpus is unlabelled (ResidentCorpus.from_documents); predict is the pass that needs no labels')
    model = trainer.model
    world = trainer.world
    rank = dist.get_rank(trainer.pg) if world > 1 else 0
    if search_threshold:
        if val is None:
            raise ValueError('fit: search_threshold=True needs a validation corpus')
        why = _refusal(model, metric)
        if why is not None:
            raise NotImplementedError(why)
    mode = monitor_mode(search_threshold and val is not None, metric)
    if augment is not None:
        train = train.augmented(augment, seed=seed)
    if mask_inner is not None:
        train = train.masked(mask_inner, seed=seed)
    sampler = train.sampler(batch_size, rank=rank, world=world, shuffle=shuffle, seed=seed)
    if len(sampler) == 0:
        raise ValueError('fit: the training corpus gives no batch (fewer documents in every global batch than ranks)')
    sweep = ThresholdSweep(thresholds=thresholds, end_boundary=end_boundary, invert=isinstance(model, SheikhBiLSTM),
                           metric=metric) if search_threshold else None
    val_docs = list(range(rank, len(val), world)) if val is not None else []
    dev = model.flat.device

    def validate():
        """-> (monitored value, record fields, threshold or None)"""
        was_training = model.training
        model.eval()
        try:
            if sweep is not None:
                sweep.reset()
                if not hasattr(model, 'th'):
                    model.th = None                    # SheikhBiLSTM's forward reads it (upstream never sets it before test_step does)
                for s in range(0, len(val_docs), batch_size):
                    idx = val_docs[s:s + batch_size]
                    batch = val.batch(idx)
                    sweep.add(_forward(model, batch), batch['tgt_tokens'], batch['src_lengths'], keys=idx)
                row = sweep.gather(trainer.pg).best(metric)
                sweep.reset()
                return row['valid_loss'], row, row['threshold']
            losses, docs = [], []
            with torch.no_grad():
                for s in range(0, len(val_docs), batch_size):
                    idx = val_docs[s:s + batch_size]
                    losses.append(_loss(model, val.batch(idx)).detach().to(torch.float64))
                    docs.append(float(len(idx)))
            sums = torch.zeros(2, dtype=torch.float64, device=dev)
            if losses:
                w = torch.tensor(docs, dtype=torch.float64, device=dev)
                sums[0], sums[1] = (torch.stack(losses) * w).sum(), w.sum()
            total, n = _sum_over_ranks(sums, trainer)
            return total / n, {'val_loss': total / n}, None
        finally:
            model.train(was_training)

    lr_rule = PlateauLR(trainer.lr, mode, lr_factor, lr_patience)
    tracker = BestTracker(mode, patience)
    best_flat, best_threshold, stopped, epochs = None, None, False, []
    for epoch in range(int(max_epochs)):
        sampler.set_epoch(epoch)
        lr_now = trainer.lr
        step_losses = [trainer.step(train.batch(*item)) for item in sampler]
        stacked = torch.stack([v.detach() for v in step_losses]).to(torch.float64)
        total, n = _sum_over_ranks(torch.stack([stacked.sum(), torch.tensor(float(len(step_losses)), dtype=torch.float64, device=stacked.device)]),
                                   trainer)
        record = {'epoch': epoch, 'train_loss': total / n, 'lr': lr_now, 'threshold': None}
        if val is not None:
            monitored, fields, threshold = validate()
            record.update(fields)
            record['threshold'] = threshold
            if threshold is not None:
                model.th = threshold
        else:
            monitored = record['train_loss']
        record['monitored'] = monitored
        trainer.lr = lr_rule.step(monitored)
        improved, stop = tracker.step(epoch, monitored)
        if improved:
            best_flat, best_threshold = model.flat.detach().clone(), record['threshold']
        epochs.append(record)
        if on_epoch_end is not None:
            on_epoch_end(record)
        if stop:
            stopped = True
            break
    if restore_best and best_flat is not None:
        with torch.no_grad():
            model.flat.copy_(best_flat)
        if hasattr(model, '_wcopy_version'):
            model._wcopy_version = None                # the bf16 mirror is re-cast from the restored master at its next use
        if best_threshold is not None:
            model.th = best_threshold
    return {'epochs': epochs, 'best_epoch': tracker.best_epoch, 'best_value': tracker.best, 'threshold': best_threshold,
            'stopped_early': stopped}
