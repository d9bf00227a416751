"""Drop-in for the reference's training entry point `Train_SMT.train` (Train_SMT.py:143-356): the epoch loop over a device-resident
pair dataset (deepmerge_amd/dataset.py), with the reference's schedule, checkpoint cadence, file names and checkpoint dict.

Per epoch: the lr of MultiStepLR(milestones, gamma) stepped once per epoch; ONE dm_pair_epoch_draw launch for the epoch's shuffled
pair draw (MyUtils1.py:275-293 + DataLoader(shuffle=True), keyed by (dataset seed, epoch)); per full batch a
feed.PairFeed gather straight into the captured step's inputs and a PairTrainer hipGraph replay; the partial last batch
(drop_last=False) through a second feed sized to it and an eager step.  Step losses are summed on the device and read once per epoch.

Resume (`is_retrained`): weights, Adam moments and the saved lr come back from the checkpoint; `start_epoch = epoch + 1`, and the
milestones are counted again from the resumed epoch, as upstream (the scheduler is created afresh and its state is not saved).
Because the draw is keyed by (seed, epoch), a resumed run sees the same data as an uninterrupted one.

Validation (`val_dataset=`): after each epoch's steps and loss read, and before the checkpoint, one evaluate.PairEvaluator (built
once, with the training margin) runs over the held-out pairs -- loss and merge P/R/F at the margin, logged through
callbacks.LossHistory when `log_dir` is given.  It reads no RNG and touches no parameter, gradient, optimizer state or captured
graph input, so the training run is the same, bit for bit, with or without it.
"""
from __future__ import annotations

import os
import time
from collections import Counter
from typing import List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import ops
from .callbacks import LossHistory
from .checkpoint import load_checkpoint, save_checkpoint
from .dataset import MAX_HARDNESS, MAX_WEIGHT_TOTAL, PairDataset, balance_weights, hardness_weights
from .evaluate import PairEvaluator, format_result
from .ExtractFeatures import Euclidean_distance  # noqa: F401  (Train_SMT.Euclidean_distance, Train_SMT.py:115-131)
from .feed import PairFeed
from .trainer import PairTrainer, stacked_pair_inputs

NUM_EPOCHS = 100                 # config.py num_epochs
MODEL_PARAS_PATH = "./model/"    # config.py model_paras_path


def epoch_lr(lr0: float, k: int, milestones: Sequence[int] = (40, 80), gamma: float = 0.2) -> float:
    """The lr of torch.optim.lr_scheduler.MultiStepLR after k per-epoch steps from lr0 (Train_SMT.py:194, :351), in torch's own
    chained form: at each milestone the current lr is multiplied by gamma ** (times the milestone is listed).  (The closed form
    lr0 * gamma ** n can differ from it in the last bit.)"""
    lr, count = float(lr0), Counter(int(m) for m in milestones)
    for e in range(1, int(k) + 1):
        if e in count:
            lr = lr * gamma ** count[e]
    return lr


def checkpoint_due(epoch: int) -> bool:
    """Train_SMT.py:317: a checkpoint after every fifth epoch and after each of the last ten of a 100-epoch run."""
    return (epoch + 1) % 5 == 0 or epoch + 1 >= 90


def checkpoint_name(epoch: int, num_epochs: int, net_name: str, t: time.struct_time) -> str:
    """The reference's file names (Train_SMT.py:318-341)."""
    if epoch + 1 == 100:
        return "model-{0}-{1}-{2}_{3}-{4}-{5}_{6}epochs.pth".format(t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min, net_name, num_epochs)
    return "model-{0}-{1}-{2}_{3}-{4}_{5}epochs.pth".format(t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min, epoch + 1)


def train(net, margin, train_bs, lr_init, normMean, normStd, lamda, belta, is_retrained=False, checkpoint_path=None, *,
          dataset: PairDataset = None, num_epochs: int = NUM_EPOCHS, milestones: Sequence[int] = (40, 80), gamma: float = 0.2,
          model_paras_path: str = MODEL_PARAS_PATH, val_dataset: Optional[PairDataset] = None, val_batch: int = 1000,
          val_thresholds: Optional[Sequence[float]] = None, log_dir: Optional[str] = None,
          val_history: Optional[list] = None, augment: Optional[str] = None, radiometric=None, balance: Optional[float] = None,
          mining: Optional[ops.Mining] = None, draws: Optional[int] = None) -> Tuple[List[int], List[float]]:
    """`Train_SMT.train` with the reference's positional signature (normMean / normStd are unused, as upstream; lamda / belta go
    to Loss).  `dataset` replaces the reference's hard-coded shapefile folders; the draw's seed is the dataset's.  Returns
    (epoch indices, per-epoch mean loss = sum of step losses / number of steps), one entry per epoch run.

    val_dataset: a held-out PairDataset (not `dataset` itself: a dataset reuses one table buffer), evaluated after every epoch by
    evaluate.PairEvaluator(net, val_dataset, val_batch, margin, val_thresholds); `(epoch, PairEvalResult)` is appended to
    `val_history` when given.  log_dir: a callbacks.LossHistory there gets (mean train loss, val loss, F at the margin) per epoch --
    without val_dataset, what upstream writes: (mean loss, mean loss, elapsed seconds rounded to 2 places).

    augment: None, "flips" or "d4" -- handed to dataset.epoch: every pair of every epoch is fed at a dihedral orientation keyed by
    (dataset seed, epoch, pair), both of its crops alike, so a resumed run sees the same views.  The
    validation pass never augments.

    radiometric: None, an ops.Radiometric or a (contrast, brightness, colour) triple -- handed to dataset.epoch: every pair of every
    epoch is fed with a gain and an offset per band keyed by (dataset seed, epoch, pair), both of its crops and designed rows alike
    (DESIGN.md 3.8 / 3.9).  Independent of `augment`; resumes like it; never applied in validation.

    balance: None or the share p of positive pairs the model should see -- every epoch is `draws` pairs sampled with replacement
    under dataset.balance_weights(flag, p) (dataset.epoch(weights=)): a draw is positive with probability exactly
    round(65536 p) / 65536 whatever the list's ratio.  The weights are a function of the list alone, so a resumed run equals the
    uninterrupted one bit for bit, always.

    mining: None or an ops.Mining(every=k, cap=c[, floor_share=f]) -- at the start of the run's first epoch and of every epoch e with
    e % k == 0, dataset.pair_terms(net, val_batch, margin, key=e) evaluates the loss term of every training pair with the model as it
    stands, and dataset.hardness_weights(term, f, c) turns it into weights (times the balance weights when both are given) that the
    epochs up to the next refresh are sampled with.  The weights are not in the checkpoint (its format is the reference's): a resumed
    run recomputes them at its first epoch, from the restored model.  So it equals the uninterrupted run bit for bit iff the resume
    epoch is a refresh epoch of that run; checkpoints fall after epochs 5, 10, ..., so `every` in {1, 5} qualifies.  Other values
    train correctly but resume on fresher weights than the uninterrupted run had at that epoch.

    draws: the epoch length in pairs when balance or mining is given (default: len(dataset)); the steps, the captured graph and the
    partial last batch follow it.  All three None: nothing of the above runs."""
    if dataset is None:
        raise ValueError("train() needs dataset=PairDataset.from_arrays(...) (the reference's hard-coded folders are not portable)")
    if val_dataset is not None and val_dataset is dataset:
        raise ValueError("val_dataset must not be the training dataset: a PairDataset keeps one table buffer, and the held-out pairs "
                         "must be pairs the model does not train on")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("train() runs on one GPU; data-parallel sharding of the epoch is not implemented")
    if int(train_bs) < 1:
        raise ValueError(f"train_bs must be >= 1, got {train_bs}")
    if augment is not None and augment not in ops.ORIENT_MASKS:
        raise ValueError(f"augment must be None, 'flips' or 'd4', got {augment!r}")
    radiometric = ops.Radiometric.of(radiometric)
    if mining is not None and not isinstance(mining, ops.Mining):
        raise ValueError(f"mining must be None or an ops.Mining, got {mining!r}")
    sampled = balance is not None or mining is not None
    if draws is not None and not sampled:
        raise ValueError("draws needs balance= or mining=: an unweighted epoch is every pair exactly once")
    if draws is not None and not 1 <= int(draws) <= 2 ** 30:
        raise ValueError(f"draws must be in 1 .. 2^30, got {draws}")
    scales = [int(s) for s in getattr(net, "input_image_scales", ())]
    if not scales:
        raise ValueError(f"{type(net).__name__} has no input_image_scales: train() feeds patch pyramids")
    dev = dataset.device
    net.to(dev)
    rows = stacked_pair_inputs(net)            # v3 family: patch-embed rows; other models: fp32 patch tensors
    numerics = getattr(net, "numerics", ops.get_numerics())
    max_window = dataset.max_window(len(scales))
    trainer = PairTrainer(net, margin=margin, lr=lr_init, lamda=lamda, belta=belta)
    start_epoch, lr0 = 0, float(lr_init)
    if is_retrained:
        state = load_checkpoint(checkpoint_path, net, trainer)
        start_epoch = int(state["epoch"]) + 1
        if start_epoch >= num_epochs:
            raise ValueError("start_epoch must be smaller than number of epochs")
        lr0 = float(trainer.lr)                 # optimizer.load_state_dict brings the saved lr back (Train_SMT.py:196-197)

    B, N = int(train_bs), len(dataset)
    class_w = weights = None
    if sampled:
        N = len(dataset) if draws is None else int(draws)          # the epoch length
        class_w = weights = balance_weights(dataset.host.flag, balance).to(dev) if balance is not None else None
        if mining is not None and class_w is not None and int(class_w.sum()) * MAX_HARDNESS >= MAX_WEIGHT_TOTAL:
            raise ValueError("balance with mining: the total weight could reach 2^62")    # at h = 256: whatever the model says
    n_full, tail = N // B, N % B
    feed = tail_feed = None
    if n_full:
        trainer.enable_graph(warmup=1)
        feed = PairFeed(dataset.tiles, scales, B, max_window, rows=rows, numerics=numerics, trainer=trainer if rows else None)
    if tail:
        tail_feed = PairFeed(dataset.tiles, scales, tail, max_window, rows=rows, numerics=numerics)
    evaluator = PairEvaluator(net, val_dataset, batch=val_batch, margin=margin, thresholds=val_thresholds) \
        if val_dataset is not None else None
    history = LossHistory(log_dir) if log_dir is not None else None
    name = getattr(net, "name", type(net).__name__)
    print(len(dataset), dataset.positive_pair_number, dataset.negative_pair_number)
    iteration_history_train, loss_history_train = [], []
    previous_time = 0.0
    start_time = time.time()
    for epoch in range(start_epoch, num_epochs):
        lr = epoch_lr(lr0, epoch - start_epoch, milestones, gamma)
        trainer.lr = lr                         # what the optimizer holds this epoch (checkpoint.optimizer_state_dict writes it)
        if mining is not None and (epoch == start_epoch or epoch % mining.every == 0):
            term = dataset.pair_terms(net, val_batch, margin, key=epoch)
            weights = hardness_weights(term, mining.floor_share, mining.cap, class_weights=class_w)
        if sampled:
            table = dataset.epoch(epoch, B, augment=augment, radiometric=radiometric, weights=weights, draws=N)
        else:
            table = dataset.epoch(epoch, B, augment=augment, radiometric=radiometric)
        total = torch.zeros((), dtype=torch.float32, device=dev)
        for s in range(len(table)):
            if s < n_full:
                total += trainer.step(*feed.fill(table.step(s)), lr=lr)
            else:
                total += trainer.step(*tail_feed.fill(table.step(s)), lr=lr, eager=True)
        mean_loss = float(total) / len(table)
        for f in (feed, tail_feed):
            if f is not None:
                f.check()
        val = evaluator.run() if evaluator is not None else None
        end_time = time.time()
        iteration_history_train.append(epoch)
        loss_history_train.append(mean_loss)
        line = f"epoch {epoch + 1}/{num_epochs}: lr {lr:.3e} mean loss {mean_loss:.6f}"
        if val is not None:
            line += " " + format_result(val)
            if val_history is not None:
                val_history.append((epoch, val))
        print(f"{line} time {end_time - start_time:.2f} s", flush=True)
        if history is not None:
            if val is not None:
                history.append_loss(mean_loss, val.loss, val.f_score)
            else:                               # upstream's stand-ins (Train_SMT.py:350)
                history.append_loss(mean_loss, mean_loss, round(end_time - start_time, 2))
        if checkpoint_due(epoch):
            os.makedirs(model_paras_path, exist_ok=True)
            path = os.path.join(model_paras_path, checkpoint_name(epoch, num_epochs, name, time.localtime()))
            save_checkpoint(path, trainer, epoch, end_time - start_time + previous_time)
    print(f"training finished: {round(time.time() - start_time + previous_time, 2)} s")
    return iteration_history_train, loss_history_train
