"""Held-out pair validation: the contrastive loss and the merge decision's precision / recall / F on pairs the model did not train
on -- the `val_loss` and `f_score` that the reference's `LossHistory.append_loss` (callbacks.py:41-57, called at Train_SMT.py:350)
was meant to log and never computed.

`PairEvaluator(net, dataset).run()` draws the dataset's pairs once with a fixed key (`dataset.epoch(draw_key, batch)`, DESIGN.md 3.9:
the same held-out samples every run), gathers each batch with a feed.PairFeed, runs ONE eval forward over the stacked
[left; right] batch, and per batch computes
  simi    ops.edge_similarity(F, (i, b + i)) -- the sweep's own distance kernel, so each pair's decision `simi < margin` is the
          one ExtractFeatures.rag_similarity_sweep would take for the same two embeddings;
  term    ops.contrastive_terms(F[:b], F[b:], flag, margin) -- the per-pair contrastive loss in the pinned order.
After the last batch ONE ops.pair_eval_summary launch counts merges per class at every threshold and sums the terms; its small
result block is the only host read (besides the feeds' error flags).  Metrics are computed on the host in float64 from the counts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .feed import PairFeed
from .trainer import stacked_pair_inputs

MAX_THRESHOLDS = ops.PAIR_EVAL_MAX_THRESHOLDS
MAX_FEATURE_DIM = 128          # dm_edge_similarity's pinned summation order (oracle/sweep_strict.c)


def default_thresholds(margin: float) -> np.ndarray:
    """64 thresholds margin/32, 2 margin/32, ..., 2 margin (the margin itself is one of them)."""
    return (float(margin) * np.arange(1, 65, dtype=np.float64) / 32.0).astype(np.float32)


def threshold_set(thresholds: Optional[Sequence[float]], margin: float) -> np.ndarray:
    """The float32 thresholds an evaluation counts at: `thresholds` (finite, strictly ascending as float32; default
    `default_thresholds(margin)`) with the margin merged in, sorted, duplicates dropped.  Raises ValueError on anything else, and
    when the set is empty or holds more than 1024 values."""
    m = np.float32(margin)
    if not np.isfinite(m):
        raise ValueError(f"margin must be finite, got {margin}")
    t = default_thresholds(margin) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if t.size == 0:
        raise ValueError("thresholds: at least one value is needed")
    if not np.all(np.isfinite(t)):
        raise ValueError("thresholds must be finite")
    with np.errstate(over="ignore"):
        t32 = t.astype(np.float32)
    if not np.all(np.isfinite(t32)):
        raise ValueError("thresholds must be finite in float32")
    if t32.size > 1 and not np.all(t32[1:] > t32[:-1]):
        raise ValueError("thresholds must be strictly ascending (as float32)")
    out = np.union1d(t32, np.asarray([m], dtype=np.float32)).astype(np.float32)
    if out.size > MAX_THRESHOLDS:
        raise ValueError(f"{out.size} thresholds with the margin merged in; at most {MAX_THRESHOLDS}")
    return out


def _ratio(num: float, den: float) -> float:
    return num / den if den else 0.0


def prf(tp: int, fp: int, fn: int) -> Tuple[float, float, float]:
    """(precision, recall, F) of the merge class, float64; each is 0 when its denominator is 0."""
    p, r = _ratio(float(tp), float(tp + fp)), _ratio(float(tp), float(tp + fn))
    return p, r, _ratio(2.0 * p * r, p + r)


@dataclass(frozen=True)
class PairEvalResult:
    """One evaluation.  Positive class: merge (flag 1, same object); a pair is merged at threshold t when simi < t."""
    n_pairs: int
    n_pos: int
    n_neg: int
    loss: float                          # mean contrastive term = loss_sum / n_pairs
    margin: float
    thresholds: Tuple[float, ...]        # float32 values, ascending, the margin among them
    merged_pos: Tuple[int, ...]          # per threshold: positive pairs merged (true positives)
    merged_neg: Tuple[int, ...]          # per threshold: negative pairs merged (false positives)
    tp: int                              # at the margin
    fp: int
    fn: int
    tn: int
    precision: float
    recall: float
    f_score: float
    accuracy: float
    best_threshold: float                # the smallest threshold that reaches the maximum F
    best_f_score: float

    @classmethod
    def from_counts(cls, n_pairs: int, n_pos: int, loss_sum: float, margin: float, thresholds: Sequence[float],
                    merged_pos: Sequence[int], merged_neg: Sequence[int]) -> "PairEvalResult":
        th = tuple(float(np.float32(x)) for x in thresholds)
        mp, mn = tuple(int(x) for x in merged_pos), tuple(int(x) for x in merged_neg)
        if not (len(th) == len(mp) == len(mn)) or not th:
            raise ValueError("one count per threshold, and at least one threshold")
        n_pairs, n_pos = int(n_pairs), int(n_pos)
        n_neg = n_pairs - n_pos
        m32 = float(np.float32(margin))
        if m32 not in th:
            raise ValueError(f"the margin {margin} is not among the thresholds")
        j = th.index(m32)
        tp, fp = mp[j], mn[j]
        fn, tn = n_pos - tp, n_neg - fp
        p, r, f = prf(tp, fp, fn)
        fs = [prf(a, b, n_pos - a)[2] for a, b in zip(mp, mn)]
        best = max(range(len(th)), key=lambda k: (fs[k], -k))
        return cls(n_pairs=n_pairs, n_pos=n_pos, n_neg=n_neg, loss=float(loss_sum) / n_pairs, margin=float(margin), thresholds=th,
                   merged_pos=mp, merged_neg=mn, tp=tp, fp=fp, fn=fn, tn=tn, precision=p, recall=r, f_score=f,
                   accuracy=_ratio(float(tp + tn), float(n_pairs)), best_threshold=th[best], best_f_score=fs[best])


class PairEvaluator:
    """Evaluate `net` on every pair of `dataset` (a deepmerge_amd.dataset.PairDataset the model does not train on).

    batch: pairs per eval forward (2 batch samples per forward); margin: the merge threshold and the loss margin; thresholds: the
    extra thresholds to count at (see `threshold_set`); draw_key: the epoch key of the fixed draw.  Feeds and buffers are built
    once; `run()` may be called after every training epoch.  `simi` / `term` are views of the device buffers of the last run."""

    def __init__(self, net, dataset, batch: int = 1000, margin: float = 1.0, thresholds: Optional[Sequence[float]] = None,
                 draw_key: int = 0):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("PairEvaluator runs on one GPU, as train() does")
        if int(batch) < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        self.thresholds = threshold_set(thresholds, margin)
        scales = [int(s) for s in getattr(net, "input_image_scales", ())]
        if not scales:
            raise ValueError(f"{type(net).__name__} has no input_image_scales: the evaluator feeds patch pyramids")
        self.net, self.dataset, self.margin, self.draw_key = net, dataset, float(margin), int(draw_key)
        self.batch = int(batch)
        dev = dataset.device
        N = len(dataset)
        self.n_pairs = N
        self.n_full, tail = N // self.batch, N % self.batch
        rows = stacked_pair_inputs(net)        # v3 family: patch-embed rows; other models: fp32 patch tensors (as train() feeds)
        numerics = getattr(net, "numerics", ops.get_numerics())
        mw = dataset.max_window(len(scales))
        # trainer=None: validation never writes into a captured training step's static inputs
        self._feed = PairFeed(dataset.tiles, scales, self.batch, mw, rows=rows, numerics=numerics) if self.n_full else None
        self._tail = PairFeed(dataset.tiles, scales, tail, mw, rows=rows, numerics=numerics) if tail else None
        self._edges = {}
        for b in ([self.batch] if self.n_full else []) + ([tail] if tail else []):
            i = torch.arange(b, dtype=torch.int32, device=dev)
            self._edges[b] = torch.stack((i, i + b), 1).contiguous()
        self._simi = torch.empty(N, dtype=torch.float32, device=dev)
        self._term = torch.empty(N, dtype=torch.float32, device=dev)
        self._d2 = torch.empty(N, dtype=torch.float32, device=dev)
        self._th = torch.from_numpy(self.thresholds).to(dev)
        self._block = torch.empty(2 * len(self.thresholds) + 2, dtype=torch.int64, device=dev)

    @property
    def simi(self) -> torch.Tensor:
        """fp32 [N]: per pair (in the draw's position order) the sweep's distance of its two embeddings (last run)."""
        return self._simi

    @property
    def term(self) -> torch.Tensor:
        """fp32 [N]: per pair the contrastive term (last run)."""
        return self._term

    def run(self) -> PairEvalResult:
        net, B = self.net, self.batch
        table = self.dataset.epoch(self.draw_key, B)
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                for s in range(len(table)):
                    b, off = table.pairs_in_step(s), s * B
                    feed = self._feed if s < self.n_full else self._tail
                    _, _, _, _, flag = feed.fill(table.step(s))
                    F = net(feed.both, feed.dboth)
                    if not (isinstance(F, torch.Tensor) and F.dim() == 2 and F.shape[0] == 2 * b and 1 <= F.shape[1] <= MAX_FEATURE_DIM
                            and F.dtype == torch.float32):
                        raise ValueError(f"the model's eval output must be a float32 [n, D] tensor with D <= {MAX_FEATURE_DIM} (the range "
                                         f"of the sweep's pinned distance order), got "
                                         f"{getattr(F, 'dtype', type(F).__name__)} {tuple(getattr(F, 'shape', ()))}")
                    F = F.contiguous()
                    simi, _ = ops.edge_similarity(F, self._edges[b], self.margin, validate=False)
                    self._simi[off:off + b].copy_(simi)
                    ops.contrastive_terms(F[:b], F[b:], flag, self.margin, d2=self._d2[off:off + b], term=self._term[off:off + b])
                ops.pair_eval_summary(self._term, self._simi, table.cols["flag"], self._th, validate=False, out=self._block)
        finally:
            net.train(was_training)
        block = self._block.cpu()
        for f in (self._feed, self._tail):
            if f is not None:
                f.check()
        T = len(self.thresholds)
        loss_sum = float(block[:1].view(torch.float64)[0])
        merged = block[2:].view(2, T).numpy()
        return PairEvalResult.from_counts(self.n_pairs, int(block[1]), loss_sum, self.margin, self.thresholds, merged[0], merged[1])


def format_result(r: PairEvalResult) -> str:
    """The validation part of train()'s per-epoch line."""
    return f"val loss {r.loss:.6f} P/R/F @ {r.margin:g} {r.precision:.4f}/{r.recall:.4f}/{r.f_score:.4f}"


__all__ = ["PairEvaluator", "PairEvalResult", "threshold_set", "default_thresholds", "prf", "format_result"]
