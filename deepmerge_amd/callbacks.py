"""Drop-in for the reference's `callbacks.LossHistory` (callbacks.py): one line per epoch in three text files under
`log_dir/loss_<%Y_%m_%d_%H_%M_%S>/` -- `epoch_loss_<t>.txt`, `epoch_val_loss_<t>.txt`, `epoch_f_score_<t>.txt`, each value
written as `str(value)` and a newline.  Upstream defines `append_loss` twice; the three-argument definition is the one in force.

The PNG curve (`epoch_loss_<t>.png`, with Savitzky-Golay smoothed copies of both curves) is drawn only when matplotlib (a bare
Agg Figure) and scipy import; otherwise it is skipped silently.  The plot is not part of the contract.
"""
from __future__ import annotations

import datetime
import os
from typing import List


class LossHistory:
    def __init__(self, log_dir: str):
        self.log_dir = log_dir
        self.time_str = datetime.datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
        self.save_path = os.path.join(log_dir, "loss_" + self.time_str)
        self.losses: List[float] = []
        self.val_loss: List[float] = []
        self.f_scores: List[float] = []
        os.makedirs(self.save_path, exist_ok=True)

    def _path(self, kind: str, ext: str = "txt") -> str:
        return os.path.join(self.save_path, f"epoch_{kind}_{self.time_str}.{ext}")

    def append_loss(self, loss, val_loss, f_score):
        self.losses.append(loss)
        self.val_loss.append(val_loss)
        self.f_scores.append(f_score)
        for kind, value in (("loss", loss), ("val_loss", val_loss), ("f_score", f_score)):
            with open(self._path(kind), "a") as f:
                f.write(str(value))
                f.write("\n")
        self.loss_plot()

    def loss_plot(self):
        try:
            from matplotlib.figure import Figure       # a bare Figure renders with Agg and leaves pyplot's backend alone
            from scipy import signal
        except Exception:
            return
        iters = range(len(self.losses))
        fig = Figure()
        ax = fig.subplots()
        ax.plot(iters, self.losses, linewidth=2, label="train loss")
        ax.plot(iters, self.val_loss, linewidth=2, label="val loss")
        window = 5 if len(self.losses) < 25 else 15
        try:
            ax.plot(iters, signal.savgol_filter(self.losses, window, 3), linestyle="--", linewidth=2, label="smooth train loss")
            ax.plot(iters, signal.savgol_filter(self.val_loss, window, 3), linestyle="--", linewidth=2, label="smooth val loss")
        except Exception:                    # fewer epochs than the smoothing window
            pass
        ax.grid()
        ax.set_xlabel("Epoch")
        ax.set_ylabel("Loss")
        ax.legend()
        fig.savefig(self._path("loss", "png"))
