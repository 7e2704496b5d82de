"""Learned task weights (homoscedastic-uncertainty weighting, Kendall, Gal and Cipolla 2018): one log-variance per enabled task."""
import torch
from torch import nn


class TaskLogVariance(nn.Module):
    """``log_var[t]`` = s_t of the objective J = sum_t w_t (exp(-s_t) L_t + s_t), one f32 element per enabled task in the step's
    task order, initial value 0 (exp(-0) = 1: the first step is the fixed-weight step).  Its gradient is written by the step
    (egk_task_scale_grad), never by autograd.  Not part of the backbone's or any task's state dict: a checkpoint carries it under
    its own top-level entry (train.task_weighting_state), the reference's key layout stays."""

    def __init__(self, tasks):
        super().__init__()
        self.tasks = tuple(tasks)
        if not self.tasks:
            raise ValueError("TaskLogVariance: no enabled task")
        self.log_var = nn.Parameter(torch.zeros(len(self.tasks), dtype=torch.float32))

    def configure_optimizers(self):
        return [self.log_var]

    @torch.no_grad()
    def effective_weights(self, weights) -> dict:
        """{task: (s_t, w_t exp(-s_t))} as Python floats (one device synchronisation)."""
        s = self.log_var.detach().double().cpu()
        return {t: (float(s[i]), float(weights[t]) * float(torch.exp(-s[i]))) for i, t in enumerate(self.tasks)}
