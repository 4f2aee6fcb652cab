"""The sampling state of a running decode batch: per-row temperature, top-k, top-p and min-p held in device tensors that
ops.sample_tokens reads in its one launch (mio_sample_tokens).  A generation loop owns one Sampler per batch, calls set_row
when a request joins or changes its parameters, and calls the sampler on every step's logits."""
from __future__ import annotations

import torch

from . import ops


class Sampler:
    """Per-row sampling parameters of `batch` rows on `device`.  Rows start greedy (temperature 0) with every filter off
    (top_k 0, top_p 1, min_p 0).  set_row writes in place and moves no pointer, so a step captured in a graph stays valid; the
    uniforms live in self.u and are redrawn in place by every call."""

    def __init__(self, batch: int, device):
        if batch < 0:
            raise ValueError("Sampler: batch must not be negative")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
        self.batch = batch
        self.temperature = torch.zeros(batch, dtype=torch.float32, device=device)
        self.top_k = torch.zeros(batch, dtype=torch.int32, device=device)
        self.top_p = torch.ones(batch, dtype=torch.float32, device=device)
        self.min_p = torch.zeros(batch, dtype=torch.float32, device=device)
        self.u = torch.zeros(batch, dtype=torch.float32, device=device)

    def set_row(self, i: int, temperature=None, top_k=None, top_p=None, min_p=None) -> None:
        """Update row i in place; an argument left None keeps its value."""
        if not 0 <= i < self.batch:
            raise IndexError(f"Sampler: row {i} of a batch of {self.batch}")
        for t, v in ((self.temperature, temperature), (self.top_k, top_k), (self.top_p, top_p), (self.min_p, min_p)):
            if v is not None:
                t[i].fill_(v)

    def __call__(self, logits: torch.Tensor, generator=None) -> torch.Tensor:
        """tokens [batch] for logits [batch, V]: fresh uniforms into self.u, then one launch."""
        if logits.dim() != 2 or logits.shape[0] != self.batch:
            raise ValueError(f"Sampler: logits must be [{self.batch}, V], got {tuple(logits.shape)}")
        self.u.uniform_(0.0, 1.0, generator=generator)
        return ops.sample_tokens(logits, self.temperature, self.top_k, self.top_p, self.min_p, u=self.u)
