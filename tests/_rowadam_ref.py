"""Numpy fp64 restatement of row-sparse lazy Adam (include/ppgat.h ppgat_adam_rows;
optim.Adam with a sparse gradient) -- test infrastructure only.

The rule.  One global step count t per table.  A step names rows R (unique) and gives one gradient
row per name; for r in R and every column:
    g += wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
    p -= step_size m / (sqrt(v) / bc2s + eps),   step_size = lr / (1 - b1^t),  bc2s = sqrt(1 - b2^t)
and every row outside R keeps p, m and v as they are (no momentum step, no weight decay).
"""
from __future__ import annotations

import numpy as np


class LazyAdam:
    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.p = np.array(p, np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.t = 0
        self.lr, (self.b1, self.b2), self.eps, self.wd = lr, betas, eps, weight_decay

    def step(self, rows, grad_rows):
        """rows [k] unique, grad_rows [k, d]; the count advances whether or not k > 0."""
        rows = np.asarray(rows, np.int64)
        assert len(np.unique(rows)) == len(rows) and ((rows >= 0) & (rows < len(self.p))).all()
        self.t += 1
        ss = self.lr / (1.0 - self.b1 ** self.t)
        bc2s = np.sqrt(1.0 - self.b2 ** self.t)
        g = np.asarray(grad_rows, np.float64).reshape(len(rows), -1) + self.wd * self.p[rows]
        m = self.b1 * self.m[rows] + (1.0 - self.b1) * g
        v = self.b2 * self.v[rows] + (1.0 - self.b2) * g * g
        self.m[rows], self.v[rows] = m, v
        self.p[rows] = self.p[rows] - ss * m / (np.sqrt(v) / bc2s + self.eps)
