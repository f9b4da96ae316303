"""Shared generators and yardsticks of the FULL-variance tests (test_full_variance.py, test_full_variance_gpu.py).

A block-diagonal problem is a list of entity shapes ``(n_e, d_e)``: entity e owns the rows ``row_ptr[e]:row_ptr[e+1]``
and the packed coefficients ``col_ptr[e]:col_ptr[e+1]``; its rows hold at most 51 entries with distinct, increasing
columns inside the entity's range (the canonical CSR the kernels need), values N(0, 1).
"""
import numpy as np
import torch

MAX_ROW_NNZ = 51


class BlockProblem:
    def __init__(self, shapes, seed=0, weights=(0.5, 1.0, 2.0), zero_weight_fraction=0.0, duplicate_rows=()):
        """``duplicate_rows``: entity indices whose rows are all copies of their first two rows (singular Gram
        matrix); ``zero_weight_fraction``: share of every entity's rows that get weight 0."""
        rng = np.random.default_rng(seed)
        self.shapes = [(int(n), int(d)) for n, d in shapes]
        n_e = np.array([s[0] for s in self.shapes], dtype=np.int64)
        d_e = np.array([s[1] for s in self.shapes], dtype=np.int64)
        self.row_ptr = np.concatenate([[0], np.cumsum(n_e)])
        self.col_ptr = np.concatenate([[0], np.cumsum(d_e)])
        indptr, cols, vals = [0], [], []
        for e, (n, d) in enumerate(self.shapes):
            rows = []
            for i in range(n):
                if e in duplicate_rows and i >= 2:
                    c, v = rows[i % 2]
                else:
                    k = int(rng.integers(1, min(d, MAX_ROW_NNZ) + 1)) if d else 0
                    c = np.sort(rng.choice(d, size=k, replace=False)) if d else np.zeros(0, np.int64)
                    v = rng.standard_normal(k)
                rows.append((c, v))
                cols.append(c + self.col_ptr[e])
                vals.append(v)
                indptr.append(indptr[-1] + len(c))
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.cols = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
        self.vals = np.concatenate(vals) if vals else np.zeros(0)
        N = int(self.row_ptr[-1])
        self.w = rng.choice(np.asarray(weights, dtype=np.float64), size=N)
        if zero_weight_fraction:
            for e in range(len(self.shapes)):
                r0, r1 = self.row_ptr[e], self.row_ptr[e + 1]
                k = int((r1 - r0) * zero_weight_fraction)
                if k:
                    self.w[rng.choice(np.arange(r0, r1), size=k, replace=False)] = 0.0
        # curvature of a logistic-like loss: weight x l'' with l'' in (0.05, 0.25)
        self.c = self.w * rng.uniform(0.05, 0.25, size=N)

    @property
    def n_entities(self):
        return len(self.shapes)

    def entity_dense(self, e):
        """``X_e [n_e, d_e]`` as a dense numpy matrix."""
        n, d = self.shapes[e]
        X = np.zeros((n, d))
        for i in range(n):
            r = self.row_ptr[e] + i
            k0, k1 = self.indptr[r], self.indptr[r + 1]
            X[i, self.cols[k0:k1] - self.col_ptr[e]] = self.vals[k0:k1]
        return X

    def hessian(self, e, lam, c=None):
        c = self.c if c is None else c
        X = self.entity_dense(e)
        ce = c[self.row_ptr[e]:self.row_ptr[e + 1]]
        return X.T @ (ce[:, None] * X) + lam * np.eye(X.shape[1])

    def numpy_variances(self, lam, c=None, cond_max=None):
        """``diag(inv(H_e))`` of every entity with ``numpy.linalg.inv``, packed like ``col_ptr``; with ``cond_max``
        asserts ``cond(H_e) <= cond_max`` so that the yardstick itself stays inside the tests' tolerance."""
        out = np.zeros(int(self.col_ptr[-1]))
        for e, (n, d) in enumerate(self.shapes):
            if d == 0:
                continue
            H = self.hessian(e, lam, c)
            if cond_max is not None:
                cond = np.linalg.cond(H)
                assert cond <= cond_max, (e, self.shapes[e], cond)
            out[self.col_ptr[e]:self.col_ptr[e + 1]] = np.diag(np.linalg.inv(H))
        return out

    def tensors(self, device="cpu"):
        """``(row_ptr, col_ptr, (indptr, cols, vals), c)`` as torch tensors on ``device``."""
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return t(self.row_ptr), t(self.col_ptr), (t(self.indptr), t(self.cols), t(self.vals)), t(self.c)


def mixed_shapes(seed=0, count=40):
    """About ``count`` entities: tall, square and wide, with an entity without rows in the middle."""
    rng = np.random.default_rng(seed)
    shapes = []
    for k in range(count):
        kind = k % 3
        if kind == 0:
            d = int(rng.integers(1, 24))
            shapes.append((int(d * rng.integers(2, 5)), d))
        elif kind == 1:
            d = int(rng.integers(1, 30))
            shapes.append((d, d))
        else:
            n = int(rng.integers(1, 20))
            shapes.append((n, int(n + rng.integers(1, 60))))
    shapes.insert(count // 2, (0, 7))
    return shapes


def relative_error(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want))) if want.size else 0.0
