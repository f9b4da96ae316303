"""Shapes shared by the tall-forward-unit tests (tests/test_tl_tall.py on the CPU, tests/test_tl_tall_gpu.py on the
GPU): small chunks that force the tall layout (``tiled.TLFwdChunk(tall=True)``) through every section shape."""
import numpy as np
import scipy.sparse as sp


CASES = ["zipf", "short", "uniform", "hot", "widedim"]


def zipf_cols(rng, rows, dim, k, s=1.1):
    """``k`` distinct columns per row: a hot Zipf head (narrow rounds) over a sparse tail (wide entries)."""
    p = np.arange(1, dim + 1, dtype=np.float64) ** -s
    cdf = np.cumsum(p) / p.sum()
    col = np.minimum(np.searchsorted(cdf, rng.random((rows, k))), dim - 1)
    return col


def csr_of(rows, dim, col, rng):
    r = np.repeat(np.arange(rows), col.shape[1])
    x = sp.csr_matrix((np.ones(col.size), (r, col.reshape(-1))), shape=(rows, dim))   # duplicates merged
    x.data = rng.normal(size=x.nnz)
    x.sort_indices()
    return x


def make_case(name):
    """name -> (csr matrix, what the chunk must hold: narrow rounds?, wide entries?, per-round wide bases?)."""
    rng = np.random.default_rng(CASES.index(name))
    if name == "zipf":        # 2 full tall units + a ragged one whose last sub-block is partial
        rows, dim = 9692, 3000
        return csr_of(rows, dim, zipf_cols(rng, rows, dim, 12), rng), True, True, False
    if name == "short":       # one ragged unit, fewer rows than one sub-block
        rows, dim = 700, 3000
        return csr_of(rows, dim, zipf_cols(rng, rows, dim, 12), rng), True, True, False
    if name == "uniform":     # uniform columns: no narrow round anywhere
        rows, dim = 5000, 3000
        return csr_of(rows, dim, rng.integers(0, dim, (rows, 6)), rng), False, True, False
    if name == "hot":         # 8 distinct of 40 hot columns per row, full sub-blocks (32 rounds each): no wide entry
        rows, dim = 5120, 3000
        col = np.argsort(rng.random((rows, 40)), axis=1)[:, :8]
        return csr_of(rows, dim, col, rng), True, False, False
    if name == "widedim":     # col << 12 overflows 32 bits: per-round bases of the wide section
        rows, dim = 5000, 3_000_000
        col = np.where(rng.random((rows, 10)) < 0.5, zipf_cols(rng, rows, 3000, 10), rng.integers(0, dim, (rows, 10)))
        return csr_of(rows, dim, col, rng), True, True, True
    raise KeyError(name)


