"""Shapes of the tile-group tests (tests/test_tl_tgroup.py, tests/test_tl_tgroup_gpu.py): Zipf columns over 70 001
features = 69 column tiles of 1024: 17 complete quadruples, a leftover tile and a ragged last tile."""
import numpy as np
import scipy.sparse as sp

DIM = 70_001
ITEM_ENTRIES = 1024          # the hottest tiles hold more entries than that: multi-item tiles next to the groups
EMPTY_TILE = 9               # columns [9216, 10240) hold nothing: an empty tile inside group 2


def make_matrix(rows: int, seed: int = 0, wide_exponents: bool = False) -> sp.csr_matrix:
    """``rows`` x DIM, 24 Zipf-distributed columns per row (hot head: dense tiles with narrow rounds; tail: a few
    entries per tile) plus 6 columns of tile 12 on the first 60 rows (a single-item tile with narrow AND wide rounds).
    ``wide_exponents``: values spread over 2^-20 .. 2^20, so a sum's bits depend on the order of its additions."""
    rng = np.random.default_rng(seed)
    k = 24
    p = np.arange(1, DIM + 1, dtype=np.float64) ** -1.05
    cdf = np.cumsum(p) / p.sum()
    col = np.minimum(np.searchsorted(cdf, rng.random((rows, k))), DIM - 1)
    mid = np.zeros((rows, 6), dtype=np.int64)                 # (column 0 again: merged by sum_duplicates)
    mid[:60] = 12 * 1024 + rng.integers(0, 1024, (60, 6))
    col = np.concatenate([col, mid], 1)
    col[:, 0] = DIM - 1                                       # the ragged last tile is never empty
    hole = (col >= EMPTY_TILE * 1024) & (col < (EMPTY_TILE + 1) * 1024)
    col[hole] = DIM - 1 - (col[hole] - EMPTY_TILE * 1024)     # (to the last tiles, far from every item limit)
    val = rng.uniform(0.5, 1.5, col.shape)
    if wide_exponents:
        val = val * 2.0 ** rng.integers(-20, 21, col.shape)
    row = np.repeat(np.arange(rows), col.shape[1])
    x = sp.coo_matrix((val.reshape(-1), (row, col.reshape(-1))), shape=(rows, DIM)).tocsr()
    x.sum_duplicates()
    x.sort_indices()
    return x
