"""Per-feature statistics on the GPU: ``DeviceGLMData.column_stats`` (``tl_colsum_kernel`` / ``tl_colminmax_kernel``
over the transpose copies) and ``BasicStatisticalSummary.from_device`` on top of it.

EXACT: on the designed matrices of test_tl_bits_layout.py (values multiples of 0.5 of magnitude <= 2, fewer than
2^16 per column: sum v, sum v^2 and sum |v| are exact in fp64 in any order) all six statistics are ``torch.equal``
to numpy on the float64 matrix at tile widths 5, 8, 10, 11 and 12 bits for bf16, fp32 and fp64 shards — two chunks,
a split tile through the two-level combine, narrow rounds with 64 / 32 / 16-key windows, fused bf16 records; plus
the two-array bf16 narrow rounds (``FUSE = 0``) and the plain stream order (``INTERLEAVE = 0``). A tolerance would
not notice one lost entry (test_tl_bits_layout.py shows that).
SEMANTICS against ``BasicStatisticalSummary.compute`` at the tolerance of the CPU test of the same function
(test_tiled_layout.py: rtol = atol = 1e-12): relabelled shard with an intercept column split over many items, an
all-negative, an all-positive and an empty column, an explicit zero; a shard in column windows.
REPEATABILITY: two calls, the same bits."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.data.matrix import LabeledData
from photon_ml_amd.stat.summary import BasicStatisticalSummary
from test_tl_bits_gpu import _build

pytestmark = pytest.mark.gpu

WIDTHS = ((5, 5), (8, 8), (10, 10), (11, 11), (12, 12))
NAMES = ("sum", "sum of squares", "sum of |v|", "stored entries", "max", "min")
FIELDS = ("mean", "variance", "num_nonzeros", "max", "min", "norm_l1", "norm_l2", "mean_abs")


def numpy_column_stats(x):
    """(sum v, sum v^2, sum |v|, stored entries, max, min) of a scipy matrix in float64; max / min over the stored
    entries only (-inf / +inf for a column without any), as ``column_stats`` defines them."""
    x = sp.csc_matrix(x, dtype=np.float64)
    d = x.shape[1]
    cnt = np.diff(x.indptr)
    col = np.repeat(np.arange(d), cnt)
    out = [np.zeros(d) for _ in range(3)]
    np.add.at(out[0], col, x.data)
    np.add.at(out[1], col, x.data * x.data)
    np.add.at(out[2], col, np.abs(x.data))
    mx, mn = np.full(d, -np.inf), np.full(d, np.inf)
    np.maximum.at(mx, col, x.data)
    np.minimum.at(mn, col, x.data)
    return out + [cnt.astype(np.float64), mx, mn]


def assert_exact(dev, x):
    got = dev.column_stats()
    assert len(got) == 6
    for name, g, w in zip(NAMES, got, numpy_column_stats(x)):
        w = torch.from_numpy(w)
        assert g.is_cuda and g.dtype == torch.float64 and g.shape == w.shape
        g = g.cpu()
        bad = torch.nonzero(g != w).reshape(-1)
        assert torch.equal(g, w), (f"{name}: {bad.numel()} of {w.numel()} columns differ, first at "
                                   f"{bad[:5].tolist()}: {g[bad[:5]].tolist()} != {w[bad[:5]].tolist()}")


@pytest.mark.parametrize("precision", ["bf16", "f32", "f64"])
@pytest.mark.parametrize("bits", WIDTHS, ids=lambda b: f"c{b[1]}")
def test_column_stats_equal_numpy_bit_for_bit(bits, precision):
    case, _, dev, _, _ = _build(bits, precision)
    assert len(dev.csc) == 2 and all(t.nmt >= 1 and t.n_narrow_rounds > 0 for t in dev.csc)
    assert all(t.fused == (precision == "bf16") for t in dev.csc)
    assert_exact(dev, case.x)


def test_two_array_bf16_narrow_rounds(monkeypatch):
    from photon_ml_amd.ops import tiled
    monkeypatch.setattr(tiled, "FUSE", 0)
    case, _, dev, _, _ = _build((11, 11), "bf16")
    assert all(not t.fused and t.n_narrow_rounds > 0 for t in dev.csc)
    assert_exact(dev, case.x)


@pytest.mark.parametrize("bits,precision", [((10, 10), "f64"), ((12, 12), "bf16")])
def test_plain_stream_order(monkeypatch, bits, precision):
    from photon_ml_amd.ops import tiled
    monkeypatch.setattr(tiled, "INTERLEAVE", 0)
    case, _, dev, _, _ = _build(bits, precision)
    assert all(not t.il and t.n_narrow_rounds == 0 and t.nmt >= 1 for t in dev.csc)
    assert_exact(dev, case.x)


# ---- semantics ------------------------------------------------------------------------------------------------
N, D, CHUNK = 3000, 200, 1600
INTERCEPT, NEG, POS, EMPTY, ZERO = 0, 5, 7, 9, 11


def semantics_matrix(seed=2):
    rng = np.random.default_rng(seed)
    x = sp.random(N, D, density=0.05, format="lil", random_state=seed, data_rvs=lambda k: rng.normal(size=k))
    for c in (INTERCEPT, NEG, POS, EMPTY):
        x[:, c] = 0.0
    x[:, INTERCEPT] = 1.0
    rows = rng.choice(N, size=40, replace=False)
    x[rows[:20], NEG] = -np.abs(rng.normal(size=20)) - 0.1
    x[rows[20:], POS] = np.abs(rng.normal(size=20)) + 0.1
    x = x.tocsr()
    # one stored (explicit) zero: it counts as an entry and takes part in max / min
    r0 = int(np.flatnonzero(np.diff(x.indptr) > 1)[0])
    k = x.indptr[r0] + 1
    assert x.indices[k] != INTERCEPT
    x.data[k] = 0.0
    return x, int(x.indices[k])


@pytest.fixture(scope="module")
def semantics():
    from photon_ml_amd.ops.device import DeviceGLMData
    x, zero_col = semantics_matrix()
    data = LabeledData(x, np.zeros(N))
    dev = DeviceGLMData.from_labeled(data, "cuda", "f64", chunk_rows=CHUNK, relabel=True, layout="tiled",
                                     item_entries=256)
    return x, zero_col, dev, BasicStatisticalSummary.compute(x)


def assert_summaries_close(got, want):
    assert got.count == want.count
    for f in FIELDS:
        torch.testing.assert_close(getattr(got, f), getattr(want, f), rtol=1e-12, atol=1e-12, msg=lambda m: f"{f}: {m}")


def test_from_device_matches_compute_on_a_relabelled_shard(semantics):
    x, zero_col, dev, want = semantics
    assert len(dev.csc) == 2 and dev.old_of_new is not None
    assert all(t.nitems > 40 and t.nmt >= 1 for t in dev.csc)      # the hot tile: many items, two-level combine
    got = BasicStatisticalSummary.from_device(dev)
    assert_summaries_close(got, want)
    assert got.num_nonzeros[INTERCEPT] == N and got.max[INTERCEPT] == 1.0 and got.min[INTERCEPT] == 1.0
    assert abs(float(got.variance[INTERCEPT])) < 1e-12 and got.mean[INTERCEPT] == 1.0
    assert got.max[NEG] == 0.0 and got.min[NEG] < 0.0              # implicit zeros: fewer entries than rows
    assert got.min[POS] == 0.0 and got.max[POS] > 0.0
    assert got.max[EMPTY] == 0.0 and got.min[EMPTY] == 0.0 and got.num_nonzeros[EMPTY] == 0
    assert got.num_nonzeros[zero_col] == np.diff(x.tocsc().indptr)[zero_col]    # the stored zero is an entry
    raw = dev.column_stats()
    assert raw[4][EMPTY] == float("-inf") and raw[5][EMPTY] == float("inf")     # max / min over stored entries only


def test_column_stats_are_bitwise_repeatable(semantics):
    _, _, dev, _ = semantics
    a, b = dev.column_stats(), dev.column_stats()
    for name, s, t in zip(NAMES, a, b):
        assert torch.equal(s, t), name


def test_from_device_on_a_shard_in_column_windows():
    """Chunks stored in their own (tile-aligned) column windows: chunk 1 starts at column 1024."""
    from photon_ml_amd.ops.device import DeviceGLMData
    rng = np.random.default_rng(5)
    m, dim = 700, 2700
    blocks = [sp.random(m, 1500, density=0.02, format="csr", random_state=1, data_rvs=lambda k: rng.normal(size=k)),
              sp.random(m - 50, 1500, density=0.02, format="csr", random_state=2, data_rvs=lambda k: rng.normal(size=k))]
    x = sp.vstack([sp.hstack([blocks[0], sp.csr_matrix((m, dim - 1500))]),
                   sp.hstack([sp.csr_matrix((m - 50, 1100)), blocks[1], sp.csr_matrix((m - 50, dim - 2600))])]).tocsr()
    n = x.shape[0]
    z = np.zeros(n)
    dev = DeviceGLMData.from_device_csr(torch.from_numpy(x.indptr.astype(np.int64)),
                                        torch.from_numpy(x.indices.astype(np.int64)), torch.from_numpy(x.data),
                                        z, z, np.ones(n), dim, "cuda", "f64", chunk_rows=m, col_windows=True)
    assert dev.col_lo[0] == 0 and dev.col_lo[1] == 1024 and dev.csc[1].dim < dim
    assert_summaries_close(BasicStatisticalSummary.from_device(dev), BasicStatisticalSummary.compute(x))


def test_wrapper_rejects_short_result_buffers(semantics):
    """``PML_CHECK_KERNEL_INPUTS=1`` (on in the tests): the last tile is partial, the kernels write columns below
    the chunk's ``dim`` only, and the wrapper refuses result buffers shorter than that before anything is launched."""
    from photon_ml_amd.ops.native import tl_colstats
    _, _, dev, _ = semantics
    outs = [torch.zeros(dev.dim - 1, dtype=torch.float64, device="cuda") for _ in range(6)]
    with pytest.raises(ValueError, match="result buffers"):
        tl_colstats(dev.prec, dev.csc[0], 0, outs, dev.parts)
    with pytest.raises(ValueError, match="scratch"):
        tl_colstats(dev.prec, dev.csc[0], 0, [torch.zeros(dev.dim, dtype=torch.float64, device="cuda")
                                             for _ in range(6)], dev.parts[:1])


def test_segmented_shard_still_raises():
    from photon_ml_amd.ops.device import DeviceGLMData
    x, _ = semantics_matrix()
    dev = DeviceGLMData.from_labeled(LabeledData(x, np.zeros(N)), "cuda", "f64", layout="segmented")
    with pytest.raises(ValueError, match="tiled"):
        BasicStatisticalSummary.from_device(dev)
    with pytest.raises(ValueError, match="tiled"):
        dev.column_stats()
