"""``prior_fold_kernel`` (incremental training: a Gaussian prior folded into the entity-sorted CSR) against torch fp64.

The kernel reads the CSR once: prior margins ``m[r] = sum_k val[k] mu[pos[k]]`` from the original values, then
``val[k] *= sigma[pos[k]]`` in place. The scaled values are a single fp64 multiply each (bitwise the torch product);
the margins are an fp64 sum in another order than torch's, so they agree within the standard summation bound ``n_r
2^-53 sum_k |val_k mu_k|`` per row. Two launches give the same bits (no atomics).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# row lengths: every length around the 16-lane row width and its multiples, one long row; empty rows first, in the
# middle and last
LENGTHS = [0, 0, 1, 15, 16, 17, 0, 31, 32, 33, 0, 0, 64, 65, 1000, 0]
ENT_DIMS = [40, 7, 300]               # three entities' coefficient ranges of the packed vector


def make_csr(seed=0):
    rng = np.random.default_rng(seed)
    d_total = sum(ENT_DIMS)
    base = np.concatenate([[0], np.cumsum(ENT_DIMS)])
    nip = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    pos = np.empty(nip[-1], dtype=np.int64)
    for r, n in enumerate(LENGTHS):
        e = r % 3                                                        # the row's entity
        pos[nip[r]:nip[r + 1]] = base[e] + rng.integers(0, ENT_DIMS[e], size=n)
    val = rng.normal(size=nip[-1])
    mu = rng.normal(size=d_total)
    sigma = np.sqrt(rng.uniform(0.25, 4.0, size=d_total))
    return tuple(torch.from_numpy(a) for a in (nip, pos, val, mu, sigma))


@pytest.fixture(scope="module")
def csr():
    return make_csr()


def reference(nip, pos, val, mu, sigma):
    n = nip.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n), nip[1:] - nip[:-1])
    prod = val * mu[pos]
    m = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, prod)
    bound = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, prod.abs()) * (nip[1:] - nip[:-1]) * 2.0 ** -53
    return m, val * sigma[pos], bound


def run(nip, pos, val, mu, sigma):
    from photon_ml_amd.ops.native import prior_fold
    v = val.cuda().clone()
    m = prior_fold(nip.cuda(), pos.cuda(), v, mu.cuda(), sigma.cuda())
    torch.cuda.synchronize()
    return m.cpu(), v.cpu()


def test_prior_fold_matches_torch_fp64(csr):
    m_ref, v_ref, bound = reference(*csr)
    m, v = run(*csr)
    assert torch.equal(v, v_ref)                                  # one fp64 multiply per entry: bitwise
    err = (m - m_ref).abs()
    print("prior margins: max |err| / bound =", float((err / bound.clamp(min=1e-300)).max()))
    assert bool((err <= bound).all()), (err, bound)
    lens = csr[0][1:] - csr[0][:-1]
    assert bool((m[lens == 0] == 0).all())                        # empty rows: written, and zero


def test_prior_fold_is_bitwise_repeatable(csr):
    m1, v1 = run(*csr)
    m2, v2 = run(*csr)
    assert torch.equal(m1, m2) and torch.equal(v1, v2)


def test_prior_fold_zero_rows():
    from photon_ml_amd.ops.native import prior_fold
    z = lambda dt: torch.zeros(0, dtype=dt, device="cuda")
    m = prior_fold(torch.zeros(1, dtype=torch.int64, device="cuda"), z(torch.int64), z(torch.float64),
                   torch.zeros(3, dtype=torch.float64, device="cuda"), torch.ones(3, dtype=torch.float64, device="cuda"))
    assert m.shape == (0,) and m.dtype == torch.float64


def test_prior_fold_input_validation_raises_before_launch(csr, monkeypatch):
    """PML_CHECK_KERNEL_INPUTS=1: a position equal to d_total and a negative sigma raise on the host; nothing is
    launched (the values stay untouched)."""
    from photon_ml_amd.ops.native import prior_fold
    monkeypatch.setenv("PML_CHECK_KERNEL_INPUTS", "1")
    nip, pos, val, mu, sigma = (t.cuda() for t in csr)
    bad_pos = pos.clone()
    bad_pos[5] = mu.numel()
    v = val.clone()
    with pytest.raises(ValueError, match="positions"):
        prior_fold(nip, bad_pos, v, mu, sigma)
    assert torch.equal(v, val)
    bad_sigma = sigma.clone()
    bad_sigma[3] = -1.0
    with pytest.raises(ValueError, match="sigma"):
        prior_fold(nip, pos, v, mu, bad_sigma)
    assert torch.equal(v, val)
    bad_nip = nip.clone()
    bad_nip[-1] += 1
    with pytest.raises(ValueError, match="row pointer"):
        prior_fold(nip=bad_nip, pos=pos, val=v, mu=mu, sigma=sigma)
    assert torch.equal(v, val)
    m = prior_fold(nip, pos, v, mu, sigma)                        # valid inputs pass the same checks
    assert m.numel() == nip.numel() - 1
