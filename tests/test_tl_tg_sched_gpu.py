"""The scheduler of the grouped shard-wide transpose (``tl_tg_multi_kernel``: persistent work-groups drawing groups and
items from two ticket counters, one work-group running several units on the same 32 KB of LDS). Every case forces the
tile groups on (``tgroup=True``, what ``PML_TL_TGROUP=1`` does) and compares the shard-wide pass

* BIT FOR BIT with the per-chunk launches (``tl_multi=0``: ``tl_tg_kernel`` + ``tl_t_kernel``, one unit per
  work-group, no scheduler), and
* with the fp64 CPU product at the tolerance of tests/test_tl_tgroup_gpu.py.

Shapes (tests/tl_tgroup_util.py, 70 001 columns = 69 tiles, Zipf columns, items of 1024 entries): 3 chunks of 2^14
rows (groups and split-tile items), one chunk of 2^12 rows (far fewer units than work-groups), 128 chunks of 2^10 rows
(2048 groups + 2560 items on a grid of 5 work-groups per CU: every work-group runs units back to back, of both kinds
once a queue runs out), and two uniform shards that hold only groups / only items."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from photon_ml_amd.ops.tiled import TG_EMPTY
from test_tl_tgroup_gpu import TOL, close
from tl_tgroup_util import DIM, ITEM_ENTRIES, make_matrix

pytestmark = pytest.mark.gpu

SLOTS = 5                     # work-groups per CU of the persistent launch (TL_TG_SLOTS)
_SHARDS = {}


def uniform_matrix(rows, dim, k, seed):
    rng = np.random.default_rng(seed)
    col = rng.integers(0, dim, (rows, k))
    x = sp.coo_matrix((rng.uniform(0.5, 1.5, col.size), (np.repeat(np.arange(rows), k), col.reshape(-1))),
                      shape=(rows, dim)).tocsr()
    x.sum_duplicates()
    x.sort_indices()
    return x


# name: (matrix, dim, chunk rows, item entries)
SHAPES = {
    "plain": (lambda: make_matrix(3 << 14, seed=3), DIM, 1 << 14, ITEM_ENTRIES),
    "few": (lambda: make_matrix(1 << 12, seed=1), DIM, 1 << 12, ITEM_ENTRIES),
    "many": (lambda: make_matrix(128 << 10, seed=4), DIM, 1 << 10, ITEM_ENTRIES),
    "groups_only": (lambda: uniform_matrix(1 << 12, 17 * 4096, 8, 2), 17 * 4096, 1 << 12, 1 << 18),
    "items_only": (lambda: uniform_matrix(1 << 12, DIM, 30, 2), DIM, 1 << 12, ITEM_ENTRIES),
}


def shard(name, precision="bf16"):
    """(device shard with its shard-wide tables, stored matrix, row vector on a 2^-10 grid); built once."""
    from photon_ml_amd.ops.device import DeviceGLMData
    key = (name, precision)
    if key not in _SHARDS:
        make, dim, chunk_rows, item_entries = SHAPES[name]
        x = make()
        val = torch.from_numpy(x.data).to(torch.bfloat16 if precision == "bf16" else torch.float32).double()
        x = sp.csr_matrix((val.numpy(), x.indices, x.indptr), shape=x.shape)          # what the shard stores
        n = x.shape[0]
        one = torch.ones(n, dtype=torch.float64)
        dev = DeviceGLMData.from_device_csr(
            torch.from_numpy(x.indptr.astype(np.int64)), torch.from_numpy(x.indices.astype(np.int64)), val,
            torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), one, dim, "cuda", precision,
            chunk_rows=chunk_rows, item_entries=item_entries, tgroup=True)
        dev._build_multi_t()
        assert dev._multi_t is not None and dev.validate() is not False
        r = torch.from_numpy(np.random.default_rng(7).integers(-60, 61, n) / 1024.0)
        _SHARDS[key] = (dev, x, r)
    return _SHARDS[key]


def transpose(dev, r, square, multi):
    """The transpose of the shard (permuted column order, as the kernels write it) through the shard-wide launch
    (``multi`` = 1) or the per-chunk launches (0)."""
    from photon_ml_amd.ops.native import configure
    G = torch.zeros(dev.dim, dtype=torch.float64, device="cuda")
    try:
        configure(tl_multi=multi)
        dev.t_all(r.cuda().to(dev.vdt), G, square=int(square))
    finally:
        configure(tl_multi=1)
    torch.cuda.synchronize()
    return G


def check(name, precision="bf16", square=False):
    dev, x, r = shard(name, precision)
    got = transpose(dev, r, square, 1)
    assert torch.equal(got, transpose(dev, r, square, 0))
    want = torch.from_numpy((x.multiply(x) if square else x).T.tocsr() @ r.numpy())
    assert close(dev._unperm(got), want, TOL[precision])
    return dev


def grid():
    return SLOTS * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_groups_and_items(precision):
    dev = check("plain", precision)
    mt = dev._multi_t
    assert mt.ngroups > 0 and mt.nitems > 0 and mt.nmt > 0 and len(dev.csc) == 3


def test_one_queue_empty_from_the_start():
    """Groups without items: the item slots fall over to the groups at once and every work-group leaves through the
    both-empty exit. Items without groups: the shard-wide launch of the ungrouped kernel."""
    mt = check("groups_only")._multi_t
    assert mt.ngroups > 0 and mt.nitems == 0 and mt.desc.ngroups == mt.ngroups and mt.desc.nitems == 0
    mt = check("items_only")._multi_t
    assert mt.ngroups == 0 and mt.nitems > 0 and mt.desc.ngroups == 0 and mt.desc.nitems == mt.nitems


def test_far_fewer_units_than_work_groups():
    mt = check("few")._multi_t
    assert 0 < mt.ngroups and 0 < mt.nitems and 4 * (mt.ngroups + mt.nitems) < grid()


@pytest.mark.parametrize("square", [False, True])
def test_work_groups_run_units_back_to_back(square):
    """More groups and more items than work-groups, and three units per work-group overall: every slot has units of
    its own kind to run one after the other on the same LDS, and takes the other kind when its queue runs out."""
    mt = check("many", square=square)._multi_t
    assert mt.ngroups >= grid() and mt.nitems >= grid() and mt.ngroups + mt.nitems >= 3 * grid()


def launch(dev, desc, r, G, square=0):
    from photon_ml_amd.ops.native import check as rc_check, stream_handle
    rc_check(dev.lib.pml_tl_t_multi(dev.prec, ctypes.byref(desc), r.data_ptr(), square, G.data_ptr(),
                                    dev.parts.data_ptr(), stream_handle(dev.device)), "tl_t_multi")


def test_live_flags_skip_units_and_nothing_else():
    """About half the items and half the groups switched off: a skipped unit uses up its ticket and writes nothing
    (its partial rows keep the fill value), every other unit's partial rows are those of the full pass."""
    dev, _, r = shard("many")
    mt = dev._multi_t
    C = 1 << mt.cbits
    rr = r.cuda().to(dev.vdt)
    nrows = mt.nparts * C
    G = torch.zeros(dev.dim, dtype=torch.float64, device="cuda")
    dev.parts.fill_(7.0)
    launch(dev, mt.desc, rr, G)
    full = dev.parts[:nrows].clone().reshape(-1, C)
    rng = np.random.default_rng(1)
    live = torch.from_numpy((rng.random(mt.nitems) < 0.5).astype(np.uint8)).cuda()
    live_g = torch.from_numpy((rng.random(mt.ngroups) < 0.5).astype(np.uint8)).cuda()
    desc = type(mt.desc).from_buffer_copy(mt.desc)
    desc.live, desc.live_g = live.data_ptr(), live_g.data_ptr()
    dev.parts.fill_(7.0)
    launch(dev, desc, rr, torch.zeros_like(G))
    got = dev.parts[:nrows].clone().reshape(-1, C)
    ip, gp = mt.items[:, 4].to(torch.int64), mt.groups[:, 1:5].to(torch.int64)
    assert bool((ip >= 0).all()) and bool(((gp >= 0) | (gp == TG_EMPTY)).all())      # every unit writes partial rows
    on = torch.cat([ip[live.bool()], gp[live_g.bool()].reshape(-1)])
    off = torch.cat([ip[~live.bool()], gp[~live_g.bool()].reshape(-1)])
    on, off = on[on >= 0], off[off >= 0]
    assert on.numel() > 1000 and off.numel() > 1000 and on.numel() + off.numel() == mt.nparts
    assert torch.equal(got[on], full[on]) and bool((full[on] != 7.0).any())
    assert bool((got[off] == 7.0).all())


def test_counters_are_reset_before_every_launch():
    """Two passes queued back to back, then a gated one (flag 0, which returns before any ticket is drawn), then a
    third: the normal passes agree bit for bit, the gated one writes neither G nor a partial row."""
    dev, _, r = shard("many")
    mt = dev._multi_t
    rr = r.cuda().to(dev.vdt)
    nrows = mt.nparts << mt.cbits
    out = [torch.zeros(dev.dim, dtype=torch.float64, device="cuda") for _ in range(3)]
    launch(dev, mt.desc, rr, out[0])
    launch(dev, mt.desc, rr, out[1])
    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    kept = torch.full((dev.dim,), 7.0, dtype=torch.float64, device="cuda")
    dev.parts.zero_()                      # (the combine adds the partial rows whether or not a unit ran)
    dev.lib.pml_set_gate(gate.data_ptr())
    try:
        launch(dev, mt.desc, rr, kept)
    finally:
        dev.lib.pml_set_gate(None)
    torch.cuda.synchronize()
    assert bool((kept == 7.0).all()) and bool((dev.parts[:nrows] == 0.0).all())
    launch(dev, mt.desc, rr, out[2])
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    assert torch.equal(out[0], transpose(dev, r, False, 0))


def test_every_number_of_group_slots_gives_the_same_bits():
    """Experiment build only (run the suite with ``PML_GLM_LIB`` naming it): k = 0, 2, 5 group slots of 5, and the
    static interleaves 5 : 0 and 3 : 2."""
    from photon_ml_amd.ops.native import configure, tl_experiment_build
    if not tl_experiment_build():
        pytest.skip("needs the experiment build of the GLM kernels")
    dev, _, r = shard("many")
    want = transpose(dev, r, False, 0)
    try:
        for sched, a, b in ((1, 0, 0), (1, 2, 0), (1, 5, 0), (0, 5, 0), (0, 3, 2), (0, 0, -1)):
            configure(tl_tg_sched=sched, tl_tg_a=a, tl_tg_b=b)
            assert torch.equal(transpose(dev, r, False, 1), want), (sched, a, b)
    finally:
        configure(tl_tg_sched=1, tl_tg_a=4, tl_tg_b=0)
