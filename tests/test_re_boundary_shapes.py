"""The data of the random-effect boundary cases (``re_boundary_cases.py``, ``re_parity_util.make_ragged_entities``)
is what the cases say it is: exact projected widths, the promised row lengths (rows without any entry among them),
rows at exactly 0 weight, duplicated rows. No GPU: ``test_re_boundary_gpu.py`` runs the same data through the
solvers, and its routing assertions rest on these properties."""
import numpy as np
import pytest

from re_boundary_cases import (CASES, MIXED, QUADDY, RAGGED, RAGGED64, RS_FAIL, RS_SMALL_ROWS, SCALAR, case_data,
                               case_spec)
from re_parity_util import make_ragged_entities

QUAD_MIN_ROW_NNZ = 12


def _res_params():
    from photon_ml_amd.ops.native import require_re_lib
    lib = require_re_lib()
    return int(lib.pml_re_res_cap()), int(lib.pml_re_res_dmax())


def _case(name):
    cap, rdmax = _res_params() if name == "resident" else (None, None)
    return case_spec(name, cap, rdmax), case_data(name, "LOGISTIC", cap, rdmax)


def _entities(data):
    x, ids = data.shards["user"].tocsr(), data.id_tags["userId"]
    lens = np.diff(x.indptr)
    for e in np.unique(ids):
        r = np.nonzero(ids == e)[0]
        yield int(e), r, lens[r], x[r]


@pytest.mark.parametrize("name", list(CASES) + ["resident"])
def test_generator_claims(name):
    (spec, seed, dup), data = _case(name)
    x = data.shards["user"].tocsr()
    assert x.has_canonical_format and (x.data != 0).all()
    assert len(np.unique(data.id_tags["userId"])) == len(spec)
    base = 0
    for (e, r, lens, xe), (n, d, lengths) in zip(_entities(data), spec):
        want = [min(lengths[i % len(lengths)], d) for i in range(n)]
        for i, j in (dup or {}).get(e, ()):              # a duplicated row has the length of the row it copies
            want[i] = want[j]
        assert len(r) == n and list(lens) == want, (name, e)
        # the entity's columns are exactly its own block of d_e global columns: the projected width is d_e
        assert np.array_equal(np.unique(xe.indices), np.arange(base, base + d)), (name, e)
        base += d
    # weights of make_entities: multiples of 1/4 in [0.25, 4] and rows at exactly 0; offsets 0.3 sin(i)
    w = data.weights
    assert (w == 0).any() and 0.05 < (w == 0).mean() < 0.3 and set(np.unique(w * 4)) <= set(range(17))
    assert np.array_equal(data.offsets, 0.3 * np.sin(np.arange(data.n_rows)))
    # the same seed gives the same data; another seed another
    again = make_ragged_entities(spec, seed, duplicate_rows=dup)
    assert (again.shards["user"] != x).nnz == 0 and np.array_equal(again.response, data.response)
    assert (make_ragged_entities(spec, seed + 1, duplicate_rows=dup).shards["user"] != x).nnz != 0


def _lengths(data, entities=None):
    return {int(v) for e, _, lens, _ in _entities(data) if entities is None or e in entities for v in lens}


@pytest.mark.parametrize("name", ["lean_scalar", "narrow_scalar_a", "narrow_scalar_b"])
def test_scalar_rows_stay_below_the_quad_threshold(name):
    _, data = _case(name)
    x = data.shards["user"]
    assert x.nnz < QUAD_MIN_ROW_NNZ * data.n_rows
    widest = max(d for _, d, _ in CASES[name][0])
    assert _lengths(data) >= {min(v, widest) for v in RAGGED} and 0 in _lengths(data)
    assert set(SCALAR) == set(RAGGED)


@pytest.mark.parametrize("name", ["lean_quad", "narrow_quad_a", "narrow_quad_b"])
def test_quad_rows_reach_the_quad_threshold(name):
    _, data = _case(name)
    assert data.shards["user"].nnz >= QUAD_MIN_ROW_NNZ * data.n_rows
    # lengths that are no multiple of 4 (the padded quad path), just past 64 and two more rounds
    assert _lengths(data) >= set(min(v, 65) for v in QUADDY)
    for e, _, lens, _ in _entities(data):
        d = CASES[name][0][e][1]
        if d >= 130:
            assert set(lens) == set(QUADDY), (name, e)


def test_tall_rows():
    (spec, _, _), data = _case("tall")
    assert {d for _, d, _ in spec[:-1]} == {1, 15, 16, 17, 32, 33, 48, 49, 64} and spec[-1][1] == 65
    assert {n for n, _, _ in spec[:-1]} == {1, 15, 16, 17, 31, 33, 100}
    full = empty = 0
    for e, r, lens, _ in _entities(data):
        d = spec[e][1]
        full += int((lens == d).sum())
        empty += int((lens == 0).sum())
        if len(r) > 14:
            assert set(lens) == {min(v, d) for v in RAGGED[:len(r)]}, e
    assert full and empty


def test_csr_rows():
    (spec, _, _), data = _case("csr")
    assert [d for _, d, _ in spec] == [1025, 2047, 2048, 2049]
    for e, _, lens, _ in _entities(data):
        assert set(lens) == set(RAGGED) | {300}, e


def test_resident_rows():
    cap, rdmax = _res_params()
    (spec, _, _), data = _case("resident")
    assert {n for n, _, _ in spec[:-1]} == {cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1}
    assert {d for _, d, _ in spec[:-1]} == {65, 512, rdmax}
    for e, _, lens, _ in _entities(data):
        if e < len(spec) - 1:
            assert set(lens) == set(RAGGED64) and lens.max() == 64, e
        else:
            assert (lens == 65).sum() >= 1 and lens.max() == 65      # refused by the resident selection


def test_row_space_small_rows():
    (spec, _, _), data = _case("rs_small")
    assert {n for n, _, _ in spec} == set(RS_SMALL_ROWS)
    kinds = set()
    for (e, r, lens, xe), (n, d, _) in zip(_entities(data), spec):
        assert d >= n and lens.min() >= 1, e
        kinds.add("n" if d == n else "n+1" if d == n + 1 else d)
        # K_e = X_e X_e^T is positive definite: the entity stays in the row-space batch
        assert np.linalg.matrix_rank(xe.toarray()) == n, e
    assert kinds == {"n", "n+1", 200}


def _check_failed_factor(data, spec, dup, singular, healthy):
    ents = {e: (r, lens, xe) for e, r, lens, xe in _entities(data)}
    assert set(singular) | set(healthy) <= set(ents) and not set(singular) & set(healthy)
    for e in healthy:
        r, lens, xe = ents[e]
        assert lens.min() >= 1 and np.linalg.matrix_rank(xe.toarray()) == len(r), e
    for e in singular:
        r, lens, xe = ents[e]
        a = xe.toarray()
        assert np.linalg.matrix_rank(a) < len(r), e
        if e in (dup or {}):
            for i, j in dup[e]:
                assert j < i and np.array_equal(a[i], a[j]) and a[i].any(), (e, i, j)
        else:
            assert (lens == 0).any(), e                  # a row without entries: a zero pivot


def test_failed_factor_rows():
    (spec, _, dup), data = _case("rs_fail")
    assert len({-(-n // 4) for n, _, _ in spec}) == 1 and all(12 < n <= 16 <= d for n, d, _ in spec)   # one size class
    _check_failed_factor(data, spec, dup, RS_FAIL["singular"], RS_FAIL["healthy"])
    assert sum(e in dup for e in RS_FAIL["singular"]) == 3 and len(RS_FAIL["singular"]) == 5


def test_mixed_rows():
    (spec, _, _), data = _case("mixed")
    assert sorted(MIXED["row_space"] + MIXED["fused"] + MIXED["pass_path"]) == list(range(len(spec)))
    _check_failed_factor(data, spec, None, (3,), MIXED["row_space"])
    assert spec[1][0] <= 12 and spec[3][0] <= 12 and min(spec[1][0], spec[3][0]) > 8      # one size class (9 .. 12)
    assert [spec[e][1] for e in MIXED["fused"][1:]] == [16, 64, 257, 1009, 2048] and spec[9][1] == 2049
    # every entity outside the row space has more rows than the row space takes, or more rows than coefficients
    assert all(spec[e][0] > min(128, spec[e][1]) for e in MIXED["fused"][1:] + MIXED["pass_path"])
    # the policy ``auto`` of the resident kernel: an entity with more than 1 / 256 of the streaming entities' entries
    # goes to a cluster when its rows hold at most 64 entries, and to the pass path when it is wider than 1024. The
    # 2048-wide entity stays below that share (the 1009-wide one carries the entries); the lean entities have
    # rows of more than 64 entries.
    nnz = {e: int(lens.sum()) for e, _, lens, _ in _entities(data)}
    stream = sum(nnz[e] for e in MIXED["fused"] if spec[e][1] > 64)
    assert 256 * nnz[8] <= stream
    assert all(max(lens.max() for e, _, lens, _ in _entities(data) if e == k) > 64 for k in (6, 7))
    for loss in ("POISSON", "SQUARED"):
        other = case_data("mixed", loss)
        assert (other.shards["user"] != data.shards["user"]).nnz == 0
        assert not np.array_equal(other.response, data.response)


def test_entity_without_any_entry():
    """``d_e = 0``: every row empty; the shard keeps its other columns."""
    data = make_ragged_entities([(4, 6, (3,)), (5, 0, (0,)), (3, 2, (1, 2))], 1)
    x = data.shards["user"].tocsr()
    assert x.shape == (12, 8) and np.array_equal(np.diff(x.indptr)[4:9], np.zeros(5))
    assert np.array_equal(np.unique(x[9:].indices), [6, 7])


def test_rows_too_short_to_cover_the_width():
    with pytest.raises(ValueError):
        make_ragged_entities([(3, 10, (1, 2))], 1)
