"""The shapes of the random-effect boundary tests (not a test file): per case the ``make_ragged_entities`` spec, the
seed and what the case promises about its data. ``test_re_boundary_shapes.py`` checks the promises on the CPU,
``test_re_boundary_gpu.py`` runs the cases through the fused solvers."""
import functools

from re_parity_util import make_ragged_entities

# Row-length cycles. RAGGED walks every edge of the row passes: no entry, 1, a quad and its neighbours, the 16-lane
# row group and its neighbours, the 64 entries row_pass keeps in registers (RE_K x RE_G) and its neighbours, a
# second round of quads past 64, and 130 (two more rounds).
RAGGED = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 67, 68, 69, 130)
# ... with the short lengths removed, so that the mean reaches QUAD_MIN_ROW_NNZ and the rows are padded to quads
QUADDY = (13, 15, 16, 17, 60, 61, 63, 64, 65, 67, 68, 130)
# ... thinned with short rows (three after every RAGGED length), so that the mean stays below QUAD_MIN_ROW_NNZ
_SHORT = (0, 1, 3, 4, 5)
SCALAR = tuple(v for i, ln in enumerate(RAGGED) for v in (ln, _SHORT[(3 * i) % 5], _SHORT[(3 * i + 1) % 5],
                                                          _SHORT[(3 * i + 2) % 5]))
RAGGED64 = tuple(ln for ln in RAGGED if ln <= 64)          # the resident kernel's rows: at most RES_ROW_NNZ entries
CSR_ROWS = RAGGED + (300,)                                 # RAGGED plus a long row, to cover more than 1024 columns
SMALL_CSR_ROWS = (0, 1, 3, 4, 5, 15, 16, 17, 63)           # covers 2048 columns in 160 rows with few entries

LEAN_WIDTHS = (65, 255, 256, 257, 511, 512, 513, 1023, 1024)
_LEAN_ROWS = {65: 65, 255: 100, 256: 130, 257: 75, 511: 150, 512: 200, 513: 130, 1023: 260, 1024: 180,
              70: 90, 1009: 260}


def _lean(widths, cycle):
    return [(_LEAN_ROWS[d], d, cycle) for d in widths]


def _cover(lens, d):
    """``lens`` (clipped to ``d``), every row lengthened by the same amount where they would not cover ``d``."""
    lens = [min(ln, d) for ln in lens]
    short = d - sum(lens)
    if short > 0:
        add = -(-short // len(lens))
        lens = [min(ln + add, d) for ln in lens]
    return tuple(lens)


# row space, small classes: n_e rows over d_e in {n_e, n_e + 1, 200} columns, every row of at least 1 entry (after
# the first round of the cycle no row of 1 entry: two such rows on one column would make K_e singular)
RS_SMALL_ROWS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24)
_RS_FIRST, _RS_LATER = (1, 3, 4, 5, 15, 16, 17), (2, 3, 4, 5, 15, 16, 17)


def _rs_lens(n, d):
    return _cover([(_RS_FIRST if i < 7 else _RS_LATER)[i % 7] for i in range(n)], d)


def _rs_small():
    spec = []
    for k, n in enumerate(RS_SMALL_ROWS):
        d = (n, n + 1, 200)[k % 3]
        spec.append((n, d, _rs_lens(n, d)))
    return spec


# row space, failed factor: one size class (13 .. 16 rows); healthy entities, entities with a duplicated row and
# entities with a row without entries (a zero pivot)
RS_FAIL = dict(
    spec=[(14, 40, _rs_lens(14, 40)), (16, 40, _rs_lens(16, 40)), (13, 40, _rs_lens(13, 40)),       # duplicated row
          (15, 40, _rs_lens(15, 40)), (16, 200, _rs_lens(16, 200)), (13, 16, _rs_lens(13, 16)),     # healthy
          (15, 40, (3, 4, 0, 5, 15, 16, 17)), (16, 200, (40, 30, 20, 0, 50, 20, 30, 10)),           # empty row
          (16, 16, _rs_lens(16, 16))],                                                              # healthy, square
    dup={0: ((9, 2),), 1: ((1, 0), (15, 7)), 2: ((12, 0),)},
    singular=(0, 1, 2, 6, 7), healthy=(3, 4, 5, 8))

# mixed coordinate (production routing): small row-space entities, a failed factor (row without entries), tall
# entities, lean entities, a CSR entity and a pass-path entity. The register-resident policy ``auto`` sends an
# entity to the pass path ("heavy") or to the resident kernel when it holds more than 1 / RES_TAIL_SHARE of the
# streaming entities' entries: the 1009-wide entity (3000 rows of 200 entries, too long a row for the resident
# kernel) carries enough entries that no other entity is such a tail.
MIXED = dict(
    spec=[(3, 5, _rs_lens(3, 5)), (11, 200, _rs_lens(11, 200)), (20, 40, _rs_lens(20, 40)),         # row space
          (12, 30, (3, 4, 0, 5, 15, 16, 17)),                              # failed factor, in the class of the 11 rows
          (100, 16, RAGGED), (70, 64, RAGGED),                                                      # tall
          (140, 257, RAGGED), (3000, 1009, (200,)),                                                 # lean
          (160, 2048, SMALL_CSR_ROWS),                                                              # csr
          (140, 2049, CSR_ROWS)],                                                                   # pass path
    row_space=(0, 1, 2), fused=(3, 4, 5, 6, 7, 8), pass_path=(9,))

TALL_SPEC = [(17, 1, RAGGED), (1, 15, (15,)), (15, 16, RAGGED), (16, 17, RAGGED), (33, 32, RAGGED),
             (31, 33, RAGGED), (100, 48, RAGGED), (17, 49, RAGGED), (15, 64, RAGGED), (100, 64, RAGGED),
             (1, 16, (16,)), (16, 32, RAGGED), (33, 17, RAGGED),
             (70, 65, RAGGED)]                                     # the last one is too wide: a lean launch
CSR_SPEC = [(130, 1025, CSR_ROWS), (200, 2047, CSR_ROWS), (260, 2048, CSR_ROWS),
            (150, 2049, CSR_ROWS)]                                 # the last one is too wide: the pass path


def resident_spec(cap, rdmax):
    """Entities around the workgroup capacity ``cap`` (one workgroup, clusters of 2 and 3) up to the widest LDS
    image ``rdmax``; the last entity has one row of 65 entries, which the resident selection refuses."""
    return [(cap - 1, 65, RAGGED64), (cap, 512, RAGGED64), (cap + 1, rdmax, RAGGED64), (2 * cap, 65, RAGGED64),
            (2 * cap + 1, 512, RAGGED64), (2 * cap + 1, rdmax, RAGGED64),
            (90, 300, (65,) + RAGGED64)]


# name: (spec, seed, duplicate rows)
CASES = {
    "lean_scalar": (_lean(LEAN_WIDTHS, SCALAR), 1, None),
    "lean_quad": (_lean(LEAN_WIDTHS, QUADDY), 2, None),
    "narrow_scalar_a": (_lean((70, 257, 513), SCALAR), 3, None),
    "narrow_scalar_b": (_lean((1009,), SCALAR), 4, None),
    "narrow_quad_a": (_lean((70, 257, 513), QUADDY), 5, None),
    "narrow_quad_b": (_lean((1009,), QUADDY), 6, None),
    "tall": (TALL_SPEC, 6, None),
    "csr": (CSR_SPEC, 8, None),
    "rs_small": (_rs_small(), 125, None),
    "rs_fail": (RS_FAIL["spec"], 10, RS_FAIL["dup"]),
    "mixed": (MIXED["spec"], 55, None),
}


def case_spec(name, cap=None, rdmax=None):
    if name == "resident":
        return resident_spec(cap, rdmax), 12, None
    return CASES[name]


@functools.lru_cache(maxsize=None)
def case_data(name, loss="LOGISTIC", cap=None, rdmax=None):
    """The case's data (shared by the tests, never modified)."""
    spec, seed, dup = case_spec(name, cap, rdmax)
    return make_ragged_entities(spec, seed, loss=loss, duplicate_rows=dup)
