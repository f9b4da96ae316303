"""The shapes of the persistent random-effect kernel tests (not a test file): per case the ``make_ragged_entities``
spec, the seed and what the case promises about its data. ``test_re_persistent_shapes.py`` checks the promises and
the seeds on the CPU, ``test_re_persistent_gpu.py`` runs the cases through ``re_lbfgs_csr_kernel`` and
``re_tron_res_kernel`` with workgroups that serve more than one entity."""
import functools

from re_boundary_cases import CSR_ROWS, QUADDY, RAGGED, RAGGED64, SCALAR, resident_spec
from re_parity_util import make_ragged_entities

LBFGS_CLASSES = (256, 512, 1024, 2048)

# owl_edges: both ends of every LDS class of the fused OWL-QN, entities of 1 and 2 coefficients, and one entity too
# wide for the kernel (the pass path)
OWL_EDGES = [(40, 1, RAGGED), (30, 2, RAGGED), (100, 255, QUADDY), (130, 256, SCALAR), (75, 257, QUADDY),
             (150, 511, SCALAR), (200, 512, QUADDY), (130, 513, SCALAR), (260, 1023, QUADDY), (180, 1024, QUADDY),
             (130, 1025, CSR_ROWS), (200, 2047, CSR_ROWS), (260, 2048, CSR_ROWS), (150, 2049, CSR_ROWS)]
OWL_EDGES_LAUNCHES = {256: [0, 1, 2, 3], 512: [4, 5, 6], 1024: [7, 8, 9], 2048: [10, 11, 12]}
OWL_EDGES_PASS_PATH = [13]

# owl_ring: the entities of owl_edges of 255 .. 2048 coefficients (every one in a fused launch; the narrow two part
# ways by rounding beyond 5 iterations)
OWL_RING = [s for s in OWL_EDGES if 255 <= s[1] <= 2048]
OWL_RING_LAUNCHES = {256: [0, 1], 512: [2, 3, 4], 1024: [5, 6, 7], 2048: [8, 9, 10]}

# owl_reuse: 8 entities in each of the classes 512 and 1024; a launch takes them by descending non-zeros, along
# which the widths go up and down
OWL_REUSE = [(220, 300, QUADDY), (60, 512, QUADDY), (150, 257, RAGGED), (100, 511, QUADDY), (180, 330, SCALAR),
             (75, 460, QUADDY), (130, 400, RAGGED), (50, 290, QUADDY),
             (260, 700, QUADDY), (80, 1024, QUADDY), (200, 513, RAGGED), (120, 1023, QUADDY), (240, 600, SCALAR),
             (100, 900, QUADDY), (160, 800, RAGGED), (70, 560, QUADDY)]
OWL_REUSE_LAUNCHES = {512: list(range(8)), 1024: list(range(8, 16))}

_OVER_ROWS = (300, 280, 310, 290)


def owl_over_spec(grid):
    """``grid + 40`` entities of 1025 .. 2048 coefficients in few long rows: more entities than the class-2048
    launch has resident workgroups."""
    spec = []
    for k in range(grid + 40):
        d = 1025 + (37 * k) % 1024
        spec.append((max(4 + k % 4, -(-d // 280)), d, _OVER_ROWS))
    return spec


# res_singles: 20 entities of one resident workgroup each, widths and row counts in no order
RES_SINGLE_WIDTHS = (65, 1024, 130, 700, 66, 512, 300, 1000, 90, 257, 1023, 70, 513, 80, 640, 100, 256, 900, 72, 400)
RES_SINGLE_ROWS = (40, 120, 30, 100, 25, 90, 60, 110, 20, 70, 130, 35, 95, 45, 85, 50, 65, 115, 33, 75)
RES_SINGLES = [(n, d, RAGGED64) for n, d in zip(RES_SINGLE_ROWS, RES_SINGLE_WIDTHS)]
RES_CLUSTER_SINGLES = RES_SINGLES[:8]


def res_clusters_spec(cap, rdmax):
    """The cluster tasks of ``re_boundary_cases.resident_spec`` (1, 1, 2, 2, 3, 3 workgroups; the entity that the
    resident selection refuses left out) plus 8 single-workgroup entities."""
    return resident_spec(cap, rdmax)[:6] + RES_CLUSTER_SINGLES


def res_over_spec(grid):
    """``grid + 40`` single-workgroup entities: more tickets than the resident launch has workgroups."""
    spec = []
    for k in range(grid + 40):
        d = 65 + (53 * k) % 960
        spec.append((max(12 + k % 9, 12 * -(-d // 189)), d, RAGGED64))
    return spec


# name: (spec, seed). Seeds are chosen by the oracle alone (test_re_persistent_shapes.py re-checks the criteria).
CASES = {
    "owl_edges": (OWL_EDGES, 2),
    "owl_ring": (OWL_RING, 1),
    "owl_reuse": (OWL_REUSE, 1),
    "res_singles": (RES_SINGLES, 1),
}
SEEDS = {"owl_over": 5, "res_clusters": 2, "res_over": 6}
# the grids of an MI355X (256 CUs, one workgroup per CU for either kernel): the CPU tier checks the oversubscribed
# cases at these sizes; on the device the sizes follow the run-time grids
NOMINAL_GRID = 256


def case_spec(name, cap=None, rdmax=None, grid=None):
    if name == "owl_over":
        return owl_over_spec(grid), SEEDS[name]
    if name == "res_over":
        return res_over_spec(grid), SEEDS[name]
    if name == "res_clusters":
        return res_clusters_spec(cap, rdmax), SEEDS[name]
    return CASES[name]


@functools.lru_cache(maxsize=None)
def case_data(name, loss="LOGISTIC", cap=None, rdmax=None, grid=None):
    """The case's data (shared by the tests, never modified). HINGE takes the 0 / 1 labels of LOGISTIC."""
    spec, seed = case_spec(name, cap, rdmax, grid)
    return make_ragged_entities(spec, seed, loss="LOGISTIC" if loss == "HINGE" else loss)
