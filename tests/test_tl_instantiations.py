"""The production GLM library holds exactly the tiled-kernel instantiations its launch ladder can reach
(``tl_with_acc`` / ``tl_with_pipe`` in ``ops/csrc/glm_kernels.hip``): the A/B variants behind the experiment
build's knobs must not be compiled into it. The host half of a HIP shared object keeps the mangled name of every
registered kernel as a plain string, so the names are read from the file's bytes; nothing is loaded or run."""
import re

from photon_ml_amd.ops import build as B

_TYPES = {"t": "bf16", "f": "f32", "d": "f64"}         # Itanium codes: unsigned short (bf16 bits), float, double
# tl_fwd[_multi]_kernel<VT, XT, RT, AT, MAXR, U, NW, P>;  tl_t[_multi]_kernel<VT, XT, AT, SQ, MAXR, U, NW, P>
_NAME = re.compile(rb"_Z\d+tl_(fwd|t)(_multi)?_kernelI([tfd])([fd])([fd])([fd])?(?:Lb([01])E)?"
                   rb"Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE")


def _decode(m):
    kind, multi, vt, xt, c, d, sq, maxr, u, nw, p = (g.decode() if g is not None else None for g in m.groups())
    if kind == "fwd":
        assert d is not None and sq is None and c == xt, m.group(0)     # the residual type is the vector type
        acc = d
    else:
        assert d is None and sq is not None, m.group(0)
        acc = c
    return (kind + (multi or ""), _TYPES[vt], _TYPES[xt], _TYPES[acc], None if sq is None else int(sq), int(maxr),
            int(u), int(nw), int(p))


def _expected():
    f32_acc = [("f64", 1024), ("f64", 2048), ("f32", 4096)]      # widths <= 10, 11, 12
    rows = [("bf16", "f32", f32_acc), ("f32", "f32", f32_acc), ("f64", "f64", [("f64", 1024), ("f64", 2048)])]
    want = set()
    for kernel, nw, sqs in (("fwd", 2, [None]), ("fwd_multi", 2, [None]), ("t", 4, [0, 1]), ("t_multi", 4, [0, 1])):
        for vt, xt, accs in rows:
            for acc, maxr in accs:
                for sq in sqs:
                    for p in (0, 3):                                    # plain / interleaved production pipelines
                        want.add((kernel, vt, xt, acc, sq, maxr, 2, nw, p))
    return want


def test_production_library_holds_only_reachable_tiled_kernels():
    data = B.verified_path("hip", "glm").read_bytes()
    names = {m.group(0): m for m in _NAME.finditer(data)}
    # every tiled-kernel name in the file must be one the pattern above decodes in full
    loose = set(re.findall(rb"_Z\d+tl_(?:fwd|t)(?:_multi)?_kernelI\w+?EE", data))
    assert loose == set(names), sorted(loose ^ set(names))[:5]
    got = {_decode(m) for m in names.values()}
    want = _expected()
    assert len(want) == 96
    per_kernel = {k: sum(1 for r in want if r[0] == k) for k in ("fwd", "fwd_multi", "t", "t_multi")}
    assert per_kernel == {"fwd": 16, "fwd_multi": 16, "t": 32, "t_multi": 32}
    assert len(names) == len(got), "two names decode to the same row"
    assert got == want, (f"{len(got)} tiled instantiations found, {len(want)} expected; "
                         f"unexpected {sorted(got - want, key=str)[:8]}, missing {sorted(want - got, key=str)[:8]}")
