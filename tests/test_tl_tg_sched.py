"""The static interleave of the grouped shard-wide transpose (``tl_tg_interleave``, ops/csrc/glm_kernels.hip), mirrored
here as the kernel computes it: block i of ``ngroups + nitems`` runs unit u(i); u < ngroups is a group, any other an
item. For every pair of counts and every ratio the map is a bijection onto all units, full windows of a + b blocks
hold a groups and b items in table order while such windows of both kinds remain, and the rest is the groups left,
then the items left."""
import pytest

COUNTS = (0, 1, 7, 1000)
RATIOS = ((5, 0), (4, 1), (3, 2), (2, 3), (0, 5), (1, 1), (7, 1))


def interleave(i, ng, ni, a, b):
    if b <= 0 or a < 0:
        return i
    if a == 0:
        return ng + i if i < ni else i - ni
    w, nw = a + b, min(ng // a, ni // b)
    if i < nw * w:
        win, p = divmod(i, w)
        return win * a + p if p < a else ng + win * b + (p - a)
    j, rg = i - nw * w, ng - nw * a
    return nw * a + j if j < rg else ng + nw * b + (j - rg)


def proportional(ng, ni):
    """The host's a : b on windows of 8 for the proportion ngroups : nitems."""
    a = min(max((8 * ng + (ng + ni) // 2) // (ng + ni), 1), 7)
    return a, (8 - a if ni > 0 else 0)


@pytest.mark.parametrize("ni", COUNTS)
@pytest.mark.parametrize("ng", COUNTS)
def test_bijection_and_window_counts(ng, ni):
    ratios = RATIOS + ((proportional(ng, ni),) if ng + ni else ())
    for a, b in ratios:
        units = [interleave(i, ng, ni, a, b) for i in range(ng + ni)]
        assert sorted(units) == list(range(ng + ni)), (a, b)
        groups = [u for u in units if u < ng]
        items = [u for u in units if u >= ng]
        assert groups == sorted(groups) and items == sorted(items)          # table order inside each kind
        if a > 0 and b > 0:
            nw = min(ng // a, ni // b)
            for w in range(nw):
                win = units[w * (a + b):(w + 1) * (a + b)]
                assert all(u < ng for u in win[:a]) and all(u >= ng for u in win[a:]), (a, b, w)
            rest = units[nw * (a + b):]
            assert rest == sorted(rest)                                       # the groups left, then the items left
            assert ng - nw * a < a or ni - nw * b < b                         # no full window of both kinds is left
        elif b == 0:
            assert units == list(range(ng + ni))                             # the groups, then the items
        else:
            assert units == list(range(ng, ng + ni)) + list(range(ng))       # the items, then the groups


def test_proportional_ratio_tracks_the_counts():
    assert proportional(1000, 1000) == (4, 4) and proportional(1000, 7) == (7, 1) and proportional(7, 1000) == (1, 7)
    assert proportional(7, 0) == (7, 0) and proportional(3, 1) == (6, 2)
