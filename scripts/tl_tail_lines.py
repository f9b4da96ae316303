"""Cache lines per tail gather of the tiled forward pass as a function of the unit height (CPU simulation, numpy).

Model (profiles/tl_window_rounds_ab.md): the texture-address time of a wide-round gather is the number of DISTINCT
cache lines of the coefficient vector that each quad of 4 neighbouring lanes touches; in the lane-interleaved layout
those are 4 consecutive entries of the unit's wide section sorted by (column, row). The script re-creates the bench
shard (``data/synthetic.generate_device_shard``: n - 1 fields with Zipf(s) ranks over (features - 1) // (n - 1)
columns each, an intercept, hottest-first relabel by expected frequency), classifies every 1024-row block's entries like
``ops/tiled.split_narrow`` (sorted by (column, row), cut into 256-entry rounds, a full round whose keys span < 64
is narrow) and merges the remaining (wide) entries of ``height // 1024`` consecutive blocks.

    python scripts/tl_tail_lines.py --rows 16384 --heights 1024,4096,16384 --line 64

prints one row per height: the narrow share and the distinct lines per wide entry, over all wide entries and over
those with keys >= --cold (the scattered part). 0.25 is the floor (4 entries of a quad on one line).

    python scripts/tl_tail_lines.py --transpose --rows 1048576 --groups 1,4

does the same for the transpose copy of one chunk (``ops/tiled.TLTChunk``: 1024-column tiles sorted by (row, column),
items of --item-entries, gathers of the fp32 per-row vector) with the wide entries of --groups consecutive single-item
tiles merged into the four sub-windows of a tile group, and prints the share of the wide entries that land in groups.
"""
import argparse

import numpy as np


def shard(rows, features, nnz, s, seed):
    fields = nnz - 1
    fs = (features - 1) // fields
    p = np.arange(1, fs + 1, dtype=np.float64) ** -s
    cdf = np.cumsum(p) / p.sum()
    rng = np.random.default_rng(seed)
    rank = np.minimum(np.searchsorted(cdf, rng.random((rows, fields))), fs - 1)
    # hottest-first relabel by EXPECTED frequency (what the counts of a 125M-row shard give; the counts of a few
    # thousand simulated rows would pack the once-seen cold columns into consecutive labels): the intercept, then
    # rank 0 of every field, rank 1 of every field, ...
    col = np.empty((rows, nnz), dtype=np.int64)
    col[:, :fields] = 1 + rank * fields + np.arange(fields)
    col[:, fields] = 0
    return col


def wide_entries(col, sub=1024, rnd=256, width=64):
    """Per 1024-row block: (column, row) of the entries that stay wide, and the total / narrow entry counts."""
    out, n_all, n_narrow = [], 0, 0
    for b0 in range(0, col.shape[0], sub):
        c = col[b0:b0 + sub]
        r = np.repeat(np.arange(b0, b0 + c.shape[0]), c.shape[1])
        c = c.reshape(-1)
        o = np.lexsort((r, c))
        c, r = c[o], r[o]
        full = c.size // rnd
        first, last = c[: full * rnd: rnd], c[rnd - 1: full * rnd: rnd]
        nar = np.repeat((last - first) < width, rnd)
        keep = np.ones(c.size, dtype=bool)
        keep[: full * rnd] = ~nar
        out.append((c[keep], r[keep]))
        n_all += c.size
        n_narrow += int(nar.sum())
    return out, n_all, n_narrow


def lines_per_entry(blocks, group, line_bytes, cold):
    """Distinct lines per wide entry with ``group`` consecutive blocks merged; (all entries, keys >= cold)."""
    per_line = line_bytes // 4                      # fp32 coefficients
    tot = np.zeros(2)
    cnt = np.zeros(2)
    for g in range(0, len(blocks), group):
        c = np.concatenate([b[0] for b in blocks[g:g + group]])
        r = np.concatenate([b[1] for b in blocks[g:g + group]])
        c = c[np.lexsort((r, c))]
        pad = (-c.size) % 4
        ln = np.r_[c // per_line, np.full(pad, -1)].reshape(-1, 4)
        key = np.r_[c, np.full(pad, -1)].reshape(-1, 4)
        live = ln >= 0
        distinct = (live & np.c_[np.ones(len(ln), dtype=bool), ln[:, 1:] != ln[:, :-1]]).sum(1)   # sorted -> runs
        tot[0] += distinct.sum()
        cnt[0] += c.size
        quad_cold = key[:, 0] >= cold                # a quad is sorted: cold iff its first key is
        tot[1] += distinct[quad_cold].sum()
        cnt[1] += live[quad_cold].sum()
    return tot / np.maximum(cnt, 1), cnt


def transpose_chunk(col, cbits=10, item_entries=1 << 18, rnd=256, width=64):
    """One row chunk's transpose copy as ``ops/tiled.TLTChunk`` builds it: per wide entry (in (tile, row, column)
    order) its tile, row, item and quarter (the wave of ``tl_t_item`` that walks its round: round r of an item
    with nr wide rounds belongs to wave (4 r + 3) // nr); plus items per tile and the total / narrow entry counts."""
    rows, nnz = col.shape
    r = np.repeat(np.arange(rows, dtype=np.int64), nnz)
    c = col.reshape(-1).astype(np.int64)
    key = np.sort(((c >> cbits) << 42) | (r << cbits) | (c & ((1 << cbits) - 1)))
    del r, c
    tile, row = key >> 42, (key >> cbits) & ((1 << (42 - cbits)) - 1)
    ntiles = int(tile[-1]) + 1
    tptr = np.searchsorted(tile, np.arange(ntiles + 1))
    cnt = np.diff(tptr)
    nz = np.flatnonzero(cnt)
    n_it = np.maximum(1, -(-cnt[nz] // item_entries))
    it_tile = np.repeat(nz, n_it)
    it_i = np.arange(len(it_tile)) - np.repeat(np.cumsum(n_it) - n_it, n_it)
    it_k = np.repeat(n_it, n_it)
    a, b = tptr[it_tile], tptr[it_tile + 1]
    lo, hi = a + (b - a) * it_i // it_k, a + (b - a) * (it_i + 1) // it_k
    gcount = (hi - lo) // rnd
    gi = np.repeat(np.arange(len(lo)), gcount)
    gs = lo[gi] + rnd * (np.arange(len(gi)) - np.repeat(np.cumsum(gcount) - gcount, gcount))
    base = np.minimum(row[gs], rows - width)
    nar = (row[gs + rnd - 1] - base) < width
    keep = np.ones(key.size, dtype=bool)
    keep[(gs[nar][:, None] + np.arange(rnd)[None, :]).reshape(-1)] = False
    item = np.repeat(np.arange(len(lo)), hi - lo)[keep]
    wn = np.bincount(item, minlength=len(lo))
    j = np.arange(item.size) - (np.cumsum(wn) - wn)[item]
    nr = -(-wn // rnd)
    quarter = (4 * (j // rnd) + 3) // np.maximum(nr[item], 1)
    items_of_tile = np.zeros(ntiles, dtype=np.int64)
    items_of_tile[nz] = n_it
    return tile[keep], row[keep], item, quarter, items_of_tile, key.size, int(nar.sum()) * rnd


def transpose_lines(tile, row, item, quarter, items_of_tile, group, line_bytes, cold_tile):
    """Distinct lines of the fp32 per-row vector per wide entry when the wide entries of ``group`` consecutive
    single-item tiles are merged into four sub-windows sorted by (quarter, row, column) and lane-interleaved (quads
    of 4 consecutive sorted entries, each sub-window padded to whole rounds); multi-item tiles and tiles of a group
    that holds one keep their own items. Returns (lines / entry: all, tiles >= cold_tile), the share of wide entries
    in merged groups and the pad entries per wide entry."""
    per_line = line_bytes // 4
    ntiles = len(items_of_tile)
    g_of_tile = np.arange(ntiles) // group
    bad = np.bincount(g_of_tile, weights=(items_of_tile > 1), minlength=g_of_tile[-1] + 1) > 0
    if group == 1:
        bad[:] = True
    merged = ~bad[g_of_tile[tile]]
    # window id: a merged entry's (group, quarter), any other entry's item (kept apart by an offset)
    win = np.where(merged, g_of_tile[tile] * 4 + quarter, 4 * (g_of_tile[-1] + 1) + item)
    order = np.lexsort((tile, row, win))            # (window, row, column in group); items are already in order
    win, ln, tl = win[order], (row // per_line)[order], tile[order]
    first = np.r_[True, win[1:] != win[:-1]]
    start = np.flatnonzero(first)
    pos = np.arange(win.size) - np.repeat(start, np.diff(np.r_[start, win.size]))
    new_quad = first | (pos % 4 == 0)
    distinct = new_quad | np.r_[True, ln[1:] != ln[:-1]]
    wcount = np.diff(np.r_[start, win.size])
    pad = int(((-wcount) % 256).sum())
    coldm = tl >= cold_tile
    return (distinct.sum() / max(win.size, 1), distinct[coldm].sum() / max(coldm.sum(), 1),
            merged.mean() if merged.size else 0.0, coldm.mean() if coldm.size else 0.0, pad / max(win.size, 1))


def main_transpose(a):
    col = shard(a.rows, a.features, a.nnz, a.zipf, a.seed)
    tile, row, item, quarter, iot, n_all, n_narrow = transpose_chunk(col, item_entries=a.item_entries)
    del col
    print(f"transpose copy of one chunk: {a.rows} rows x {a.nnz} nnz, {a.features} features, Zipf({a.zipf}), "
          f"1024-column tiles, items of {a.item_entries} entries; narrow share {n_narrow / n_all:.1%}; "
          f"{int((iot > 1).sum())} of {int((iot > 0).sum())} non-empty tiles have several items; {a.line}-byte lines")
    print(f"| tiles per group | lines / wide entry | same, tiles of columns >= {a.cold} | share of wide entries "
          f"there | share of wide entries in groups | pad entries / wide entry |")
    print("|---:|---:|---:|---:|---:|---:|")
    for g in (int(x) for x in a.groups.split(",")):
        all_, cold_, share, cshare, pad = transpose_lines(tile, row, item, quarter, iot, g, a.line, a.cold // 1024)
        print(f"| {g} | {all_:.3f} | {cold_:.3f} | {cshare:.1%} | {share:.1%} | {pad:.4f} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--transpose", action="store_true",
                    help="the transpose copy instead: lines of the per-row vector per wide entry with the wide entries "
                         "of --groups consecutive single-item column tiles merged (ops/tiled.py, TILE GROUPS)")
    ap.add_argument("--groups", default="1,2,4,8", help="--transpose: tiles per group")
    ap.add_argument("--item-entries", type=int, default=1 << 18, help="--transpose: entries per work item")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--heights", default="1024,4096,16384", help="unit heights in rows (multiples of 1024)")
    ap.add_argument("--line", type=int, default=64, help="cache line size in bytes")
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=100)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--cold", type=int, default=128 * 1024, help="keys at or above this count as the cold tail")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.transpose:
        return main_transpose(a)
    col = shard(a.rows, a.features, a.nnz, a.zipf, a.seed)
    blocks, n_all, n_narrow = wide_entries(col)
    print(f"{a.rows} rows x {a.nnz} nnz, {a.features} features, Zipf({a.zipf}); narrow share {n_narrow / n_all:.1%}; "
          f"{a.line}-byte lines")
    print(f"| unit height | lines / wide entry | lines / wide entry, keys >= {a.cold} | share of wide entries there |")
    print("|---:|---:|---:|---:|")
    for h in (int(x) for x in a.heights.split(",")):
        if h % 1024:
            raise SystemExit("heights must be multiples of 1024")
        (all_, cold_), cnt = lines_per_entry(blocks, h // 1024, a.line, a.cold)
        print(f"| {h} | {all_:.3f} | {cold_:.3f} | {cnt[1] / max(cnt[0], 1):.1%} |")


if __name__ == "__main__":
    main()
