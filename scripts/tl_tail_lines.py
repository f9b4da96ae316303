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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--heights", default="1024,4096,16384", help="unit heights in rows (multiples of 1024)")
    ap.add_argument("--line", type=int, default=64, help="cache line size in bytes")
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=100)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--cold", type=int, default=128 * 1024, help="keys at or above this count as the cold tail")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
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
