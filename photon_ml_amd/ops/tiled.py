"""Tiled ("TL") sparse layout for the gather-coalesced HIP kernels (``glm_kernels.hip``, section TILED LAYOUT).

One row chunk of a feature shard is stored twice:

* forward copy — ROW BLOCKS of ``2^rbits`` consecutive rows; inside a block the entries are sorted by
  (column, row) and packed into one uint32 ``(col << rbits) | local_row``. Block table: ``{row_lo, nrows, e_lo,
  e_hi}``. ``rbits = min(10, 32 - bits(D))``.
* transpose copy — COLUMN TILES of ``2^cbits`` columns; inside a tile entries are sorted by (row, column) and
  packed as ``(local_row << cbits) | (col & (2^cbits - 1))``; a tile is cut into work items of at most
  ``item_entries`` entries. Item table: ``{tile, e_lo, e_hi, part}`` with ``part = -1`` for single-item tiles
  and a partial-row index otherwise; split tiles are combined in item order by a two-level fixed-order
  reduction (units of ``COMBINE_SEG`` partial rows, then the units of a tile) — deterministic.
  ``cbits = min(10, 32 - bits(chunk_rows))``.

NARROW SECTION (``PML_TL_NARROW``, default on with the interleaved layout): a unit's sorted entries are cut into
groups of 256 (one kernel round); a full group whose gather keys span fewer than 64 values (hot columns in the
forward copy, dense rows in the transpose copy: about half of the entries at the bench shape) is moved to the
unit's narrow section and stored with a 16-bit pack ``((key - base) << bits) | slot`` and one int32 ``base`` per
round (``base + 63 < len(x)``). The kernel reads such a round's key window with one coalesced load and picks the
values with cross-lane permutes (``tl_stream_narrow``): 4 B/entry of stream instead of 6 (bf16) and a third of the
gather instructions. Unit tables gain ``{n_lo, n_hi}`` (the unit's narrow rounds); a unit's narrow rounds are
processed before its remaining (wide) entries, both in sorted order.

FUSED NARROW RECORDS (``PML_TL_FUSE``, default on; bf16 values only): the narrow section is ONE stream of 16-byte
lane records instead of a pack array and a value array — lane L of narrow round r reads the record at byte
``(r * 64 + L) * 16``, eight 16-bit words ``{p0, p1, p2, p3, v0, v1, v2, v3}``: its four packs, then the bit
patterns of its four bf16 values, in the interleaved order (logical entries L, L+64, L+128, L+192 of the round).
Same entries in the same order; a narrow round then costs one 16-byte stream load per lane instead of two 8-byte
ones. ``npack`` / ``nval`` of such a chunk are strided views into the record stream ``nrec`` and the kernels get a
null narrow-value pointer. fp32 / fp64 chunks (16-byte value quads already) keep the two arrays.

TALL FORWARD UNITS (``PML_TL_TALL=0/1``; by default bf16 / fp32 shards in the interleaved + narrow layout with
``dim >= 2^16`` and chunks of at least 4096 rows; fp64 shards keep the row blocks above): a forward chunk is cut
into units of ``2^tbits = 4096`` rows, each 4 SUB-BLOCKS of ``2^rbits = 1024`` rows (the last unit and its last
sub-block may be ragged). The narrow section is built per sub-block exactly as above (same split rule, 16-bit packs
``((key - base) << 10) | row_in_sub_block``, same records and bases; a chunk's narrow rounds are stored sub-block
by sub-block). The entries that stay wide are MERGED per unit: one wide section sorted by (column, row in unit),
packed ``(col << 12) | row12``, lane-interleaved and padded to whole rounds per unit (``dim > 2^20``: keys relative
to the per-round bases ``wbase``). Entries are moved, not duplicated, and four blocks' pad rounds become one. A
tail gather instruction then reads the columns of four times as many rows: 0.40 instead of 0.53 distinct 64-byte
lines per wide entry at the bench shape (``scripts/tl_tail_lines.py``). Unit table: 10 ints ``{row_lo, nrows, e_lo,
e_hi, n_lo, n_hi, n1, n2, n3, sb}`` -- the narrow rounds of sub-block k are ``[n_k, n_k+1)`` with ``n_0 = n_lo`` and
``n_4 = n_hi``. ``nstats`` is one (loss, sum l') pair per non-empty SUB-BLOCK, number ``sb + k`` with ``sb`` = 4 x
the unit's index: the kernel sums a sub-block's pair exactly as the row-block kernel sums a 1024-row block's, so a
shard's loss does not depend on the unit height, bit for bit. The kernel (``tl_fwd_tall_block``) keeps ONE fp64 accumulator row of
4096 slots per work-group: wave k walks sub-block k's narrow rounds, then one wave walks the wide section.

TILE GROUPS (``PML_TL_TGROUP=0/1`` or ``tgroup=``; by default, ``shard_tgroup``: bf16 / fp32 shards in the
interleaved + narrow layout with 1024-column tiles, chunks whose rows fit 20 bits, ``dim >= 2^16`` and at least 96
full chunks -- smaller shards are slower with them, ``profiles/tl_t_groups.md``; fp64 shards and the 2048-column
tiles of sparse shards keep the items above): the mirror image of the tall forward units. A GROUP is four consecutive tiles ``4g .. 4g+3`` of a
transpose chunk in which every non-empty tile has exactly one item; split (hot) tiles, their quadruples and the
leftover tiles keep their items and ``tl_t_item``. The narrow rounds are built per tile exactly as above and stay
where they are. The entries that stay wide are MERGED per group into FOUR sub-windows: an entry goes to sub-window q
when ``tl_t_item``'s wave q would walk its round (round r of a tile with nr wide rounds: ``nr q / 4 <= r <
nr (q + 1) / 4``), and a sub-window is sorted by (row, column in group), packed ``(local_row << 12) | col12``,
lane-interleaved and padded to whole rounds. Entries are moved, not duplicated, and up to four tiles' pad rounds
become one. A wide gather then reads the per-row values of four tiles' entries: 0.41 instead of 0.53 distinct 64-byte
lines per wide entry in such tiles (``scripts/tl_tail_lines.py --transpose``). Restricted to one column, a sub-window
holds that column's entries of quarter q in row order, so the kernel (``tl_t_group``: one fp64 accumulator row of
4096 slots, for q = 0..3 the four tiles' narrow quarters q, then sub-window q, then ``tot = q ? tot + acc : acc``)
performs the additions of ``tl_t_item`` in its order and grouping and the results are the ungrouped layout's BIT FOR
BIT. Group table (``groups``, 24 ints): ``{tile0, part[4], n_lo[4], n_hi[4], e_lo[4], e_hi[4], chunk, row_base,
-}``; ``part`` = -1 (add into G), a partial-row slot (shard-wide tables: the slot the tile's item would have, so
the combine is unchanged) or ``TG_EMPTY`` for a tile without entries. ``items`` holds the remaining items only;
:meth:`TLTChunk.unit_tiles` / ``unit_counts`` / ``logical`` list the items, then the groups' tiles. Readers that walk
items (column statistics, row-sampled copies) take :meth:`TLTChunk.ungrouped`.

Both copies are stored LANE-INTERLEAVED by default (``il``; ``PML_TL_IL=0`` keeps the plain order): every work
unit (forward block / transpose item) starts on a 256-entry round boundary and is zero-padded to whole rounds,
and inside a round the 16-B quad of lane L holds the unit's sorted entries L, L+64, L+128, L+192, so each gather
instruction of the kernels reads 64 consecutive sorted entries (``tl_stream_il`` in ``glm_kernels.hip``). Padding
costs < 0.5 % of the stream at the bench shapes.

The builders run with torch ops on the data's device (GPU sort for the 100M-entry bench chunks, CPU in tests).
Values keep the shard precision (bf16 / fp32 / fp64). Both copies cost 4 B + sizeof(value) per entry, the same
as the segmented-stream CSR/CSC pair they replace. Shapes the packing cannot represent (``D > 2^27`` or chunks
of more than 2^27 rows) fall back to the segmented-stream layout (:mod:`photon_ml_amd.ops.device`).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .native import TLFwdDesc, TLTDesc

# Widths the kernels run (glm_kernels.hip tl_maxbits / tl_with_acc), the same through the shard-wide launches
# (tl_fwd_multi / tl_t_multi) and the per-chunk ones (tl_fwd / tl_t): 5 .. 11 bits for every precision with fp64 LDS
# accumulators (4 waves x 2048 x 8 B = 64 KB at 11); 12 bits (4096 rows per block / columns per tile) for bf16 and
# fp32 shards only, which accumulate in fp32 there (4 waves x 4096 x 4 B = 64 KB). An fp64 shard asking for 12 gets 11.
TL_MAXBITS = 12
TL_MAXBITS_F64 = 11
TL_MINBITS = 5
DEFAULT_RBITS = int(os.environ.get("PML_TL_RBITS", 10))
DEFAULT_CBITS = int(os.environ.get("PML_TL_CBITS", 10))
DEFAULT_ITEM_ENTRIES = 1 << 18  # 125M rows (profiles/bench_knob_sweep.md): 64K 40.41, 128K 38.71-39.10, 256K 38.43-38.51, 512K 38.58, 1M 38.63 ms/step
_PAD = 8                 # kernels read 4-entry quads; pad so that the last quad stays in bounds
COMBINE_SEG = 16         # minimum partial rows summed per level-1 combine work-group


# XCD-aware item order of the shard-wide transpose (PML_TL_XCD=8 turns it on). Work-groups are dispatched
# round-robin over the 8 XCDs by blockIdx, each XCD has its own 4 MB L2, and an item gathers the per-row vector of
# ITS chunk (1M rows x 4 B): interleaving 8 streams (chunks c = k mod 8 in stream k) makes the blocks that share
# an XCD walk one chunk at a time. Pure scheduling (bitwise-identical results) -- but MEASURED SLOWER on the
# headline bench (40.0-40.1 vs 39.2 ms/step, profiles/bench_xcd_order_ab.md), so the default is the plain
# chunk-major order, in which all XCDs share the few in-flight chunks.
XCD_GROUPS = int(os.environ.get("PML_TL_XCD", "0"))


def xcd_order(chunk_of_item: np.ndarray, groups: int) -> np.ndarray:
    """Permutation of items (chunk-major input order kept inside each stream) such that position b holds an
    item of stream b % groups while every stream has items left."""
    stream = np.asarray(chunk_of_item) % groups
    lists = [np.flatnonzero(stream == k) for k in range(groups)]
    longest = max(len(l) for l in lists)
    grid = np.full((longest, groups), -1, dtype=np.int64)
    for k, l in enumerate(lists):
        grid[: len(l), k] = l
    order = grid.reshape(-1)
    return order[order >= 0]


def combine_seg(k: int) -> int:
    """Partial rows per level-1 combine unit of a tile split into ``k`` items: ~sqrt(k) (at least COMBINE_SEG), so
    neither level loops over more than ~sqrt(k) rows per thread. A hot tile of a 125M-row shard has ~47K items:
    fixed 16-row units left its level-2 sum a 2.9K-long serial chain per thread (1 ms per pass, measured)."""
    return max(COMBINE_SEG, int(math.ceil(math.sqrt(k))))
IL_ROUND = 256           # entries per wave-round of the kernels (64 lanes x 4-entry quads)
TL_VEC = 4               # entries per lane per round
INTERLEAVE = int(os.environ.get("PML_TL_IL", "1"))
NARROW = int(os.environ.get("PML_TL_NARROW", "1"))
NARROW_W = 64            # key window loaded per narrow round (one wave64 load)
FUSE = int(os.environ.get("PML_TL_FUSE", "1"))   # bf16 narrow rounds as fused 16-byte lane records
WIDE_BASE = int(os.environ.get("PML_TL_WIDE_BASE", "1"))   # per-round key bases for wide shards (TLFwdChunk)
# Tall forward units (TLFwdChunk, "TALL FORWARD UNITS" above): PML_TL_TALL=0/1 overrides the engagement rule.
TALL = os.environ.get("PML_TL_TALL")
TALL = None if TALL is None else bool(int(TALL))
TALL_DEFAULT = True      # the rule engages on its own (False: only PML_TL_TALL=1 / the constructor argument)
TALL_BITS = 12           # rows of a tall unit (2^12 fp64 sums = 32 KB of LDS per work-group)
TALL_SUB_BITS = 10       # rows of its sub-blocks: the slot bits of the narrow rounds' 16-bit packs
TALL_MIN_DIM = 1 << 16
TALL_COLS = 10           # ints per row of a tall unit table
# Tile groups (TLTChunk, "TILE GROUPS" above): PML_TL_TGROUP=0/1 (read when a chunk is built) overrides the rule.
# Engaged per SHARD (shard_tgroup): bit-for-bit equal results; on the 125M-row headline 33.38-33.48 vs 34.14-34.18
# ms/step (three alternated runs each), neutral at 62.5M rows and SLOWER on small shards, whose few groups are long
# one-wave units that leave CUs idle (16M rows: 5.76 vs 4.88 ms/step, 3M rows: 2.83 vs 1.27); profiles/tl_t_groups.md.
TGROUP_DEFAULT = True    # False: only PML_TL_TGROUP=1 / the constructor argument
TG_MIN_CHUNKS = 96       # full chunks of a shard for the groups to engage on their own (~22K groups at the bench shape)
TG_BITS = 12             # columns of a tile group (2^12 fp64 sums = 32 KB of LDS per work-group)
TG_SUB_BITS = 10         # columns of its tiles
TG_MIN_DIM = 1 << 16
TG_COLS = 24             # ints per row of a group table
TG_EMPTY = -2            # ``part`` of a group's tile without entries (nothing is written for it)


def narrow_width(sbits: int) -> int:
    """Largest key span of a narrow round: the 16-bit pack holds (key - base) in 16 - sbits bits."""
    return min(NARROW_W, 1 << max(16 - sbits, 0))


def _bits(n: int) -> int:
    return max(1, int(n - 1).bit_length())


def _cap(want: int, f64: bool) -> int:
    return min(want, TL_MAXBITS_F64 if f64 else TL_MAXBITS)


# fp64 shards over wide feature spaces use 2048-row forward blocks: an fp64 coefficient gather covers half the
# columns per cache line of an fp32 one, so the denser keys of a bigger block pay there (game5pl fp64 fixed effect:
# 54.4 -> 52.2 ms per coordinate update; the bf16 shards are faster with 1024-row blocks: 32.2 vs 33.2 ms;
# profiles/tl_tile_knobs_r4.md). PML_TL_RBITS overrides.
F64_WIDE_RBITS = 11


def default_rbits(dim: int, f64: bool) -> int:
    if f64 and dim >= (1 << 16) and "PML_TL_RBITS" not in os.environ:
        return F64_WIDE_RBITS
    return DEFAULT_RBITS


def fwd_bits(dim: int, f64: bool = False, want: Optional[int] = None) -> Optional[int]:
    r = min(_cap(default_rbits(dim, f64) if want is None else want, f64), 32 - _bits(dim))
    return r if r >= TL_MINBITS else None


def t_bits(chunk_rows: int, f64: bool = False, want: Optional[int] = None) -> Optional[int]:
    c = min(_cap(DEFAULT_CBITS if want is None else want, f64), 32 - _bits(chunk_rows))
    return c if c >= TL_MINBITS else None


# Sparse shards: when a 1024-column tile of a row chunk holds fewer than this many entries on average, the transpose
# copies use 2048-column tiles and 128K-entry items instead (measured on the game5pl fixed-effect shard, 25M rows x
# 30 non-zeros over 1M features, ~31K entries per tile and chunk: FE coordinate 34.65 -> 32.83 ms; the headline
# shard, ~102K entries per tile and chunk, is faster with the defaults: 37.88 vs 38.12 ms/step;
# profiles/tl_tile_knobs_r4.md). PML_TL_CBITS / PML_TL_ITEM_ENTRIES override.
SPARSE_TILE_ENTRIES = 1 << 16


def shard_t_config(nnz: int, n_rows: int, dim: int, chunk_rows: int):
    """``(cbits, item_entries)`` for the transpose copies of a whole shard (one choice for every chunk: the
    shard-wide transpose needs one tile width); ``(None, None)`` = the defaults."""
    if "PML_TL_CBITS" in os.environ or "PML_TL_ITEM_ENTRIES" in os.environ or n_rows <= 0 or dim < (1 << 16):
        return None, None                      # (small feature spaces keep the defaults: a few tiles at most)
    per_tile = (nnz / n_rows) * min(chunk_rows, n_rows) / math.ceil(dim / 1024)
    if per_tile < SPARSE_TILE_ENTRIES:
        return 11, 1 << 17
    return None, None


def tl_supported(dim: int, chunk_rows: int) -> bool:
    return fwd_bits(dim) is not None and t_bits(chunk_rows) is not None


def _to_u32_bits(x64: torch.Tensor) -> torch.Tensor:
    """int64 values in [0, 2^32) -> int32 tensor with the same low 32 bits (the kernels read uint32)."""
    return torch.where(x64 >= (1 << 31), x64 - (1 << 32), x64).to(torch.int32)


def _pad(t: torch.Tensor) -> torch.Tensor:
    return torch.cat([t, torch.zeros(_PAD, dtype=t.dtype, device=t.device)]).contiguous()


def il_phys(e_lo: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """Physical positions of the logical entries of units starting at ``e_lo`` (round-aligned) with ``n``
    entries each, in unit order: logical j of a unit lives at e_lo + 256*(j//256) + 4*(j%64) + (j%256)//64."""
    e_lo = e_lo.to(torch.int64)
    n = n.to(torch.int64)
    tot = int(n.sum())
    unit = torch.repeat_interleave(torch.arange(n.numel(), device=n.device), n)
    j = torch.arange(tot, device=n.device) - (torch.cumsum(n, 0) - n)[unit]
    t = j & (IL_ROUND - 1)
    return e_lo[unit] + (j - t) + ((t & 63) << 2) + (t >> 6)


def _interleave(pack: torch.Tensor, val: torch.Tensor, n: torch.Tensor, tail: int = _PAD):
    """Lane-interleave sorted streams whose units are consecutive runs of ``n`` entries. Returns the padded
    streams and the new (round-aligned) unit starts. ``tail``: spare entries after the last round (the interleaved
    readers stay inside whole rounds, so 0 is safe for them)."""
    n = n.to(torch.int64)
    padded = (n + IL_ROUND - 1) // IL_ROUND * IL_ROUND
    new_lo = torch.cumsum(padded, 0) - padded
    total = int(padded.sum()) + tail
    phys = il_phys(new_lo, n)
    p = torch.zeros(total, dtype=pack.dtype, device=pack.device)
    v = torch.zeros(total, dtype=val.dtype, device=val.device)
    p[phys] = pack
    v[phys] = val
    return p, v, new_lo


def _empty_narrow(val: torch.Tensor):
    dev = val.device
    return (torch.zeros(IL_ROUND, dtype=torch.int16, device=dev), torch.zeros(IL_ROUND, dtype=val.dtype, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))


def split_narrow(pack: torch.Tensor, val: torch.Tensor, n: torch.Tensor, sbits: int, xlen: int, enable: bool = True):
    """Move the narrow rounds of every unit out of sorted, unit-contiguous streams.

    ``pack`` (int64, low 32 bits = the packed entry ``key << sbits | slot``) and ``val`` hold units of ``n[u]``
    consecutive entries, each unit sorted by key. Returns ``(wide_pack, wide_val, wide_n, npack, nval, nbase,
    nrounds)``: the remaining entries per unit (same order), the interleaved 16-bit narrow stream (int16 bit
    patterns), its values, one base per narrow round and the number of narrow rounds per unit. bf16 values with
    ``FUSE``: ``npack`` is the fused record stream (int16, 8 words per lane: 4 packs, 4 value bit patterns) and
    ``nval`` is None."""
    dev = pack.device
    n = n.to(torch.int64)
    U = n.numel()
    gcount = n // IL_ROUND
    W = narrow_width(sbits)
    ok = enable and NARROW and W >= 16 and xlen >= NARROW_W and int(gcount.sum()) > 0
    if not ok:
        z = torch.zeros(U, dtype=torch.int64, device=dev)
        return (pack, val, n, *_empty_narrow(val), z)
    starts = torch.cumsum(n, 0) - n
    gu = torch.repeat_interleave(torch.arange(U, device=dev), gcount)
    gi = torch.arange(gu.numel(), device=dev) - (torch.cumsum(gcount, 0) - gcount)[gu]
    gs = starts[gu] + IL_ROUND * gi
    key = pack >> sbits
    first, last = key[gs], key[gs + IL_ROUND - 1]
    base = torch.clamp(first, max=xlen - NARROW_W)        # the 64-wide window load stays inside x
    nar = (last - base) < W
    gs_n, base = gs[nar], base[nar]
    idx = gs_n[:, None] + torch.arange(IL_ROUND, device=dev)[None, :]
    p16 = ((key[idx] - base[:, None]) << sbits) | (pack[idx] & ((1 << sbits) - 1))
    # interleave: logical t = 64 k + L of a round lives at 4 L + k
    il = lambda t: t.reshape(-1, TL_VEC, 64).transpose(1, 2).reshape(-1)
    npack = il(torch.where(p16 >= 32768, p16 - 65536, p16).to(torch.int16)).contiguous()
    nval = il(val[idx]).contiguous()
    if FUSE and val.dtype == torch.bfloat16:
        npack = torch.cat([npack.view(-1, TL_VEC), nval.view(torch.int16).view(-1, TL_VEC)], 1).reshape(-1)
        nval = None
    nbase = base.to(torch.int32).contiguous()
    # narrow rounds per unit: gu is non-decreasing (units' rounds are consecutive), so a prefix sum of the flags read
    # at the unit boundaries (torch.bincount on these long runs of one bin serialised its atomics)
    cs = torch.zeros(nar.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nar.to(torch.int64), 0, out=cs[1:])
    ge = torch.cumsum(gcount, 0)
    nrounds = cs[ge] - cs[ge - gcount]
    keep = torch.ones(pack.numel(), dtype=torch.bool, device=dev)
    keep[idx.reshape(-1)] = False
    del idx, p16
    return pack[keep], val[keep], n - IL_ROUND * nrounds, npack, nval, nbase, nrounds



def narrow_logical(npack: torch.Tensor, nval: torch.Tensor, nbase: torch.Tensor, r_lo, r_hi, sbits: int):
    """(pack32 as int64, val) of narrow rounds [r_lo, r_hi) in logical order."""
    r = torch.arange(int(r_lo), int(r_hi), device=npack.device)
    if not r.numel():
        return torch.zeros(0, dtype=torch.int64, device=npack.device), nval[:0].reshape(-1)
    ph = (r[:, None] * IL_ROUND + torch.arange(IL_ROUND, device=npack.device)[None, :]).reshape(-1, 64, TL_VEC)
    ph = ph.transpose(1, 2).reshape(-1)          # physical position of logical entry t of each round
    # (a fused chunk passes its strided views into the record stream: position 4 L + k = word k of lane L's record)
    rl, rh = int(r_lo) * IL_ROUND, int(r_hi) * IL_ROUND
    ph = ph - rl
    p16 = npack.reshape(-1, TL_VEC)[rl // TL_VEC:rh // TL_VEC].reshape(-1)[ph].to(torch.int64) & 0xFFFF
    base = nbase[r].to(torch.int64).repeat_interleave(IL_ROUND)
    return ((((p16 >> sbits) + base) << sbits) | (p16 & ((1 << sbits) - 1)),
            nval.reshape(-1, TL_VEC)[rl // TL_VEC:rh // TL_VEC].reshape(-1)[ph])


class _NarrowMixin:
    """Narrow-section bookkeeping shared by the forward and transpose chunks (``table`` columns 4, 5 hold the
    per-unit narrow round range [n_lo, n_hi); the wide window is columns ``_ew``)."""

    wbase = None          # forward copies only: int32 key base per physical wide round (see TLFwdChunk)

    nrec = None           # fused chunks: the record stream (int16, 8 words per lane record)

    def _set_narrow(self, npack, nval, nbase):
        """``nval`` None: ``npack`` is the fused record stream (``split_narrow``); the kernels tell the layouts
        apart by the null value pointer."""
        from .native import TLNarrow
        self.nrec = npack if nval is None else None
        if nval is None:
            rec = npack.view(-1, 2 * TL_VEC)
            npack, nval = rec[:, :TL_VEC], rec[:, TL_VEC:].view(torch.bfloat16)
        self.npack, self.nval, self.nbase = npack, nval, nbase
        self.nar = TLNarrow(npack.data_ptr(), None if self.fused else nval.data_ptr(), nbase.data_ptr(),
                            None if self.wbase is None else self.wbase.data_ptr())

    @property
    def fused(self) -> bool:
        return self.nrec is not None

    @property
    def n_narrow_rounds(self) -> int:
        t = self._table()
        return int((t[:, 5] - t[:, 4]).sum()) if t.shape[0] else 0

    def unit_counts(self) -> torch.Tensor:
        t = self._table().to(torch.int64)
        lo, hi = self._ew
        return (t[:, hi] - t[:, lo]) + IL_ROUND * (t[:, 5] - t[:, 4])

    def narrow_window(self, r_lo: int, r_hi: int):
        return narrow_logical(self.npack, self.nval, self.nbase, r_lo, r_hi, self._sbits)

    def _logical_all(self, wide_pack, wide_val):
        """Units in table order; inside a unit its narrow entries, then its wide entries."""
        t = self._table().to(torch.int64)
        dev = wide_pack.device
        lo, hi = self._ew
        nn = IL_ROUND * (t[:, 5] - t[:, 4])
        nw = t[:, hi] - t[:, lo]
        if int(nn.sum()) == 0:
            return wide_pack, wide_val
        npk, nvl = narrow_logical(self.npack, self.nval, self.nbase, 0, int(t[:, 5].max()), self._sbits)
        # narrow rounds of a unit are consecutive and in unit order -> gather them unit by unit
        U = t.shape[0]
        nu = torch.repeat_interleave(torch.arange(U, device=dev), nn.to(dev))
        nj = torch.arange(int(nn.sum()), device=dev) - (torch.cumsum(nn, 0) - nn).to(dev)[nu]
        npos = t[:, 4].to(dev)[nu] * IL_ROUND + nj
        wu = torch.repeat_interleave(torch.arange(U, device=dev), nw.to(dev))
        unit = torch.cat([nu, wu])
        order = torch.sort(unit, stable=True).indices
        wp = wide_pack.to(torch.int64) & 0xFFFFFFFF if wide_pack.dtype == torch.int32 else wide_pack.to(torch.int64)
        pk = torch.cat([npk[npos], wp])[order]
        vl = torch.cat([nvl[npos], wide_val])[order]
        return pk, vl


def tall_engages(tall: Optional[bool], dim: int, m: int, dtype, il: int, want_rbits: int) -> bool:
    """Whether a forward chunk of ``m`` rows is built with tall units. The layout can hold bf16 / fp32 chunks in the
    interleaved + narrow layout with 1024-row sub-blocks (fp64 shards keep their own block policy). Forced by
    ``tall`` (constructor) or ``PML_TL_TALL``; else wide feature spaces (``dim >= 2^16``: below, the whole
    coefficient vector is a few hundred cache lines and the tail gathers are cheap already) and chunks of at least
    one full unit."""
    if not (il and NARROW and dtype != torch.float64 and want_rbits == TALL_SUB_BITS):
        return False
    if tall is None:
        tall = TALL
    if tall is None:
        tall = TALL_DEFAULT and dim >= TALL_MIN_DIM and m >= (1 << TALL_BITS)
    return bool(tall)


def tgroup_engages(tgroup: Optional[bool], dim: int, chunk_rows: int, dtype, il: int, cbits: int) -> bool:
    """Whether a transpose chunk is built with tile groups (module docstring, TILE GROUPS). The layout can hold
    bf16 / fp32 chunks in the interleaved + narrow layout with 1024-column tiles whose rows fit ``32 - 12`` bits
    (fp64 shards and the 2048-column tiles of sparse shards keep their items), and then only when asked for: by
    ``tgroup`` (constructor; the shard builders pass :func:`shard_tgroup`) or ``PML_TL_TGROUP``."""
    if not (il and NARROW and dtype != torch.float64 and cbits == TG_SUB_BITS
            and _bits(chunk_rows) + TG_BITS <= 32):
        return False
    if tgroup is None and os.environ.get("PML_TL_TGROUP") is not None:
        tgroup = bool(int(os.environ["PML_TL_TGROUP"]))
    return bool(tgroup)


def shard_tgroup(dim: int, n_rows: int, chunk_rows: int) -> Optional[bool]:
    """One choice for every transpose chunk of a shard: wide feature spaces (``dim >= 2^16``) and at least
    ``TG_MIN_CHUNKS`` full chunks -- a group is a long unit (four tiles walked by one work-group, their wide entries by
    one wave at a time), and a shard with few of them leaves CUs idle (module constants). None (``PML_TL_TGROUP``
    decides) when that is set."""
    if os.environ.get("PML_TL_TGROUP") is not None:
        return None
    return bool(TGROUP_DEFAULT and dim >= TG_MIN_DIM and n_rows >= TG_MIN_CHUNKS * chunk_rows)


def shard_tall(dim: int, chunk_rows: int) -> Optional[bool]:
    """One choice for every chunk of a shard (the shard-wide forward launch needs one unit height): the rule applied
    to the shard's widest column window and to its full chunks, so a short last chunk follows the others (a ragged
    tall unit). None (each chunk's own rule) when ``PML_TL_TALL`` decides anyway."""
    if TALL is not None:
        return None
    return bool(TALL_DEFAULT and dim >= TALL_MIN_DIM and chunk_rows >= (1 << TALL_BITS))


class TLFwdChunk(_NarrowMixin):
    """Forward copy of one row chunk (``m`` rows)."""

    kind = "tl"

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, dim: int,
                 rbits: Optional[int] = None, il: Optional[int] = None, tall: Optional[bool] = None):
        """``tall``: True / False force the tall-unit layout on / off (where the layout can hold the chunk at all:
        bf16 / fp32 values, interleaved + narrow, 1024-row sub-blocks); None: ``PML_TL_TALL``, else the rule of
        :func:`tall_engages`."""
        dev = val.device
        self.il = INTERLEAVE if il is None else int(il)
        rowptr = rowptr.to(dev, torch.int64)
        col = col.to(dev, torch.int64)
        m = rowptr.numel() - 1
        f64 = val.dtype == torch.float64
        self.rbits = fwd_bits(dim, f64, rbits)
        if self.rbits is None:
            raise ValueError(f"tiled forward layout cannot pack dim={dim}")
        # wide shards: (col << rbits) would overflow 32 bits at the wanted block size -> keys relative to one base
        # per wide round (the full block size instead of 2^(32 - bits(D)) rows; see tl_stream_ring)
        want = _cap(default_rbits(dim, f64) if rbits is None else rbits, f64)
        self.tbits = 0
        if tall_engages(tall, dim, m, val.dtype, self.il, want) and self._init_tall(rowptr, col, val, dim, m):
            return
        use_base = bool(self.il) and WIDE_BASE and want > self.rbits
        if use_base:
            self.rbits = want
        R = 1 << self.rbits
        kbits = _bits(dim) + self.rbits                       # bits of (col << rbits) | row
        nnz = col.numel()
        rows = torch.repeat_interleave(torch.arange(m, device=dev), rowptr[1:] - rowptr[:-1]) if nnz else \
            torch.zeros(0, dtype=torch.int64, device=dev)
        pack = (col << self.rbits) | (rows & (R - 1))
        key = ((rows >> self.rbits) << kbits) | pack
        key, perm = torch.sort(key, stable=True)
        nblk = (m + R - 1) // R
        b = torch.arange(nblk, device=dev)
        lo = b * R
        hi = torch.clamp(lo + R, max=m)
        e_lo, e_hi = rowptr[lo], rowptr[hi]
        self._sbits, self._ew = self.rbits, (2, 3)
        n_lo = n_hi = torch.zeros(nblk, dtype=torch.int64, device=dev)
        if self.il:
            wp, wv, wn, npk, nvl, nbs, nr = split_narrow(key & ((1 << kbits) - 1), val[perm], e_hi - e_lo,
                                                         self.rbits, dim)
            del key, perm
            if use_base:
                wp = self._rebase(wp, wn)
                if wp is None:      # a wide round spans more keys than 32 - rbits bits: plain packs, fewer rows
                    del wv, npk, nvl, nbs
                    self.__init__(rowptr, col, val, dim, fwd_bits(dim, f64, rbits), il, tall=False)
                    return
            self.pack, self.val, e_lo = _interleave(_to_u32_bits(wp), wv, wn)
            e_hi = e_lo + wn
            n_hi = torch.cumsum(nr, 0)
            n_lo = n_hi - nr
            del wp, wv
        else:
            self.pack = _pad(_to_u32_bits(key & ((1 << kbits) - 1)))
            self.val = _pad(val[perm].contiguous())
            npk, nvl, nbs = _empty_narrow(val)
            del key, perm
        del rows
        self._set_narrow(npk, nvl, nbs)
        self.blk = torch.stack([lo, hi - lo, e_lo, e_hi, n_lo, n_hi], 1).to(torch.int32).contiguous()
        self.nblk, self.m, self.nnz = nblk, m, nnz
        self.desc = TLFwdDesc(self.blk.data_ptr(), nblk, self.rbits, self.pack.data_ptr(), self.val.data_ptr(),
                              self.il, self.nar)

    def _init_tall(self, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, dim: int, m: int) -> bool:
        """The tall-unit layout (module docstring, TALL FORWARD UNITS). False: some wide round of a shard with
        per-round bases spans more keys than 32 - 12 bits, nothing was set and the caller builds today's layout."""
        dev = val.device
        S, T = TALL_SUB_BITS, TALL_BITS
        cb = _bits(dim)
        nnz = col.numel()
        rows = torch.repeat_interleave(torch.arange(m, device=dev), rowptr[1:] - rowptr[:-1]) if nnz else \
            torch.zeros(0, dtype=torch.int64, device=dev)
        # narrow sections: per 1024-row sub-block, exactly as in the plain layout
        key = ((rows >> S) << (cb + S)) | (col << S) | (rows & ((1 << S) - 1))
        del rows
        key, perm = torch.sort(key, stable=True)
        nunit = (m + (1 << T) - 1) >> T
        nsub = nunit << (T - S)                               # sub-block slots; those past the last row are empty
        slo = torch.clamp(torch.arange(nsub, device=dev) << S, max=m)
        cnt = rowptr[torch.clamp(slo + (1 << S), max=m)] - rowptr[slo]
        wp, wv, wn, npk, nvl, nbs, nr = split_narrow(key & ((1 << (cb + S)) - 1), val[perm], cnt, S, dim)
        del key, perm
        # wide section: the wide entries of a unit's sub-blocks merged and sorted by (column, row in unit)
        # (the entries arrive sorted by (sub-block, column, row), so a STABLE sort by (unit, column) alone leaves them
        # in (unit, column, sub-block, row) = (unit, column, row in unit) order: a 32-bit key at the bench shape, half
        # the radix passes of the full 64-bit key)
        sub = torch.repeat_interleave(torch.arange(nsub, device=dev), wn)
        tp = ((wp >> S) << T) | ((sub & ((1 << (T - S)) - 1)) << S) | (wp & ((1 << S) - 1))
        ukey = ((sub >> (T - S)) << cb) | (wp >> S)
        del sub, wp
        if _bits(max(nunit, 1)) + cb <= 31:
            ukey = ukey.to(torch.int32)
        tperm = torch.sort(ukey, stable=True).indices
        del ukey
        tp, wv = tp[tperm], wv[tperm]
        del tperm
        un = wn.view(nunit, -1).sum(1)
        if cb + T > 32:
            tp = self._rebase(tp, un, T) if WIDE_BASE else None
            if tp is None:
                self.wbase = None
                return False
        self.rbits, self.tbits = S, T
        # (no spare quad after the last round: tall chunks are interleaved only, and the 16 bytes a unit table row
        # gains over a row block's must not make a one-sub-block chunk larger than the plain layout's)
        self.pack, self.val, e_lo = _interleave(_to_u32_bits(tp), wv, un, tail=0)
        del tp, wv
        nh = torch.cumsum(nr, 0)
        nl = (nh - nr).view(nunit, -1)
        ulo = torch.arange(nunit, device=dev) << T
        self._sbits, self._ew = S, (2, 3)
        self._set_narrow(npk, nvl, nbs)
        self.blk = torch.stack([ulo, torch.clamp(ulo + (1 << T), max=m) - ulo, e_lo, e_lo + un, nl[:, 0],
                                nh.view(nunit, -1)[:, -1], nl[:, 1], nl[:, 2], nl[:, 3], ulo >> S],
                               1).to(torch.int32).contiguous()
        self.nblk, self.m, self.nnz = nunit, m, nnz
        self.desc = TLFwdDesc(self.blk.data_ptr(), nunit, S, self.pack.data_ptr(), self.val.data_ptr(), 1, self.nar,
                              tbits=T)
        return True

    @property
    def ubits(self) -> int:
        """Row bits of a unit of the table = slot bits of the wide packs and of :meth:`logical`'s packs."""
        return self.tbits or self.rbits

    def _rebase(self, wp: torch.Tensor, wn: torch.Tensor, bits: Optional[int] = None) -> Optional[torch.Tensor]:
        """Wide packs (int64 ``(key << bits) | slot``, units of ``wn`` sorted entries; ``bits``: rbits unless given)
        relative to the first key of their round of the interleaved layout; sets ``self.wbase`` (int32 per physical
        round). None when some round's key span does not fit 32 - bits bits."""
        dev = wp.device
        bits = self.rbits if bits is None else bits
        n = wn.to(torch.int64)
        tot = int(n.sum())
        padded = (n + IL_ROUND - 1) // IL_ROUND * IL_ROUND
        nrounds = int(padded.sum()) // IL_ROUND
        wbase = torch.zeros(nrounds + 1, dtype=torch.int64, device=dev)
        if tot:
            unit = torch.repeat_interleave(torch.arange(n.numel(), device=dev), n, output_size=tot)
            j = torch.arange(tot, device=dev) - (torch.cumsum(n, 0) - n)[unit]
            rid = ((torch.cumsum(padded, 0) - padded)[unit] + j) // IL_ROUND     # same rounds as _interleave
            del unit
            key = wp >> bits
            first = (j % IL_ROUND) == 0
            del j
            wbase[rid[first]] = key[first]
            rel = key - wbase[rid]
            del rid, key, first
            if int(rel.max()) >= 1 << (32 - bits):
                return None
            wp = (rel << bits) | (wp & ((1 << bits) - 1))
        self.wbase = wbase.to(torch.int32).contiguous()
        return wp

    @property
    def nstats(self) -> int:
        # tall units: one pair per non-empty sub-block (table column 9 holds a unit's first pair)
        return (self.m + (1 << self.rbits) - 1) >> self.rbits if self.tbits else self.nblk

    parts_needed = 0

    def _table(self):
        return self.blk

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.blk, self.pack, self.val, self.npack, self.nval,
                                                           self.nbase) + (() if self.wbase is None else (self.wbase,)))

    def logical(self):
        """(pack, val) of the non-zeros in unit order (per block: its narrow entries, then its wide entries, each
        sorted by column), whatever the storage order; packs as non-negative int64 ``(col << ubits) | row`` (a tall
        unit: its narrow entries sub-block by sub-block, ``row`` = the row in the unit)."""
        if not self.il:
            return self.pack[: self.nnz].to(torch.int64) & 0xFFFFFFFF, self.val[: self.nnz]
        ph = il_phys(self.blk[:, 2], self.blk[:, 3] - self.blk[:, 2])
        wp = self.pack[ph].to(torch.int64) & 0xFFFFFFFF
        ub = self.ubits
        if self.wbase is not None:
            wp = ((self.wbase[ph // IL_ROUND].to(torch.int64) + (wp >> ub)) << ub) | (wp & ((1 << ub) - 1))
        if not self.tbits:
            return self._logical_all(wp, self.val[ph])
        t = self.blk.to(torch.int64)
        dev = wp.device
        U = t.shape[0]
        if not U or int((t[:, 5] - t[:, 4]).sum()) == 0:
            return wp, self.val[ph]
        S, T = self.rbits, self.tbits
        # the narrow rounds of a chunk are stored sub-block by sub-block, so unit by unit: rounds [0, last n_hi)
        npk, nvl = narrow_logical(self.npack, self.nval, self.nbase, 0, int(t[-1, 5]), S)
        bounds = torch.stack([t[:, 4], t[:, 6], t[:, 7], t[:, 8], t[:, 5]], 1)
        per_sub = (bounds[:, 1:] - bounds[:, :-1]).reshape(-1)
        esub = torch.repeat_interleave(torch.arange(per_sub.numel(), device=dev), IL_ROUND * per_sub.to(dev))
        npk = ((npk >> S) << T) | ((esub & ((1 << (T - S)) - 1)) << S) | (npk & ((1 << S) - 1))
        unit = torch.cat([esub >> (T - S), torch.repeat_interleave(torch.arange(U, device=dev),
                                                                   (t[:, 3] - t[:, 2]).to(dev))])
        order = torch.sort(unit, stable=True).indices
        return torch.cat([npk, wp])[order], torch.cat([nvl, self.val[ph]])[order]

    # host emulation of the kernel arithmetic (tests / CPU fallback)
    def emulate_matvec(self, x: torch.Tensor) -> torch.Tensor:
        pk, vl = self.logical()
        p = pk.to(torch.int64)
        col = p >> self.ubits
        blk_of_entry = torch.repeat_interleave(torch.arange(self.nblk, device=p.device), self.unit_counts())
        row = (blk_of_entry << self.ubits) + (p & ((1 << self.ubits) - 1))
        z = torch.zeros(self.m, dtype=torch.float64, device=p.device)
        return z.index_add_(0, row, vl.to(torch.float64) * x.to(torch.float64)[col])


class TLTChunk(_NarrowMixin):
    """Transpose copy of one row chunk."""

    kind = "tl"

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, dim: int, chunk_rows: int,
                 cbits: Optional[int] = None, item_entries: Optional[int] = None, il: Optional[int] = None,
                 tgroup: Optional[bool] = None):
        """``tgroup``: True / False force the tile-group layout on / off (where the layout can hold the chunk at
        all); None: ``PML_TL_TGROUP``, else the rule of :func:`tgroup_engages`."""
        self.il = INTERLEAVE if il is None else int(il)
        if item_entries is None:
            item_entries = int(os.environ.get("PML_TL_ITEM_ENTRIES", DEFAULT_ITEM_ENTRIES))
        self._chunk_rows, self._item_entries = chunk_rows, item_entries
        dev = val.device
        rowptr = rowptr.to(dev, torch.int64)
        col = col.to(dev, torch.int64)
        m = rowptr.numel() - 1
        self.cbits = t_bits(max(chunk_rows, m), val.dtype == torch.float64, cbits)
        if self.cbits is None:
            raise ValueError(f"tiled transpose layout cannot pack chunk_rows={chunk_rows}")
        C = 1 << self.cbits
        nnz = col.numel()
        rows = torch.repeat_interleave(torch.arange(m, device=dev), rowptr[1:] - rowptr[:-1]) if nnz else \
            torch.zeros(0, dtype=torch.int64, device=dev)
        tile = col >> self.cbits
        pack = (rows << self.cbits) | (col & (C - 1))
        key = (tile << 32) | pack
        del rows, pack
        key, perm = torch.sort(key, stable=True)
        del tile
        ntiles = (dim + C - 1) // C
        # entries per tile from the sorted keys (tile = key >> 32): binary search, no atomics
        tptr = torch.searchsorted(key >> 32, torch.arange(ntiles + 1, device=dev)).cpu().numpy().astype(np.int64)
        counts = np.diff(tptr)
        pack = _to_u32_bits(key & 0xFFFFFFFF)
        val = val[perm]
        del key, perm
        nz = np.nonzero(counts)[0]
        n_it = np.maximum(1, -(-counts[nz] // item_entries))
        # items of every non-empty tile, vectorised: item i of a tile of k items covers [a + (b-a) i / k, ...)
        it_tile = np.repeat(nz, n_it)
        it_i = np.arange(len(it_tile)) - np.repeat(np.cumsum(n_it) - n_it, n_it)
        it_k = np.repeat(n_it, n_it)
        a, b = tptr[it_tile], tptr[it_tile + 1]
        lo, hi = a + (b - a) * it_i // it_k, a + (b - a) * (it_i + 1) // it_k
        split = it_k > 1
        part_of = np.full(len(it_tile), -1, np.int64)
        part_of[split] = np.arange(int(split.sum()))
        # level-1 combine units of ~sqrt(k) consecutive partial rows per split tile (combine_seg)
        km = n_it[n_it > 1]
        plo = np.cumsum(km) - km
        sg = np.maximum(COMBINE_SEG, np.ceil(np.sqrt(km)).astype(np.int64)) if len(km) else km
        nu = -(-km // sg)
        u_mt = np.repeat(np.arange(len(km)), nu)
        u_first = np.repeat(plo, nu) + np.repeat(sg, nu) * (np.arange(int(nu.sum())) - np.repeat(np.cumsum(nu) - nu, nu))
        u_last = np.minimum(u_first + np.repeat(sg, nu), np.repeat(plo + km, nu))
        cu = np.column_stack([u_mt, u_first, u_last]) if len(km) else np.zeros((0, 3), np.int64)
        mt_tiles = nz[n_it > 1].tolist()
        mt_ptr = np.r_[0, np.cumsum(nu)].tolist() if len(km) else [0]
        self.nitems, self.nmt, self.nparts, self.ncu = len(it_tile), len(mt_tiles), int(km.sum()), len(cu)
        items = np.column_stack([it_tile, lo, hi, part_of]).astype(np.int64).reshape(-1, 4)
        items = np.column_stack([items, np.zeros((len(items), 2), np.int64)])
        self._sbits, self._ew = self.cbits, (1, 2)
        # tile groups: complete quadruples of tiles 4g .. 4g+3 whose non-empty tiles all have one item
        gsel = np.zeros(len(items), dtype=bool)
        gok = np.zeros(0, dtype=bool)
        if len(items) and ntiles >= 4 and tgroup_engages(tgroup, dim, max(chunk_rows, m), val.dtype, self.il,
                                                          self.cbits):
            k_of_tile = np.zeros(ntiles, np.int64)
            k_of_tile[nz] = n_it
            gok = k_of_tile[: (ntiles >> 2) << 2].reshape(-1, 4).max(1) == 1
            g_of_item = items[:, 0] >> 2
            gsel = (g_of_item < len(gok)) & gok[np.minimum(g_of_item, len(gok) - 1)]
        groups = np.zeros((0, TG_COLS), np.int64)
        if self.il:
            cnt = torch.from_numpy(items[:, 2] - items[:, 1]).to(dev)
            wp, wv, wn, npk, nvl, nbs, nr = split_narrow(pack.to(torch.int64) & 0xFFFFFFFF, val, cnt, self.cbits, m)
            del pack, val
            nr = nr.cpu().numpy()
            items[:, 5] = np.cumsum(nr)
            items[:, 4] = items[:, 5] - nr
            if gsel.any():
                wp, wv, wn, gcnt = self._merge_groups(wp, wv, wn, items[:, 0], gsel, len(gok))
                gidx = np.flatnonzero(gok)
                groups = np.zeros((len(gidx), TG_COLS), np.int64)
                it_of_tile = np.full(ntiles, -1, np.int64)
                it_of_tile[items[gsel, 0]] = np.flatnonzero(gsel)
                it4 = it_of_tile[gidx[:, None] * 4 + np.arange(4)[None, :]]
                groups[:, 0] = gidx * 4
                groups[:, 1:5] = np.where(it4 >= 0, -1, TG_EMPTY)
                groups[:, 5:9] = np.where(it4 >= 0, items[it4, 4], 0)
                groups[:, 9:13] = np.where(it4 >= 0, items[it4, 5], 0)
                items = items[~gsel]
            self.pack, self.val, new_lo = _interleave(_to_u32_bits(wp), wv, wn)
            del wp, wv
            new_lo, wn = new_lo.cpu().numpy(), wn.cpu().numpy()
            items[:, 1] = new_lo[: len(items)]
            items[:, 2] = items[:, 1] + wn[: len(items)]
            if len(groups):
                groups[:, 13:17] = new_lo[len(items):].reshape(-1, 4)
                groups[:, 17:21] = groups[:, 13:17] + wn[len(items):].reshape(-1, 4)
            self.nitems = len(items)
        else:
            self.pack, self.val = _pad(pack), _pad(val.contiguous())
            npk, nvl, nbs = _empty_narrow(val)
            del pack, val
        self._set_narrow(npk, nvl, nbs)
        self.items = torch.tensor(items.astype(np.int32), device=dev)
        self.mt_tiles = torch.tensor(np.asarray(mt_tiles or [0], dtype=np.int32), device=dev)
        self.mt_ptr = torch.tensor(np.asarray(mt_ptr, dtype=np.int32), device=dev)
        self.cu = torch.tensor(np.asarray(cu if len(cu) else [(0, 0, 0)], dtype=np.int32).reshape(-1, 3), device=dev)
        self.m, self.nnz, self.dim = m, nnz, dim
        self.ngroups = len(groups)
        self.groups = torch.tensor(groups.astype(np.int32), device=dev).reshape(-1, TG_COLS)
        self._make_desc()

    def _make_desc(self):
        self.desc = TLTDesc(self.items.data_ptr(), self.nitems, self.cbits, self.pack.data_ptr(),
                            self.val.data_ptr(), self.mt_tiles.data_ptr(), self.mt_ptr.data_ptr(), self.nmt, self.dim,
                            self.cu.data_ptr(), self.ncu, self.nparts, self.il, self.nar,
                            groups=self.groups.data_ptr() if self.ngroups else None, ngroups=self.ngroups)

    @staticmethod
    def _merge_groups(wp, wv, wn, tile_of_item, gsel, ngroups_all):
        """Move the wide entries of the grouped items (``gsel``) behind those of the other items, merged per group
        into four sub-windows: an entry goes to the sub-window of its QUARTER, the wave of ``tl_t_item`` that walks
        its round today (round r of an item with nr wide rounds: wave (4 r + 3) // nr, i.e. nr w / 4 <= r <
        nr (w + 1) / 4), and a sub-window is sorted by (row, column in group), packed ``(row << 12) | col12``.
        Returns the new streams, the entries per unit (the remaining items, then 4 sub-windows per group that
        holds entries) and the sub-window counts."""
        dev = wp.device
        S, T = TG_SUB_BITS, TG_BITS
        gs = torch.from_numpy(gsel).to(dev)
        n_items = wn.numel()
        tot = int(wn.sum())
        item = torch.repeat_interleave(torch.arange(n_items, device=dev), wn, output_size=tot)
        eg = gs[item]
        it_g = item[eg]
        j = torch.arange(tot, device=dev)[eg] - (torch.cumsum(wn, 0) - wn)[it_g]
        del item
        nrw = (wn + IL_ROUND - 1) // IL_ROUND
        quarter = (4 * (j // IL_ROUND) + 3) // nrw[it_g]
        tile = torch.from_numpy(np.ascontiguousarray(tile_of_item)).to(dev)[it_g]
        del j, it_g
        p = wp[eg]
        p12 = ((p >> S) << T) | ((tile & 3) << S) | (p & ((1 << S) - 1))
        win = (tile >> 2) * 4 + quarter
        del p, tile, quarter
        skey = (win << 32) | p12
        order = torch.sort(skey, stable=True).indices
        del skey
        gp, gv = p12[order], wv[eg][order]
        bounds = torch.searchsorted(win[order].contiguous(), torch.arange(4 * ngroups_all + 1, device=dev))
        wcnt = (bounds[1:] - bounds[:-1]).view(-1, 4)
        gok = torch.zeros(ngroups_all, dtype=torch.bool, device=dev)
        gok[torch.from_numpy(np.unique(tile_of_item[gsel] >> 2)).to(dev)] = True
        gcnt = wcnt[gok].reshape(-1)
        keep = ~eg
        return (torch.cat([wp[keep], gp]), torch.cat([wv[keep], gv]), torch.cat([wn[~gs], gcnt]), gcnt)

    @property
    def parts_needed(self) -> int:
        """fp64 scratch: item partial rows followed by the level-1 combine rows."""
        return (self.nparts + self.ncu) << self.cbits

    def _table(self):
        return self.items

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.items, self.mt_tiles, self.mt_ptr, self.cu, self.pack,
                                                           self.val, self.npack, self.nval, self.nbase, self.groups))

    # the UNITS of a chunk with tile groups: its items, then the four tiles of every group (a tile without entries
    # is a unit of none)
    def unit_tiles(self) -> torch.Tensor:
        t = self.items[:, 0].to(torch.int64)
        if not self.ngroups:
            return t
        g0 = self.groups[:, 0].to(torch.int64)
        return torch.cat([t, (g0[:, None] + torch.arange(4, device=t.device)[None, :]).reshape(-1)])

    def unit_counts(self) -> torch.Tensor:
        c = super().unit_counts()
        if not self.ngroups:
            return c
        return torch.cat([c, self._group_units()[3]])

    def narrow_table(self) -> torch.Tensor:
        """int64 rows {tile, 0, 0, 0, n_lo, n_hi} of the items and of the groups' tiles in the narrow section's
        storage order (tile order; the items of a split tile in item order)."""
        t = self.items[: self.nitems].to(torch.int64)
        if not self.ngroups:
            return t
        g = self.groups.to(torch.int64)
        gt = torch.zeros((4 * g.shape[0], 6), dtype=torch.int64, device=t.device)
        gt[:, 0] = (g[:, :1] + torch.arange(4, device=t.device)[None, :]).reshape(-1)
        gt[:, 4], gt[:, 5] = g[:, 5:9].reshape(-1), g[:, 9:13].reshape(-1)
        gt = gt[g[:, 1:5].reshape(-1) != TG_EMPTY]
        allt = torch.cat([t[:, :6], gt])
        return allt[torch.sort(allt[:, 0], stable=True).indices]

    @property
    def n_narrow_rounds(self) -> int:
        g = self.groups.to(torch.int64)
        return _NarrowMixin.n_narrow_rounds.fget(self) + (int((g[:, 9:13] - g[:, 5:9]).sum()) if self.ngroups else 0)

    def _group_units(self):
        """(unit, pack, val, counts) of the groups' entries in unit order (unit = 4 x group + tile in group; per
        unit its narrow entries, then its wide entries in stored order), packs as ``(row << cbits) | column in
        tile``; cached."""
        if getattr(self, "_gunits", None) is not None:
            return self._gunits
        S, T = TG_SUB_BITS, TG_BITS
        g = self.groups.to(torch.int64)
        dev = g.device
        G = g.shape[0]
        wcnt = (g[:, 17:21] - g[:, 13:17]).reshape(-1)
        ph = il_phys(g[:, 13:17].reshape(-1), wcnt).to(self.pack.device)
        wp = (self.pack[ph].to(torch.int64) & 0xFFFFFFFF).to(dev)
        wv = self.val[ph].to(dev)
        gw = torch.repeat_interleave(torch.arange(4 * G, device=dev), wcnt) >> 2
        unit_w = gw * 4 + ((wp >> S) & 3)
        wp = ((wp >> T) << S) | (wp & ((1 << S) - 1))
        n_lo, nn = g[:, 5:9].reshape(-1), (g[:, 9:13] - g[:, 5:9]).reshape(-1) * IL_ROUND
        if int(nn.sum()):
            npk, nvl = narrow_logical(self.npack, self.nval, self.nbase, 0, int(g[:, 9:13].max()), S)
            unit_n = torch.repeat_interleave(torch.arange(4 * G, device=dev), nn)
            pos = n_lo[unit_n] * IL_ROUND + torch.arange(int(nn.sum()), device=dev) - (torch.cumsum(nn, 0) - nn)[unit_n]
            unit = torch.cat([unit_n, unit_w])
            order = torch.sort(unit, stable=True).indices
            unit, pk, vl = unit[order], torch.cat([npk[pos], wp])[order], torch.cat([nvl[pos], wv])[order]
        else:
            order = torch.sort(unit_w, stable=True).indices
            unit, pk, vl = unit_w[order], wp[order], wv[order]
        b = torch.searchsorted(unit.contiguous(), torch.arange(4 * G + 1, device=dev))
        self._gunits = (unit, pk, vl, b[1:] - b[:-1])
        return self._gunits

    def window(self, e_lo: int, e_hi: int):
        """(pack, val) of one item's wide window in sorted order."""
        if not self.il:
            return self.pack[e_lo:e_hi], self.val[e_lo:e_hi]
        ph = il_phys(torch.tensor([e_lo]), torch.tensor([e_hi - e_lo])).to(self.pack.device)
        return self.pack[ph], self.val[ph]

    def logical(self):
        """(pack, val) of the non-zeros in unit order (:meth:`unit_tiles` / :meth:`unit_counts`: the items, then the
        tiles of the groups), packs ``(row << cbits) | column in tile``."""
        if not self.il:
            return self.pack[: self.nnz], self.val[: self.nnz]
        ph = il_phys(self.items[:, 1], self.items[:, 2] - self.items[:, 1])
        pk, vl = self._logical_all(self.pack[ph], self.val[ph])
        if not self.ngroups:
            return pk, vl
        _, gp, gv, _ = self._group_units()
        return torch.cat([pk.to(torch.int64) & 0xFFFFFFFF, gp]), torch.cat([vl, gv])

    def coo(self):
        """(row, col, val) of the chunk's non-zeros sorted by (row, column)."""
        pk, vl = self.logical()
        p = pk.to(torch.int64) & 0xFFFFFFFF
        tile = torch.repeat_interleave(self.unit_tiles(), self.unit_counts())
        key = ((p >> self.cbits) << 32) | (tile << self.cbits) | (p & ((1 << self.cbits) - 1))
        key, order = torch.sort(key, stable=True)
        return key >> 32, key & 0xFFFFFFFF, vl[order]

    def ungrouped(self, cache: bool = True) -> "TLTChunk":
        """This chunk without tile groups, for the readers that walk items only (column statistics, row-sampled
        copies): rebuilt from the stored entries, so it is the chunk that ``tgroup=False`` would have built (cached;
        a chunk without groups is returned as is)."""
        if not self.ngroups:
            return self
        twin = getattr(self, "_ungrouped", None)
        if twin is None:
            row, col, val = self.coo()
            rowptr = torch.searchsorted(row.contiguous(), torch.arange(self.m + 1, device=row.device))
            twin = TLTChunk(rowptr, col, val, self.dim, self._chunk_rows, cbits=self.cbits,
                            item_entries=self._item_entries, il=self.il, tgroup=False)
            if cache:
                self._ungrouped = twin
        return twin

    def emulate_rmatvec(self, r: torch.Tensor, square: bool = False) -> torch.Tensor:
        pk, vl = self.logical()
        p = pk.to(torch.int64) & 0xFFFFFFFF
        row = p >> self.cbits
        tile_of_entry = torch.repeat_interleave(self.unit_tiles(), self.unit_counts())
        col = (tile_of_entry << self.cbits) + (p & ((1 << self.cbits) - 1))
        v = vl.to(torch.float64)
        if square:
            v = v * v
        g = torch.zeros(self.dim, dtype=torch.float64, device=p.device)
        return g.index_add_(0, col, v * r.to(torch.float64)[row])


class TLTMulti:
    """Shard-wide transpose over every row chunk in one launch (``tl_t_multi_kernel``).

    Items of all chunks keep their launch order (chunk, item); each carries its chunk (stream pointers), its row
    base (offset into the shard-length row vector) and a partial-row slot. Tiles hit by more than one item in the
    whole shard are combined by the same two-level fixed-order combine as a single chunk's split tiles, so the
    result is deterministic and independent of chunk scheduling. Requires one ``cbits`` for all chunks and
    column windows (if any) that start on tile boundaries (``tile_offsets``).
    """

    def __init__(self, chunks: Sequence["TLTChunk"], row_starts: Sequence[int], dim: int,
                 tile_range: Optional[Tuple[int, int]] = None, tile_offsets: Optional[Sequence[int]] = None):
        """``tile_range`` = [t0, t1): only the items of those column tiles (a gradient BUCKET: columns
        [t0 * C, t1 * C) are final after this launch + its combine, so their all-reduce can start).
        ``tile_offsets``: per chunk, the global tile of its local tile 0 (chunks stored in tile-aligned column
        windows); tiles that several chunks' items share are combined like split tiles."""
        from .native import TLTMultiDesc
        dev = chunks[0].pack.device
        self.cbits = chunks[0].cbits
        self.il = chunks[0].il
        if any(ch.il != self.il for ch in chunks):
            raise ValueError("TLTMulti: chunks mix interleaved and plain streams")
        # rows: the items of a chunk, then one row per non-empty tile of its tile groups (column 7: -1 for an item,
        # else 4 x the group's row in ``grp`` + the tile's number in the group) -- such a tile counts as an item of
        # its tile, so the partial-row slots and the combine tables are those of the same shard without groups
        its, grps = [], []
        n_grp = 0
        for c, ch in enumerate(chunks):
            it = ch.items[: ch.nitems].cpu().numpy().astype(np.int64).reshape(-1, 6)
            toff = 0 if tile_offsets is None else int(tile_offsets[c])
            its.append(np.column_stack([np.full(len(it), c), it[:, 0] + toff, it[:, 1], it[:, 2],
                                        np.full(len(it), row_starts[c]), it[:, 4], it[:, 5], np.full(len(it), -1)]))
            if getattr(ch, "ngroups", 0):
                g = ch.groups.cpu().numpy().astype(np.int64).reshape(-1, TG_COLS).copy()
                g[:, 0] += toff
                g[:, 21], g[:, 22], g[:, 23] = c, row_starts[c], np.arange(len(g))
                gi, k = np.nonzero(g[:, 1:5] != TG_EMPTY)
                z = np.zeros(len(gi), np.int64)
                its.append(np.column_stack([z + c, g[gi, 0] + k, z, z, z + row_starts[c], z, z,
                                            4 * (n_grp + gi) + k]))
                grps.append(g)
                n_grp += len(g)
        it = np.concatenate(its) if its else np.zeros((0, 8), np.int64)
        grp = np.concatenate(grps) if grps else np.zeros((0, TG_COLS), np.int64)
        real = it[:, 7] < 0
        src_all = np.cumsum(real) - 1                      # a real row's index into the chunks' concatenated items
        if tile_range is not None:
            in_range = (it[:, 1] >= tile_range[0]) & (it[:, 1] < tile_range[1])
            gin = np.zeros(len(grp), np.int64)
            np.add.at(gin, it[~real, 7] >> 2, np.where(in_range[~real], 1, 1 << 20))
            if np.any((gin % (1 << 20) > 0) & (gin >= (1 << 20))):
                raise ValueError("TLTMulti: tile_range cuts a tile group (round the range to multiples of 4 tiles)")
            it = it[in_range]
            src_all = src_all[in_range]
            real = real[in_range]
        n = len(it)
        tile = it[:, 1]
        order = np.lexsort((np.arange(n), tile))          # grouped by tile, (chunk, item) order inside
        ts = tile[order]
        starts = np.flatnonzero(np.r_[True, ts[1:] != ts[:-1]]) if n else np.zeros(0, np.int64)
        k = np.diff(np.r_[starts, n])                    # items per tile (shard-wide)
        multi_tile = np.repeat(k > 1, k)
        part = np.full(n, -1, np.int64)
        part[order[multi_tile]] = np.arange(int(multi_tile.sum()))
        # level-1 units of <= COMBINE_SEG consecutive partial rows per split tile
        km = k[k > 1]
        plo = np.cumsum(km) - km
        sg = np.maximum(COMBINE_SEG, np.ceil(np.sqrt(km)).astype(np.int64)) if len(km) else km
        nu = -(-km // sg)
        u_tile = np.repeat(np.arange(len(km)), nu)
        u_first = np.repeat(plo, nu) + np.repeat(sg, nu) * (np.arange(int(nu.sum())) - np.repeat(np.cumsum(nu) - nu, nu))
        u_last = np.minimum(u_first + np.repeat(sg, nu), np.repeat(plo + km, nu))
        self.nparts, self.ncu, self.nmt = int(km.sum()), int(nu.sum()), len(km)
        # the group tiles' slots go to their group rows; the launch table holds the items only
        slot = it[~real, 7]
        grp[slot >> 2, 1 + (slot & 3)] = part[~real]
        used = np.zeros(len(grp), dtype=bool)
        used[slot >> 2] = True
        grp = grp[used]
        it, part, src = it[real], part[real], src_all[real]
        n = len(it)
        self.nitems, self.ngroups = n, len(grp)
        rows = np.column_stack([it[:, 0], it[:, 1], it[:, 2], it[:, 3], part, it[:, 4], it[:, 5],
                                it[:, 6]]).astype(np.int32)
        if XCD_GROUPS > 1 and n > XCD_GROUPS:
            xo = xcd_order(it[:, 0], XCD_GROUPS)
            rows, src = rows[xo], src[xo]
        self._src = torch.from_numpy(src.astype(np.int64)).to(dev)   # row -> index into the chunks' concatenated items
        self.items = torch.tensor(rows.reshape(-1, 8), device=dev)
        self.mt_tiles = torch.tensor(np.r_[ts[starts][k > 1], 0].astype(np.int32)[: max(self.nmt, 1)], device=dev)
        self.mt_ptr = torch.tensor(np.r_[0, np.cumsum(nu)].astype(np.int32), device=dev)
        self.cu = torch.tensor(np.column_stack([u_tile, u_first, u_last]).astype(np.int32).reshape(-1, 3)
                               if self.ncu else np.zeros((1, 3), np.int32), device=dev)
        self.ptrs = stream_ptr_table(chunks, dev)
        self._chunks = list(chunks)  # keep the streams alive
        # group rows as the chunks' (TG_COLS ints; tile0 global, the tiles' shard-wide slots, [21] chunk, [22] row
        # base); [23], the group's row in its chunk's table, is for the host emulation
        self.groups = torch.tensor(grp.astype(np.int32), device=dev).reshape(-1, TG_COLS)
        self.desc = TLTMultiDesc(self.items.data_ptr(), n, self.cbits, self.ptrs.data_ptr(),
                                 self.mt_tiles.data_ptr(), self.mt_ptr.data_ptr(), self.nmt, dim,
                                 self.cu.data_ptr(), self.ncu, self.nparts, self.il,
                                 groups=self.groups.data_ptr() if self.ngroups else None, ngroups=self.ngroups)

    @property
    def parts_needed(self) -> int:
        return (self.nparts + self.ncu) << self.cbits

    def restreamed(self, chunks: Sequence["TLTChunk"]) -> "TLTMulti":
        """The same launch over other streams of the SAME units (row-sampled copies, ``RowCompaction``): every
        row's stream window and narrow range come from ``chunks``' item tables (one device gather), tiles,
        partial-row slots and combine tables are shared. No host work beyond the pointer table."""
        import copy
        from .native import TLTMultiDesc
        if self.ngroups or any(getattr(ch, "ngroups", 0) for ch in chunks):
            raise ValueError("TLTMulti.restreamed: row-sampled copies are made of chunks without tile groups")
        dev = self.items.device
        cat =torch.cat([ch.items[: ch.nitems].to(torch.int64) for ch in chunks]) if chunks else None
        rows = self.items.to(torch.int64).clone()
        if self.nitems:
            sel = cat[self._src]
            rows[:, 2:4] = sel[:, 1:3]
            rows[:, 6:8] = sel[:, 4:6]
        new = copy.copy(self)
        new.items = rows.to(torch.int32).contiguous()
        new.ptrs = stream_ptr_table(chunks, dev)
        new._chunks = list(chunks)
        d = self.desc
        new.desc = TLTMultiDesc(new.items.data_ptr(), d.nitems, d.cbits, new.ptrs.data_ptr(), d.mt_tiles, d.mt_ptr,
                                d.nmt, d.dim, d.cu, d.ncu, d.nparts_total, d.il)
        return new

    def emulate_rmatvec(self, r: torch.Tensor, square: bool = False) -> torch.Tensor:
        """Host emulation of the launch + combine (item partial rows, direct tiles, two-level combine)."""
        C = 1 << self.cbits
        dim = self.desc.dim
        ntiles = (dim + C - 1) // C
        G = torch.zeros(ntiles * C, dtype=torch.float64)
        parts = torch.zeros((max(self.nparts, 1), C), dtype=torch.float64)
        r = r.to(torch.float64).cpu()
        for c, tile, e_lo, e_hi, part, rb, n_lo, n_hi in self.items.cpu().tolist():
            ch = self._chunks[c]
            pk, vl = ch.window(e_lo, e_hi)
            npk, nvl = ch.narrow_window(n_lo, n_hi)
            p = torch.cat([npk.cpu(), pk.to(torch.int64).cpu() & 0xFFFFFFFF])
            v = torch.cat([nvl.cpu(), vl.cpu()]).to(torch.float64)
            if square:
                v = v * v
            acc = torch.zeros(C, dtype=torch.float64).index_add_(0, p & (C - 1), v * r[rb + (p >> self.cbits)])
            if part < 0:
                G[tile * C:(tile + 1) * C] += acc
            else:
                parts[part] = acc
        for g in self.groups.cpu().tolist():
            ch = self._chunks[g[21]]
            unit, pk, vl, cnt = ch._group_units()
            ends = torch.cumsum(cnt, 0).cpu().tolist()
            for k in range(4):
                part, u = g[1 + k], 4 * g[23] + k
                if part == TG_EMPTY:
                    continue
                p = pk[ends[u] - int(cnt[u]):ends[u]].cpu()
                v = vl[ends[u] - int(cnt[u]):ends[u]].cpu().to(torch.float64)
                if square:
                    v = v * v
                acc = torch.zeros(C, dtype=torch.float64).index_add_(0, p & (C - 1), v * r[g[22] + (p >> self.cbits)])
                if part < 0:
                    G[(g[0] + k) * C:(g[0] + k + 1) * C] += acc
                else:
                    parts[part] = acc
        cu = self.cu.cpu().tolist()
        l1 = [parts[a:b].sum(0) for _, a, b in cu[: self.ncu]]
        mp = self.mt_ptr.cpu().tolist()
        for t, tile in enumerate(self.mt_tiles.cpu().tolist()[: self.nmt]):
            s = torch.zeros(C, dtype=torch.float64)
            for u in range(mp[t], mp[t + 1]):
                s += l1[u]
            G[tile * C:(tile + 1) * C] += s
        return G[:dim]


def stream_ptr_table(chunks, device) -> torch.Tensor:
    """Per-chunk stream pointers of the shard-wide kernels: {pack, val, narrow pack (fused chunks: the record
    stream), narrow val (0: fused records), narrow base, wide-round bases (0: absolute keys)}."""
    wb = lambda ch: 0 if getattr(ch, "wbase", None) is None else ch.wbase.data_ptr()
    return torch.tensor([[ch.pack.data_ptr(), ch.val.data_ptr(), ch.npack.data_ptr(),
                          0 if ch.fused else ch.nval.data_ptr(), ch.nbase.data_ptr(), wb(ch)] for ch in chunks],
                        dtype=torch.int64, device=device).reshape(-1)


# ---- row-sampled copies (K20 down-sampling work saving: DeviceGLMData.row_sampled) ---------------------------
CMP_SEG = 8              # rounds of one unit per compaction segment (tl_compact_kernel, one wave each)


def _cmp_segments(ch, narrow: bool):
    """Segment table of a chunk's units (cached per ``narrow``): int32 {unit, round_lo, round_hi} per segment, a
    unit's rounds numbered narrow first, then wide ([nn, nn + wide rounds)); ``narrow=False``: the wide rounds
    only. Plus each segment's unit, the unit's first segment (int64) and the chunk's narrow entry count."""
    cache = ch.__dict__.setdefault("_cmp_seg", {})
    if cache.get(narrow) is not None:
        return cache[narrow]
    t = ch._table().to(torch.int64)
    dev = t.device
    lo, hi = ch._ew
    nn = t[:, 5] - t[:, 4]
    R = (t[:, hi] - t[:, lo] + IL_ROUND - 1) // IL_ROUND + (nn if narrow else 0)
    ns = (R + CMP_SEG - 1) // CMP_SEG
    S = int(ns.sum())
    su = torch.repeat_interleave(torch.arange(t.shape[0], device=dev), ns, output_size=S)
    first = (torch.cumsum(ns, 0) - ns)[su]
    r_lo = (torch.arange(S, device=dev) - first) * CMP_SEG
    r_hi = torch.minimum(r_lo + CMP_SEG, R[su])
    if not narrow:
        r_lo, r_hi = r_lo + nn[su], r_hi + nn[su]
    seg = torch.stack([su, r_lo, r_hi], 1).to(torch.int32).contiguous()
    cache[narrow] = (seg, su, first, S, IL_ROUND * int(nn.sum()))
    return cache[narrow]


class RowCompaction:
    """Row-sampled copy of one interleaved tiled chunk (forward or transpose copy) by ``tl_compact_kernel``:
    the constructor queues the counting pass and the device-side scans (``total`` / ``kept`` stay on the device so
    that all chunks of a shard need ONE host sync), :meth:`finish` allocates the compacted streams, queues the
    writing pass and returns the new chunk. Every unit keeps its table slot (row block / transpose item, split-tile
    partial rows and combine tables unchanged).

    ``filter_narrow=False`` (most rows kept): only the WIDE entries are filtered and the narrow section is shared
    with the full chunk as is — a filtered narrow round no longer spans < 64 keys, and a wide round costs 4.4x a
    narrow round of texture-address time (``profiles/pmc_tl_multi_125M_r3.md``), so converting them made a
    half-kept shard as slow as the full one; the dropped rows' narrow entries still run (weight 0: their per-row
    coefficient is 0, their margins are never used). ``True`` (few rows kept, below ~80/352 of a round): the
    narrow entries are filtered too and the copy is all wide rounds."""

    def __init__(self, ch, keep: torch.Tensor, forward: bool, filter_narrow: bool = False):
        from .native import CmpArgs, check, require_game_lib, stream_handle
        if not ch.il:
            raise ValueError("row-sampled copies need the interleaved layout")
        if getattr(ch, "ngroups", 0):
            raise ValueError("row-sampled copies are made of a transpose chunk's ungrouped() copy")
        self.ch, self.keep, self.forward = ch, keep, forward
        dev = ch.pack.device
        self.filter_narrow = bool(filter_narrow)
        seg, su, first, S, self.n_narrow = _cmp_segments(ch, self.filter_narrow)
        table = ch._table()
        lo, hi = ch._ew
        self.seg_cnt = torch.zeros(max(S, 1), dtype=torch.int32, device=dev)
        self._keep_alive = (seg, table, keep)
        self.args = CmpArgs(table.data_ptr(), lo, 0 if forward else -1, seg.data_ptr(), S, ch._sbits,
                            0 if forward else 1, ch.pack.data_ptr(), ch.val.data_ptr(), ch.npack.data_ptr(),
                            None if ch.fused else ch.nval.data_ptr(), ch.nbase.data_ptr(), keep.data_ptr(),
                            self.seg_cnt.data_ptr(),
                            None, None, None, None, table.shape[1], getattr(ch, "ubits", ch._sbits) if forward
                            else ch._sbits)
        self.lib, self.stream = require_game_lib(), stream_handle(dev)
        self.vbytes = ch.val.element_size()
        if S:
            check(self.lib.pml_tl_compact(0, self.vbytes, ctypes.byref(self.args), self.stream), "tl_compact count")
        cnt = self.seg_cnt[:S].to(torch.int64)
        U = table.shape[0]
        self.unit_cnt = torch.zeros(U, dtype=torch.int64, device=dev).index_add_(0, su, cnt)
        padded = (self.unit_cnt + IL_ROUND - 1) // IL_ROUND * IL_ROUND
        self.unit_lo = (torch.cumsum(padded, 0) - padded).contiguous()
        excl = torch.cumsum(cnt, 0) - cnt
        self.seg_first = (excl - excl[first]).contiguous() if S else excl
        self.total, self.kept = padded.sum(), self.unit_cnt.sum()

    def finish(self, total: int, kept: int):
        import copy
        from .native import TLFwdDesc, TLTDesc, check
        ch = self.ch
        dev = ch.pack.device
        opack = torch.zeros(total + _PAD, dtype=torch.int32, device=dev)
        oval = torch.zeros(total + _PAD, dtype=ch.val.dtype, device=dev)
        a = self.args
        a.seg_first, a.unit_lo = self.seg_first.data_ptr(), self.unit_lo.data_ptr()
        a.opack, a.oval = opack.data_ptr(), oval.data_ptr()
        if a.nseg:
            check(self.lib.pml_tl_compact(1, self.vbytes, ctypes.byref(a), self.stream), "tl_compact write")
        lo, hi = ch._ew
        table = ch._table().to(torch.int64).clone()
        table[:, lo] = self.unit_lo
        table[:, hi] = self.unit_lo + self.unit_cnt
        if self.filter_narrow:
            table[:, 4:9] = 0            # (a tall unit table: its sub-blocks' first narrow rounds too; not column 9)
        table = table.to(torch.int32).contiguous()
        nc = copy.copy(ch)               # shares the narrow streams (npack / nval / nbase, table columns 4, 5)
        nc._cmp_seg = {}
        nc.pack, nc.val = opack, oval
        if self.filter_narrow:
            nc._set_narrow(*_empty_narrow(oval))
            nc.nnz = kept
        else:
            nc.nnz = kept + self.n_narrow
        if self.forward:
            nc.blk = table
            nc.desc = TLFwdDesc(table.data_ptr(), nc.nblk, nc.rbits, opack.data_ptr(), oval.data_ptr(), 1, nc.nar,
                                tbits=nc.tbits)
        else:
            nc.items = table
            nc.desc = TLTDesc(table.data_ptr(), nc.nitems, nc.cbits, opack.data_ptr(), oval.data_ptr(),
                              nc.mt_tiles.data_ptr(), nc.mt_ptr.data_ptr(), nc.nmt, nc.dim, nc.cu.data_ptr(), nc.ncu,
                              nc.nparts, 1, nc.nar)
        return nc
