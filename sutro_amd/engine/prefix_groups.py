"""Host-side grouping of decode rows for shared-prefix attention.

Rows whose block tables begin with the same shared (registered, multiply
held) blocks are packed into tiles of R rows; the partial kernel walks the P
common pages once per tile (csrc/attn_decode_prefix.hip). Everything here is
a deterministic function of the block tables and reference counts — no
hash-order or id-order iteration — so TP ranks build the same tiles without
communication.
"""

from __future__ import annotations

import numpy as np

GMAX = 8       # groups per step that get tiles; rows of further groups run P = 0
MIN_ROWS = 2   # a group of one shares nothing


def max_tiles(num_rows: int, tile_r: int) -> int:
    """Tiles that `num_rows` rows in at most GMAX groups can need."""
    return (num_rows + tile_r - 1) // tile_r + GMAX


def fill_prefix_tiles(tile_rows: np.ndarray, row_pages: np.ndarray,
                      bt: np.ndarray, seq_lens: np.ndarray, n: int,
                      prefix_blocks: np.ndarray, ref: np.ndarray,
                      block_size: int) -> int:
    """Fill `tile_rows` [NT, R] (-1 = empty) and `row_pages` [B] for the
    first `n` rows of `bt` [B, W]; returns the number of tiles used.

    A row's P is its count of leading table entries that are registered
    blocks (`prefix_blocks`) held by at least two tables, capped so one
    position stays beyond the prefix. A block held twice is a registered
    block, and a registered block has one parent, so equal `bt[i, P-1]`
    means equal leading P entries: rows group by that block id. A row deep
    in a chain of its own is lowered to the depth it shares with others."""
    tile_rows[:] = -1
    row_pages[:] = 0
    if n == 0:
        return 0
    R = tile_rows.shape[1]
    P = np.minimum(prefix_blocks[:n], (seq_lens[:n] - 1) // block_size)
    W = min(int(P.max()), bt.shape[1])
    if W <= 0:
        return 0
    shared = ref[bt[:n, :W]] >= 2
    shared &= np.arange(W)[None, :] < P[:, None]
    lead = np.cumprod(shared, axis=1).sum(axis=1)
    rows = np.nonzero(lead > 0)[0]
    if rows.size == 0:
        return 0
    keys = bt[rows, lead[rows] - 1]
    uniq, inv, counts = np.unique(keys, return_inverse=True,
                                  return_counts=True)
    # largest groups first, ties by block id
    order = np.lexsort((uniq, -counts))
    t = 0
    for g in order[:GMAX]:
        if counts[g] < MIN_ROWS:
            break
        members = rows[inv == g]  # ascending row order
        for i in range(0, len(members), R):
            chunk = members[i:i + R]
            tile_rows[t, :len(chunk)] = chunk
            t += 1
        row_pages[members] = lead[members]
    return t
