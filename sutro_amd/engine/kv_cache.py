"""Paged KV cache: block allocator + per-layer page tensors.

Layout (per layer, K and V separate):
    cache[num_blocks, num_kv_heads, block_size, head_dim]

chosen so a decode wave reads one page's (head, pos, :) rows as contiguous
16-byte vectors along head_dim, and the RoPE+cache-write kernel scatters each
new token's K/V row with a single dwordx4-per-lane store.

With `prefix_caching`, full blocks of computed PROMPT tokens are registered
in an exact-match index keyed by (parent physical block, the block's token
ids) and shared between rows by reference count (docs/ENGINE.md, "Prefix
cache"). Off (the default), the allocator is the plain free list.
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

# index key: (parent physical block or -1 for the first block, token ids)
PrefixKey = Tuple[int, Tuple[int, ...]]


class BlockAllocator:
    """Free-list allocator over KV page indices.

    With `prefix_caching` it also keeps per-block reference counts (the
    number of block tables holding the block), the prefix index, and an LRU
    of registered blocks nobody holds: those stay matchable until `allocate`
    runs out of free blocks and evicts them, oldest first."""

    def __init__(self, num_blocks: int, prefix_caching: bool = False) -> None:
        self.num_blocks = num_blocks
        self._free: List[int] = list(range(num_blocks - 1, -1, -1))
        self.prefix_caching = prefix_caching
        if prefix_caching:
            # numpy so the decode grouping can gather it by block table
            self.ref = np.zeros(num_blocks, dtype=np.int32)
            self._index: Dict[PrefixKey, int] = {}
            self._key_of: Dict[int, PrefixKey] = {}    # registered blocks
            self._nchild: Dict[int, int] = {}          # registered children
            # insertion-ordered (never hash- or id-ordered): the eviction
            # sequence is a function of the request sequence alone
            self._evictable: "OrderedDict[int, None]" = OrderedDict()

    @property
    def num_free(self) -> int:
        if self.prefix_caching:
            return len(self._free) + len(self._evictable)
        return len(self._free)

    def allocate(self, n: int) -> List[int]:
        if n > self.num_free:
            raise MemoryError(f"KV cache exhausted: need {n} blocks, have {self.num_free}")
        if not self.prefix_caching:
            return [self._free.pop() for _ in range(n)]
        out = []
        for _ in range(n):
            if not self._free:
                self._evict_one()
            out.append(self._free.pop())
        return out

    def free(self, blocks: List[int]) -> None:
        if not self.prefix_caching:
            self._free.extend(reversed(blocks))
            return
        # deepest block first into the LRU: a chain's leaf is always older
        # than its ancestors, so the LRU head never has registered children
        # and evicting it cannot orphan an index entry
        freed = []
        for b in reversed(blocks):
            if self.ref[b] > 0:
                self.ref[b] -= 1
            if self.ref[b] > 0:
                continue
            if b in self._key_of:
                self._evictable[b] = None
            else:
                freed.append(b)
        self._free.extend(freed)

    # ---- prefix index (prefix_caching only) ----

    def is_registered(self, block: int) -> bool:
        return block in self._key_of

    def num_evictable_in(self, blocks: Sequence[int]) -> int:
        return sum(1 for b in blocks if b in self._evictable)

    def incref(self, blocks: Sequence[int]) -> None:
        for b in blocks:
            if self.ref[b] == 0:
                self._evictable.pop(b, None)
            self.ref[b] += 1

    def lookup(self, parent: int, tokens: Tuple[int, ...]) -> Optional[int]:
        # the key holds the token ids themselves, so dict equality makes the
        # match exact — a hash collision cannot produce a hit
        return self._index.get((parent, tokens))

    def register(self, block: int, parent: int, tokens: Tuple[int, ...]) -> bool:
        """Index `block` under (parent, tokens). False when the key is taken
        (the caller keeps its block private)."""
        key = (parent, tokens)
        if key in self._index or block in self._key_of:
            return False
        assert parent < 0 or parent in self._key_of
        self._index[key] = block
        self._key_of[block] = key
        if parent >= 0:
            self._nchild[parent] = self._nchild.get(parent, 0) + 1
        return True

    def _evict_one(self) -> None:
        for b in self._evictable:
            if self._nchild.get(b, 0) == 0:
                break
        else:  # unreachable by the LRU ordering argument in free()
            raise MemoryError("no evictable KV block without registered children")
        del self._evictable[b]
        key = self._key_of.pop(b)
        del self._index[key]
        self._nchild.pop(b, None)
        if key[0] >= 0:
            self._nchild[key[0]] -= 1
        self._free.append(b)


class PagedKVCache:
    def __init__(
        self,
        num_layers: int,
        num_blocks: int,
        num_kv_heads: int,
        block_size: int,
        head_dim: int,
        dtype: torch.dtype,
        device: str,
        prefix_caching: bool = False,
    ) -> None:
        self.num_layers = num_layers
        self.num_blocks = num_blocks
        self.num_kv_heads = num_kv_heads
        self.block_size = block_size
        self.head_dim = head_dim
        shape = (num_blocks, num_kv_heads, block_size, head_dim)
        self.k_cache = [
            torch.zeros(shape, dtype=dtype, device=device) for _ in range(num_layers)
        ]
        self.v_cache = [
            torch.zeros(shape, dtype=dtype, device=device) for _ in range(num_layers)
        ]
        self.prefix_caching = prefix_caching
        self.allocator = BlockAllocator(num_blocks, prefix_caching)
        # per-sequence block tables (python side; tensorized per step)
        self.block_tables: Dict[int, List[int]] = {}
        # prefix caching: leading table entries of a row that are registered
        # blocks of one chain (matched at admission or registered by the row)
        self.prefix_blocks: Dict[int, int] = {}
        # rows whose chain ended at a block another row registered first
        self._chain_closed: set = set()

    def blocks_needed(self, seq_len: int) -> int:
        return (seq_len + self.block_size - 1) // self.block_size

    def can_grow(self, req_id: int, new_len: int) -> bool:
        have = len(self.block_tables.get(req_id, []))
        return self.blocks_needed(new_len) - have <= self.allocator.num_free

    def grow(self, req_id: int, new_len: int) -> None:
        """Ensure the sequence has pages covering new_len tokens."""
        table = self.block_tables.setdefault(req_id, [])
        need = self.blocks_needed(new_len) - len(table)
        if need > 0:
            new = self.allocator.allocate(need)
            if self.prefix_caching:
                self.allocator.incref(new)
            table.extend(new)

    def release(self, req_id: int) -> None:
        table = self.block_tables.pop(req_id, None)
        if table:
            self.allocator.free(table)
        if self.prefix_caching:
            self.prefix_blocks.pop(req_id, None)
            self._chain_closed.discard(req_id)

    def slot(self, req_id: int, pos: int) -> int:
        """Flat slot index for token position `pos` of a sequence."""
        table = self.block_tables[req_id]
        return table[pos // self.block_size] * self.block_size + pos % self.block_size

    # ---- prefix cache ----

    def match_prefix(self, prompt_token_ids: Sequence[int]) -> List[int]:
        """Longest chain of registered blocks equal to the prompt's leading
        full blocks, capped so at least one prompt token is left to compute
        (the row needs logits). No side effects."""
        bs = self.block_size
        alloc = self.allocator
        out: List[int] = []
        parent = -1
        for i in range((len(prompt_token_ids) - 1) // bs):
            b = alloc.lookup(parent, tuple(prompt_token_ids[i * bs:(i + 1) * bs]))
            if b is None:
                break
            out.append(b)
            parent = b
        return out

    def seed(self, req_id: int, blocks: List[int]) -> None:
        """Start a row's table with matched shared blocks."""
        assert req_id not in self.block_tables
        self.allocator.incref(blocks)
        self.block_tables[req_id] = list(blocks)
        self.prefix_blocks[req_id] = len(blocks)

    def register_computed(self, req_id: int, prompt_token_ids: Sequence[int],
                          num_computed: int) -> None:
        """Index the row's blocks that are now full of computed prompt
        tokens. Called after the step that computed them, never inside it."""
        if req_id in self._chain_closed:
            return
        table = self.block_tables.get(req_id)
        if table is None:
            return
        bs = self.block_size
        full = min(num_computed, len(prompt_token_ids)) // bs
        n = self.prefix_blocks.get(req_id, 0)
        alloc = self.allocator
        while n < full:
            parent = table[n - 1] if n else -1
            if not alloc.register(
                    table[n], parent, tuple(prompt_token_ids[n * bs:(n + 1) * bs])):
                self._chain_closed.add(req_id)
                break
            n += 1
        self.prefix_blocks[req_id] = n
