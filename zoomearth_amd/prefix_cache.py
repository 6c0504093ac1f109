"""Prefix cache: which token blocks the engine's pool of K/V rows holds (`ze_prefix_*`, zoomearth_amd/csrc/ze_prefix.hip).

replaces: vLLM's automatic prefix caching, which the reference's trainer switches on for its generation engine
(`enable_prefix_caching=True`, src/train/RL/src/open-r1-multimodal/src/open_r1/trainer/vllm_grpo_trainer.py:414-417)
and which its "fast" evaluation path gets from the serving back-end (src/eval/infer_vllm.py): a prompt whose leading
tokens were computed before -- by a chain that has retired since -- takes their K/V rows from the pool and prefills only its tail.

The engine's pool is a block store.  This module owns everything else: a block's KEY (a hash chained over the blocks in front of it,
its own ids and the keys of the images that reach into it -- so equal keys mean equal tokens AND equal image features from row 0
on, which is all a K/V row depends on), the allocation of block ids, and eviction (least recently used first, leaves before their
parents, never a block a planned load still needs).  Only full blocks are stored; a block with an image that has no key is never
stored, nor is anything behind it.  A weight change moves the engine's generation: the cache then forgets everything (the engine
refuses to load such blocks anyway).
"""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .scheduler import cut_at_image_run, images_in


class Match(NamedTuple):
    rows: int                   # leading rows of the prompt the pool holds (0 = a miss)
    blocks: tuple               # the pool blocks that hold them, in order (the last one possibly in part)
    images: int                 # image runs inside those rows (whole, by construction)
    keys: tuple                 # the chain keys of `blocks`
    generation: int = 0         # the weight generation the match was made under: `load` refuses it under another


MISS = Match(0, (), 0, ())


class _Block:
    __slots__ = ("id", "parent", "children", "pins")

    def __init__(self, id_, parent):
        self.id, self.parent, self.children, self.pins = id_, parent, 0, 0


class PrefixCache:
    def __init__(self, engine, rows: int, block_rows: int = 32):
        self.engine, self.block_rows = engine, int(block_rows)
        self.n_blocks = int(rows) // self.block_rows
        if self.n_blocks <= 0:
            raise ValueError(f"a prefix cache of {rows} rows holds no block of {block_rows} rows")
        self.image_token_id = engine.config.image_token_id
        # One pool per engine.  A pool of exactly this shape that an earlier owner left behind is adopted -- as an empty one: its
        # blocks are only ever read through keys this object hands out -- so a second scheduler or server on the same engine works
        # whether or not the first one was closed; a pool of another shape is the caller's to destroy.
        have = engine.prefix_pool_info()[:2]
        if have != (self.n_blocks, self.block_rows):
            if have != (0, 0):
                raise ValueError(f"the engine already has a prefix pool of {have[0]} blocks of {have[1]} rows: close its owner first")
            engine.prefix_pool_create(self.n_blocks, self.block_rows)
        self.generation = engine.prefix_pool_info()[2]
        self.blocks = OrderedDict()            # chain key -> _Block, least recently used first
        self.free = list(range(self.n_blocks))[::-1]
        self.stats = dict(hit_rows=0, saved_rows=0, evicted_blocks=0, lookups=0, hits=0, flushes=0)

    def close(self) -> None:
        """Gives the pool back to the engine (which waits for the copies in flight)."""
        if self.engine is not None:
            self.engine.prefix_pool_destroy()
            self.engine = None
            self.blocks.clear()

    # ------------------------------------------------------------------ keys
    def block_keys(self, ids: Sequence[int], image_keys: Sequence, n_rows: Optional[int] = None) -> List[bytes]:
        """The chain keys of the full blocks of ids[:n_rows], up to (not including) the first block that an image without a key
        reaches into."""
        B, img = self.block_rows, self.image_token_id
        n = len(ids) if n_rows is None else min(int(n_rows), len(ids))
        a = np.asarray(ids[:n // B * B], dtype=np.int64)
        is_img = a == img
        starts = is_img & ~np.concatenate([[False], is_img[:-1]])
        run_of = np.where(is_img, np.cumsum(starts) - 1, -1)       # image run of every position, -1 = text
        out, prev = [], b""
        for j in range(len(a) // B):
            runs = np.unique(run_of[j * B:(j + 1) * B])
            touching = [image_keys[r] if r < len(image_keys) else None for r in runs.tolist() if r >= 0]
            if any(k is None for k in touching):
                break
            h = hashlib.blake2b(prev, digest_size=16)
            h.update(a[j * B:(j + 1) * B].tobytes())
            h.update(repr(touching).encode())
            prev = h.digest()
            out.append(prev)
        return out

    # ------------------------------------------------------------------ lookup
    def check_generation(self) -> None:
        """The engine's weights changed since the blocks were saved: they are all forgotten."""
        gen = self.engine.prefix_pool_info()[2]
        if gen != self.generation:
            self.generation = gen
            if self.blocks:
                self.stats["flushes"] += 1
            # (blocks a planned load has pinned go too: the engine refuses that load, and the request fails rather than read stale rows)
            self.blocks.clear()
            self.free = list(range(self.n_blocks))[::-1]

    def match(self, ids: Sequence[int], image_keys: Sequence = ()) -> Match:
        """The longest chain of present blocks that starts `ids`, cut by the rules of scheduler.shared_prefix_len / images_in: a
        non-empty tail stays, the match does not end inside a run of image tokens, and the images counted in it are whole."""
        self.check_generation()
        self.stats["lookups"] += 1
        B = self.block_rows
        found = []
        for key in self.block_keys(ids, image_keys):
            if key not in self.blocks:
                break
            found.append(key)
        n = cut_at_image_run(ids, min(len(found) * B, len(ids) - 1), self.image_token_id)
        if n <= 0:
            return MISS
        found = found[:(n + B - 1) // B]
        for key in found:
            self.blocks.move_to_end(key)
        self.stats["hits"] += 1
        return Match(n, tuple(self.blocks[k].id for k in found), images_in(ids, n, self.image_token_id), tuple(found), self.generation)

    def pin(self, m: Match) -> None:
        """A load of `m` is planned: its blocks stay until `unpin` (the engine orders a later save behind a load it was given)."""
        for k in m.keys:
            self.blocks[k].pins += 1

    def unpin(self, m: Match) -> None:
        for k in m.keys:
            b = self.blocks.get(k)
            if b is not None and b.pins > 0:
                b.pins -= 1

    def unpin_all(self) -> None:
        for b in self.blocks.values():
            b.pins = 0

    def load(self, m: Match, slots: Sequence[int], split_row: int = 0) -> None:
        """The matched rows into the chains `slots` (ONE launch; the first becomes the holder the others' decode attention reads)."""
        self.check_generation()
        if m.generation != self.generation:
            # the cache was emptied since the match was made: its block ids may name other chains' rows by now
            raise RuntimeError("the prefix cache was flushed by a weight change after this match was made")
        self.engine.prefix_load(m.blocks, m.rows, split_row, list(slots))
        self.stats["hit_rows"] += m.rows * len(slots)

    # ------------------------------------------------------------------ store
    def _evict_one(self, protected) -> bool:
        for key, b in self.blocks.items():      # least recently used first; a parent only after its children
            if b.children == 0 and b.pins == 0 and key not in protected:
                del self.blocks[key]
                if b.parent is not None and b.parent in self.blocks:
                    self.blocks[b.parent].children -= 1
                self.free.append(b.id)
                self.stats["evicted_blocks"] += 1
                return True
        return False

    def save(self, slot: int, ids: Sequence[int], image_keys: Sequence, n_rows: int, stream=None) -> int:
        """The full blocks of the first n_rows rows of chain `slot` (whose tokens are ids[:n_rows]) that the pool does not hold yet;
        returns the rows saved.  Never more blocks than the pool has: what does not fit after evicting everything evictable is
        left out, from the chain's end."""
        self.check_generation()
        keys = self.block_keys(ids, image_keys, n_rows)
        have = 0
        while have < len(keys) and keys[have] in self.blocks:
            self.blocks.move_to_end(keys[have])
            have += 1
        new = keys[have:]
        if not new:
            return 0
        protected = set(keys[:have])
        while len(self.free) < len(new) and self._evict_one(protected):
            pass
        new = new[:len(self.free)]
        if not new:
            return 0
        block_ids = [self.free.pop() for _ in new]
        try:
            if stream is not None:
                self.engine.prefix_save(slot, have * self.block_rows, block_ids, stream=stream)
            else:
                self.engine.prefix_save(slot, have * self.block_rows, block_ids)
        except Exception:
            self.free.extend(reversed(block_ids))
            raise
        parent = keys[have - 1] if have else None
        for key, bid in zip(new, block_ids):
            self.blocks[key] = _Block(bid, parent)
            if parent is not None:
                self.blocks[parent].children += 1
            parent = key
        self.stats["saved_rows"] += len(new) * self.block_rows
        return len(new) * self.block_rows
