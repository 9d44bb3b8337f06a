"""Device-resident token history for the logit-penalty pass.

Repetition / presence / frequency penalties need each penalised row's full
token history (prompt + sampled tokens) next to the logits every step.
Uploading it per step would put O(rows x context) host traffic back into the
step loop, so the history lives on the device:

- `hist` is an int32 [max_num_seqs, Lcap] pool, allocated on the FIRST
  penalised request (engines that never see one allocate nothing);
- a penalised request owns one row (a *slot*) of it for as long as it holds
  KV pages: taken the first time the row is sampled (the prompt is written
  once, then), released by the scheduler's release hook on finish, abort and
  preemption;
- after each sampling step the sampler scatters the new token of every
  penalised row into `hist[slot, total_len]` straight from its device token
  tensor, so no token data crosses the bus again.

Invariant: whenever the penalty op runs for a request,
`hist[slot, :req.total_len]` equals `prompt_token_ids + output_token_ids`.
`hist_len` always comes from the request's own `total_len`; a preempted row
loses its output tokens (`Request.restart`), gets a fresh slot with the
prompt rewritten, and regenerates its output region.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .request import Request


class PenaltyState:
    def __init__(self, max_num_seqs: int, max_model_len: int,
                 device: str) -> None:
        self.capacity = int(max_num_seqs)
        # room for the token sampled at total_len == max_model_len - 1, kept
        # a multiple of 4 so rows stay 16-byte aligned for vector loads
        self.lcap = (int(max_model_len) + 1 + 3) // 4 * 4
        self.device = device
        self.hist: Optional[torch.Tensor] = None
        self._free: List[int] = list(range(self.capacity - 1, -1, -1))
        self._slots: Dict[int, int] = {}   # req_id -> slot

    @property
    def num_free(self) -> int:
        return len(self._free)

    def slot_of(self, req: Request) -> int:
        """The request's slot, taking one (and writing the prompt) on first
        use after admission."""
        s = self._slots.get(req.req_id)
        if s is not None:
            return s
        if self.hist is None:
            self.hist = torch.zeros((self.capacity, self.lcap),
                                    dtype=torch.int32, device=self.device)
        if not self._free:
            raise RuntimeError(
                "penalty history pool exhausted: more penalised rows are "
                "resident than max_num_seqs")
        s = self._free.pop()
        self._slots[req.req_id] = s
        toks = req.prompt_token_ids + req.output_token_ids
        if len(toks) > self.lcap:
            raise ValueError(
                f"request of {len(toks)} tokens exceeds the penalty history "
                f"row ({self.lcap})")
        if toks:
            self.hist[s, :len(toks)].copy_(
                torch.tensor(toks, dtype=torch.int32))
        return s

    def release(self, req: Request) -> None:
        """Give the request's slot back (no-op for rows that hold none)."""
        s = self._slots.pop(req.req_id, None)
        if s is not None:
            self._free.append(s)

    def append(self, slots: torch.Tensor, positions: torch.Tensor,
               tokens: torch.Tensor) -> None:
        """hist[slots[i], positions[i]] = tokens[i], all on the device."""
        self.hist.index_put_((slots, positions), tokens.to(torch.int32))
