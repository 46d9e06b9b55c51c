"""What runs between two decode steps of a generation, as one object: the pick, then - where the call asked for them - the
log-probability launch, the stop check and the slots' tick.  generate, generate_many (admit and step) and DecodeGraph's captured step all
issue that sequence through PickStage.run, so it is written once."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .ops import ProcessorSets, SlotConstraints, StopSets      # the classes, bound here: isinstance must not depend on a patched ops attribute


def pick_rows_torch(logits, ids, pad_token_id: int, eos_ids, done, tokens, cache_len, start_len, done_at, proc=None, penalties=None):
    """What ops.greedy_pick does with advance = 0, in torch, for logits that are not bf16 (an f32 model: generate() picks those on the host
    loop too): next = pad for done rows, else the argmax of the (processed) row; tokens[b, cache_len[b] - start_len[b]] = next; a row whose
    next is an eos id becomes done at that index.  In place, on the device, no synchronisation.  penalties: the per-row
    frequency_penalty / presence_penalty tensors a ProcessorSets' apply takes, or None."""
    x = logits if proc is None else proc.apply(logits, tokens=tokens, cache_len=cache_len, start_len=start_len, done=done, **(penalties or {}))
    was_done = done.bool()
    nxt = torch.where(was_done, torch.full_like(ids, pad_token_id), x.float().argmax(dim=-1))
    t = (cache_len - start_len).long()
    ok = (t >= 0) & (t < tokens.shape[1])
    col = t.clamp(0, tokens.shape[1] - 1)[:, None]
    tokens.scatter_(1, col, torch.where(ok, nxt, tokens.gather(1, col)[:, 0])[:, None])
    ids.copy_(nxt)
    if eos_ids is not None:
        hit = (nxt[:, None] == eos_ids[None, :]).any(-1) & ~was_done
        done_at.copy_(torch.where(hit, t.to(torch.int32), done_at))
        done.copy_(torch.where(hit, torch.ones_like(done), done))


def _row(x, slot: int):
    """The one-row view of a per-row tensor or slot object; anything else (None, a number, the eos ids) as it is."""
    if isinstance(x, (SlotConstraints, ProcessorSets, StopSets)):
        return x.row(slot)
    return x[slot:slot + 1] if torch.is_tensor(x) else x


class PickStage:
    """The launches behind a decode step.
      pick            the keywords of ops.greedy_pick that stay the same from token to token: pad_token_id, eos_ids, done, tokens, start_len,
                      done_at, and optionally processors, processor_sets or slot_constraints, and the per-row frequency_penalty /
                      presence_penalty tensors.  eos_ids is shared by every row; the others that are tensors hold one row per sequence
      embed, next_embeds   the embedding gather of the pick (ops.greedy_pick's arguments of that name); run(embed=False) leaves it out
      sampler         ops.sample_pick's own keywords (temperature, top_k, top_p, seed, offset): the pick is the device sampler
      rows            ops.sample_pick_rows' per-row arrays (temperature, top_k, top_p, seed, optionally min_p): the pick is the per-row sampler
      processors_row  the second ops.LogitsProcessors, which owns the B = 1 scores scratch: what row() swaps `processors` for (the call-wide
                      one's scratch address is held by the captured step)
      logprob         ops.token_logprob's output keywords (top_k, out_logprob, out_top_ids, out_top_logprobs): that launch right behind the
                      pick - it scores the token at the index the pick just wrote
      stops           an ops.StopSets: the rows' stop sequences, checked behind the pick and the log-probability launch
      limit           int32 [rows], the slots' token budgets: ops.slot_tick closes the sequence (generate_many)
      torch_pick      the pick is pick_rows_torch (f32 logits): greedy only, the processors or sets applied through their `apply`
    Everything is resolved here, once; run() only issues launches, each through the ops module's attribute of that moment."""

    def __init__(self, pick: dict, embed=None, next_embeds: Optional[torch.Tensor] = None, sampler: Optional[dict] = None,
                 rows: Optional[dict] = None, processors_row=None, logprob: Optional[dict] = None, stops=None,
                 limit: Optional[torch.Tensor] = None, torch_pick: bool = False):
        if sampler is not None and rows is not None:
            raise ops.AkiError("PickStage: the scalar sampler or the per-row sampler, not both")
        if torch_pick and (sampler is not None or rows is not None or embed is not None):
            raise ops.AkiError("PickStage: the torch pick is greedy and gathers no embedding")
        self.pick, self.embed, self.next_embeds, self.sampler, self.rows = dict(pick), embed, next_embeds, sampler, rows
        self.processors_row, self.logprob, self.stops, self.limit, self.torch_pick = processors_row, logprob, stops, limit, torch_pick
        self.tokens, self.start_len, self.done, self.done_at = (self.pick.get(k) for k in ("tokens", "start_len", "done", "done_at"))
        self._op = "sample_pick_rows" if rows is not None else "sample_pick" if sampler is not None else "greedy_pick"
        self._plain = dict(self.pick, **(rows or sampler or {}))
        self._gather = self._plain if embed is None else dict(self._plain, embed=embed, next_embeds=next_embeds)
        if torch_pick:
            proc = self.pick.get("processor_sets") if self.pick.get("processor_sets") is not None else self.pick.get("processors")
            pen = {k: self.pick[k] for k in ("frequency_penalty", "presence_penalty") if self.pick.get(k) is not None}
            self._torch = (self.pick.get("pad_token_id", 0), self.pick.get("eos_ids"), self.done, self.tokens), \
                (self.start_len, self.done_at, proc, pen or None)
        self._lp = None if logprob is None else dict(logprob, tokens=self.tokens, start_len=self.start_len, done_at=self.done_at)
        self._tick = None if limit is None else dict(done=self.done, done_at=self.done_at, start_len=self.start_len, limit=limit)
        self._tick_stops = None if limit is None or stops is None else dict(self._tick, stops=stops, tokens=self.tokens)

    @property
    def sampling(self) -> bool:
        return self.sampler is not None or self.rows is not None

    def run(self, logits: torch.Tensor, ids: torch.Tensor, cache_len: torch.Tensor, advance: bool, embed: bool = True,
            fuse_stops: bool = True) -> None:
        """pick -> token_logprob? -> stop_check? -> slot_tick?, on the current stream.  ids receives the picked tokens; advance: the pick
        advances cache_len (the decode step before it ran with advance=False).  embed=False: without the embedding gather (the captured
        step feeds ids).  fuse_stops=False: with a tick, the stops are checked by a launch of their own ahead of it (the admit: a row the
        stop ends must not be ticked as live); else they ride in the tick's launch."""
        if self.torch_pick:
            head, tail = self._torch
            pick_rows_torch(logits, ids, *head, cache_len, *tail)
        else:
            getattr(ops, self._op)(logits, ids, cache_len=cache_len, advance=advance, **(self._gather if embed else self._plain))
        if self._lp is not None:
            ops.token_logprob(logits, cache_len=cache_len, **self._lp)
        fused = self._tick_stops is not None and fuse_stops
        if self.stops is not None and not fused:
            ops.stop_check(self.tokens, cache_len, self.start_len, self.done, self.done_at, self.stops)
        if self._tick is not None:
            ops.slot_tick(cache_len=cache_len, **(self._tick_stops if fused else self._tick))

    def row(self, slot: int) -> "PickStage":
        """The same stage over one-row views of row `slot` (x[slot:slot + 1] for tensors, .row(slot) for the slot objects): what a B = 1
        run on that row's logits takes.  The call-wide LogitsProcessors is swapped for processors_row."""
        pick = {k: (v if k == "eos_ids" else _row(v, slot)) for k, v in self.pick.items()}
        if pick.get("processors") is not None:
            pick["processors"] = self.processors_row
        each = lambda d: None if d is None else {k: _row(v, slot) for k, v in d.items()}
        return PickStage(pick, self.embed, _row(self.next_embeds, slot), self.sampler, each(self.rows), self.processors_row, each(self.logprob),
                         _row(self.stops, slot), _row(self.limit, slot), self.torch_pick)
