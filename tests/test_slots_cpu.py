"""In-flight batching, the parts that need no GPU: the SlotScheduler driven by a fake token source, generate_many's keyword parsing, and the
slot capacity computed from the ids."""
import types

import pytest
import torch

from conftest import load_golden
from golden import gen

from aki_amd.slots import SlotScheduler, expanded_length, slot_capacity

LENGTHS = [1, 9, 3, 17, 8, 8, 2, 30, 1, 5, 12]


class FakeRows:
    """A token source with the device's semantics: a request of n tokens has token 0 at its admit and one more per decode step; a row is
    done from its last token on (ops.slot_tick), and only a look shows it.  Every event is logged."""

    def __init__(self, lengths, slots):
        self.lengths, self.slots = lengths, slots
        self.request = [None] * slots
        self.generated = [0] * slots
        self.done = [True] * slots
        self.step_no = 0
        self.finished_at = {}          # request -> the step count at which its last token was produced
        self.admitted_at = {}          # request -> (step count, slot)
        self.retired_at = {}           # request -> (step count, slot, tokens)
        self.look_steps = []
        self.results = {}

    def admit(self, req, slot):
        assert self.request[slot] is None, f"slot {slot} still holds request {self.request[slot]}"
        assert req not in self.admitted_at, f"request {req} admitted twice"
        self.request[slot], self.generated[slot] = req, 1
        self.done[slot] = self.lengths[req] == 1
        self.admitted_at[req] = (self.step_no, slot)
        if self.done[slot]:
            self.finished_at[req] = self.step_no
        return self.lengths[req] == 1

    def step(self, n):
        for _ in range(n):
            self.step_no += 1
            for s in range(self.slots):
                if self.request[s] is not None and not self.done[s]:
                    self.generated[s] += 1
                    if self.generated[s] >= self.lengths[self.request[s]]:
                        self.done[s] = True
                        self.finished_at[self.request[s]] = self.step_no

    def look(self):
        self.look_steps.append(self.step_no)
        return list(self.done), [g - 1 for g in self.generated]

    def retire(self, req, slot, n):
        assert self.request[slot] == req
        self.retired_at[req] = (self.step_no, slot, n)
        self.results[req] = [req * 1000 + i for i in range(n)]
        self.request[slot] = None


def run(lengths, slots, period=8):
    sched, rows = SlotScheduler(len(lengths), slots, period), FakeRows(lengths, slots)
    sched.run(rows.admit, rows.step, rows.look, rows.retire)
    return sched, rows


@pytest.mark.parametrize("lengths,slots", [(LENGTHS, 3), (LENGTHS, 16), ([4, 2], 5), (LENGTHS, 1)])
def test_scheduler_serves_every_request_once_and_in_order(lengths, slots):
    sched, rows = run(lengths, slots)
    n = len(lengths)
    assert sorted(rows.admitted_at) == sorted(rows.retired_at) == list(range(n))                   # each exactly once (admit asserts "not twice")
    out = sched.in_request_order(rows.results)
    assert [len(x) for x in out] == lengths and all(x[0] == r * 1000 for r, x in enumerate(out))      # request order, whole answers
    assert sched.lengths == lengths
    st = sched.stats()
    assert st["admits"] == n and st["requests"] == n
    assert st["live_row_steps"] == sum(lengths) - n                                                # token 0 costs no decode step
    assert st["total_row_steps"] == slots * rows.step_no and st["steps"] == rows.step_no
    assert st["looks"] == len(rows.look_steps)
    # no slot holds two requests at once: in every slot the tenancies [admitted, retired] follow each other
    for s in range(slots):
        spans = sorted((rows.admitted_at[r][0], rows.retired_at[r][0], r) for r in range(n) if rows.admitted_at[r][1] == s)
        for (a0, r0, _), (a1, _, _) in zip(spans, spans[1:]):
            assert r0 <= a1
    for r in range(n):
        # retired at the first look at or after the step that finished it
        first_look = min(t for t in rows.look_steps if t >= rows.finished_at[r])
        assert rows.retired_at[r][0] == first_look, r
    # the run ends at the first look after the last row is done
    assert rows.look_steps[-1] == min(t for t in rows.look_steps if t >= max(rows.finished_at.values()))
    assert rows.step_no == rows.look_steps[-1]


def test_a_finished_slot_is_refilled_at_the_first_look_after_it_finishes():
    sched, rows = run(LENGTHS, 3)
    order = sorted(range(len(LENGTHS)), key=lambda r: (rows.admitted_at[r][0], r))
    assert order == sorted(order, key=lambda r: rows.admitted_at[r][0])
    for r in range(3, len(LENGTHS)):                       # everything behind the first three waits for a slot
        when, slot = rows.admitted_at[r]
        freed = [q for q in range(len(LENGTHS)) if rows.retired_at[q][1] == slot and rows.retired_at[q][0] == when]
        assert freed, f"request {r} entered slot {slot} at step {when}, which no look had freed then"
    # pending requests are admitted in their order
    admits = [rows.admitted_at[r][0] for r in range(len(LENGTHS))]
    assert admits == sorted(admits)
    # the host looks every `period` steps, plus one look per batch of admits holding a one-token request
    gaps = {b - a for a, b in zip(rows.look_steps, rows.look_steps[1:])}
    assert gaps <= {0, 8}
    assert sched.looks <= -(-sched.steps // 8) + sched.admits + 1


def test_scheduler_with_no_requests_and_bad_arguments():
    sched, rows = run([], 4)
    assert sched.in_request_order(rows.results) == [] and sched.stats()["steps"] == 0 and sched.stats()["looks"] == 0
    with pytest.raises(ValueError):
        SlotScheduler(3, 0)
    with pytest.raises(ValueError):
        SlotScheduler(-1, 2)
    with pytest.raises(RuntimeError):
        SlotScheduler(2, 2).in_request_order({0: []})


def test_room_shortens_a_run_of_steps():
    """The capacity bound: `room` steps fit before the next look must happen."""
    sched, rows = SlotScheduler(2, 2, 8), FakeRows([20, 20], 2)
    sched.run(rows.admit, rows.step, rows.look, rows.retire, room=lambda: 5)
    assert {b - a for a, b in zip([0] + rows.look_steps, rows.look_steps)} == {5}
    with pytest.raises(RuntimeError):
        sched2, rows2 = SlotScheduler(1, 1, 8), FakeRows([3], 1)
        sched2.run(rows2.admit, rows2.step, rows2.look, rows2.retire, room=lambda: 0)


def _stub():
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: [7])


@pytest.mark.parametrize("kw,value", [("do_sample", True), ("constraint", object()), ("num_beams", 2), ("num_return_sequences", 3),
                                      ("output_logprobs", True), ("past_key_values", object())])
def test_generate_many_refuses_what_it_cannot_schedule(kw, value):
    """Raised by the parser and again through the public entry, before any device work: the requests are never touched."""
    from aki_amd.aki import AKI, _parse_many_kwargs
    with pytest.raises(NotImplementedError, match=kw):
        _parse_many_kwargs({kw: value, "max_new_tokens": 4}, 0, lambda: [])
    with pytest.raises(NotImplementedError, match=kw):
        AKI.generate_many(_stub(), [(None, None)], slots=2, **{kw: value})


def test_generate_many_keywords():
    from aki_amd.aki import AKI, PROCESSOR_KWARGS, _parse_many_kwargs
    for kw in ("no_such_keyword", "top_logprobs", "logits_processor", "temperature"):
        with pytest.raises(ValueError, match=kw):
            _parse_many_kwargs({kw: 1}, 0, lambda: [])
        with pytest.raises(ValueError, match=kw):
            AKI.generate_many(_stub(), [(None, None)], **{kw: 1})
    opt = _parse_many_kwargs(dict(max_new_tokens=5, pad_token_id=3, use_graph=False, do_sample=False, num_beams=1, num_return_sequences=1,
                                  output_logprobs=False, constraint=None, past_key_values=None, repetition_penalty=1.3,
                                  no_repeat_ngram_size=2), 0, lambda: [7])
    assert opt.max_new_tokens == 5 and opt.pad_id == 3 and opt.use_graph is False and opt.eos_ids == {7}
    assert opt.processors["repetition_penalty"] == 1.3 and opt.processors["no_repeat_ngram_size"] == 2
    assert set(opt.processors) == set(PROCESSOR_KWARGS)
    assert _parse_many_kwargs({"eos_token_id": []}, 9, lambda: [7]).eos_ids == set()
    assert _parse_many_kwargs({}, 9, lambda: [7]).use_graph is True
    with pytest.raises(ValueError):
        _parse_many_kwargs({"max_new_tokens": 0}, 0, lambda: [])
    # slots and request shapes are host checks too
    ids = torch.zeros((1, 3), dtype=torch.long)
    for slots in (0, 17):
        with pytest.raises(ValueError, match="slots"):
            AKI.generate_many(_stub(), [(None, ids)], slots=slots)
    for bad in [(None,), (None, ids[0]), (None, ids.int()), (None, ids, 0), (torch.zeros(1, 3), ids), (None, torch.zeros((2, 3), dtype=torch.long))]:
        with pytest.raises(ValueError, match="request 0"):
            AKI.generate_many(_stub(), [bad], slots=2)
    stub = _stub()
    assert AKI.generate_many(stub, [], slots=4) == [] and stub.last_many_stats["requests"] == 0


def test_slot_capacity_is_the_expanded_length_the_splice_produces():
    """The golden tiny batch holds the language stream the reference's splice produced: its length is the longest expanded prompt.  The
    number of vision tokens per image is the model's own constant (PerceiverResampler.num_tokens_per_media)."""
    from aki_amd.helpers import PerceiverResampler
    T = gen.TINY
    n_vis = PerceiverResampler(dim=T["vis_hidden"], dim_inner=T["lm_hidden"], num_latents=T["num_vision_tokens"]).num_tokens_per_media
    assert n_vis == T["num_vision_tokens"]
    g = load_golden("tiny_e2e.npz")
    lx, am = g["lang_x"], g["attention_mask"]
    media = T["media_token_id"]
    prompts = [lx[b, :int(am[b].sum())].tolist() for b in range(lx.shape[0])]
    assert any(media in p for p in prompts)
    for p in prompts:
        assert expanded_length(p, media, n_vis) == len(p) + (n_vis - 1) * p.count(media)
    assert max(expanded_length(p, media, n_vis) for p in prompts) == g["inputs_embeds"].shape[1]
    budgets = [3, 9, 1, 4][:len(prompts)] + [2] * max(0, len(prompts) - 4)
    assert slot_capacity(prompts, budgets, media, n_vis) == max(expanded_length(p, media, n_vis) + b for p, b in zip(prompts, budgets))
    assert expanded_length([5, 6, 7], media, 144) == 3 and expanded_length([5, media, 7, media], media, 144) == 4 + 143 * 2
    assert slot_capacity([], [], media, n_vis) == 0
    with pytest.raises(ValueError):
        slot_capacity(prompts, budgets[:-1], media, n_vis)
