"""pick_stage.PickStage on CPU tensors, the six ops launches behind it replaced by recorders: which launches each of the six sites of
generate / generate_many issues, in which order and with which keywords, for every feature on and off; and what row(slot) hands on."""
import itertools

import pytest
import torch

from aki_amd import ops
from aki_amd.phi3 import DecodeGraph
from aki_amd.pick_stage import PickStage
from aki_amd.stops import check_stop_sequences

B, V, STEPS, D = 3, 16, 4, 8
OPS = ("greedy_pick", "sample_pick", "sample_pick_rows", "token_logprob", "stop_check", "slot_tick")
PARENT_KEYS = ("done", "tokens", "start_len", "done_at")


@pytest.fixture
def calls(monkeypatch):
    """[(name, args, kwargs)] of every launch, in order."""
    seen = []
    for name in OPS:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: seen.append((_n, a, k)))
    return seen


def buffers():
    return dict(pad_token_id=0, eos_ids=torch.tensor([2]), done=torch.zeros(B, dtype=torch.uint8),
                tokens=torch.zeros((B, STEPS), dtype=torch.long), start_len=torch.zeros(B, dtype=torch.int32),
                done_at=torch.full((B,), -1, dtype=torch.int32))


def make(sampler="none", logprob=False, stops=False, tick=False, embed=False, processors=False):
    pick = buffers()
    kw = {}
    if processors:
        pick["processors"] = ops.LogitsProcessors(V, "cpu", repetition_penalty=1.3)
        kw["processors_row"] = ops.LogitsProcessors(V, "cpu", repetition_penalty=1.3)
    if sampler == "scalar":
        kw["sampler"] = dict(temperature=0.7, top_k=5, top_p=0.9, seed=11, offset=0)
    if sampler == "rows":
        kw["rows"] = dict(temperature=torch.ones(B), top_k=torch.ones(B, dtype=torch.int32), top_p=torch.ones(B),
                          seed=torch.arange(B, dtype=torch.int64))
    if logprob:
        kw["logprob"] = dict(top_k=2, out_logprob=torch.zeros((B, STEPS)), out_top_ids=torch.zeros((B, STEPS, 2), dtype=torch.long),
                             out_top_logprobs=torch.zeros((B, STEPS, 2)))
    if stops:
        kw["stops"] = ops.StopSets("cpu", [check_stop_sequences("test", [[5]])], B)
    if tick:
        kw["limit"] = torch.full((B,), STEPS, dtype=torch.int32)
    if embed:
        kw["embed"], kw["next_embeds"] = (torch.zeros((V, D), dtype=torch.bfloat16), None, V - 1), torch.zeros((B, D), dtype=torch.bfloat16)
    return PickStage(pick, **kw)


def run_args():
    return torch.zeros((B, V), dtype=torch.bfloat16), torch.zeros(B, dtype=torch.long), torch.zeros(B, dtype=torch.int32)


PICK_OF = {"none": "greedy_pick", "scalar": "sample_pick", "rows": "sample_pick_rows"}


def expected_names(sampler, logprob, stops, tick, fuse_stops=True):
    names = [PICK_OF[sampler]]
    if logprob:
        names.append("token_logprob")
    if stops and not (tick and fuse_stops):
        names.append("stop_check")
    if tick:
        names.append("slot_tick")
    return names


# ---- generate: token 0 and the eager step carry the embedding gather, the captured step does not; no tick ever
@pytest.mark.parametrize("sampler,logprob,stops", list(itertools.product(("none", "scalar"), (False, True), (False, True))))
@pytest.mark.parametrize("site", ("token0", "eager", "captured"))
def test_generate_sites(calls, site, sampler, logprob, stops):
    stage = make(sampler, logprob, stops, embed=True)
    logits, ids, cache_len = run_args()
    advance, gather = {"token0": (False, True), "eager": (True, True), "captured": (True, False)}[site]
    stage.run(logits, ids, cache_len, advance=advance, embed=gather)
    assert [c[0] for c in calls] == expected_names(sampler, logprob, stops, False)
    name, args, kw = calls[0]
    assert args[0] is logits and args[1] is ids and kw["cache_len"] is cache_len and kw["advance"] is advance
    assert ("embed" in kw) == gather and ("next_embeds" in kw) == gather
    assert ("seed" in kw) == (sampler == "scalar") and "processors" not in kw
    assert args[0].shape[0] == B and kw["tokens"].shape[0] == B
    if logprob:
        _, a, k = calls[1]
        assert a[0] is logits and k["cache_len"] is cache_len and k["tokens"] is stage.tokens and k["top_k"] == 2 and k["out_logprob"].shape[0] == B
    if stops:
        _, a, k = calls[-1]
        assert a[0] is stage.tokens and a[1] is cache_len and a[2] is stage.start_len and a[3] is stage.done and a[4] is stage.done_at
        assert a[5] is stage.stops and not k


# ---- generate_many's step, eager and captured alike: the stops ride in the tick
@pytest.mark.parametrize("sampler,logprob,stops", list(itertools.product(("none", "rows"), (False, True), (False, True))))
@pytest.mark.parametrize("gather", (True, False))
def test_many_step(calls, gather, sampler, logprob, stops):
    stage = make(sampler, logprob, stops, tick=True)
    logits, ids, cache_len = run_args()
    stage.run(logits, ids, cache_len, advance=True, embed=gather)
    assert [c[0] for c in calls] == expected_names(sampler, logprob, stops, True)
    _, args, kw = calls[0]
    assert kw["advance"] is True and "embed" not in kw and args[0].shape[0] == B
    if sampler == "rows":
        assert all(kw[k] is stage.rows[k] for k in ("temperature", "top_k", "top_p", "seed"))
    _, a, k = calls[-1]
    assert not a and k["cache_len"] is cache_len and k["limit"] is stage.limit and k["done"] is stage.done and k["done_at"] is stage.done_at
    assert k["start_len"] is stage.start_len
    assert (k.get("stops") is stage.stops and k.get("tokens") is stage.tokens) if stops else ("stops" not in k and "tokens" not in k)


# ---- generate_many's admit: row(1), advance=False, the stop check a launch of its own AHEAD of a tick without stops
@pytest.mark.parametrize("sampler,logprob,stops", list(itertools.product(("none", "rows"), (False, True), (False, True))))
def test_many_admit_row_views(calls, sampler, logprob, stops):
    stage = make(sampler, logprob, stops, tick=True, processors=True)
    logits, ids, cache_len = run_args()
    one = stage.row(1)
    one.run(logits[1:2], ids[1:2], cache_len[1:2], advance=False, fuse_stops=False)
    assert [c[0] for c in calls] == expected_names(sampler, logprob, stops, True, fuse_stops=False)

    def is_row1(view, parent):
        return view.shape[0] == 1 and view.shape[1:] == parent.shape[1:] and view.data_ptr() == parent[1].data_ptr()

    _, args, kw = calls[0]
    assert kw["advance"] is False and args[0].shape[0] == 1 and args[1].data_ptr() == ids[1:2].data_ptr()
    assert is_row1(kw["cache_len"], cache_len)
    assert all(is_row1(kw[k], stage.pick[k]) for k in PARENT_KEYS)
    assert kw["eos_ids"] is stage.pick["eos_ids"]                      # shared by every row: not a row view
    assert kw["processors"] is stage.processors_row and kw["processors"] is not stage.pick["processors"]
    if sampler == "rows":
        assert all(is_row1(kw[k], stage.rows[k]) for k in ("temperature", "top_k", "top_p", "seed"))
    if logprob:
        _, a, k = calls[1]
        assert a[0].shape[0] == 1 and k["top_k"] == 2 and is_row1(k["cache_len"], cache_len)
        assert all(is_row1(k[n], stage.logprob[n]) for n in ("out_logprob", "out_top_ids", "out_top_logprobs"))
        assert all(is_row1(k[n], stage.pick[n]) for n in ("tokens", "start_len", "done_at"))
    if stops:
        _, a, k = calls[-2]
        assert all(is_row1(v, p) for v, p in zip(a[:5], (stage.tokens, cache_len, stage.start_len, stage.done, stage.done_at)))
        assert is_row1(a[5].row_set, stage.stops.row_set) and is_row1(a[5].stop_hit, stage.stops.stop_hit) and a[5].ids is stage.stops.ids
    _, a, k = calls[-1]
    assert "stops" not in k and "tokens" not in k and not a
    assert is_row1(k["limit"], stage.limit) and is_row1(k["cache_len"], cache_len)
    assert all(is_row1(k[n], stage.pick[n]) for n in ("done", "done_at", "start_len"))


def test_row_views_of_the_slot_objects(calls):
    pick = buffers()
    pick["processor_sets"] = ops.ProcessorSets(V, "cpu", [2], [], B)
    pick["slot_constraints"] = ops.SlotConstraints(torch.zeros((2, V), dtype=torch.int16), B, STEPS)
    stage = PickStage(pick, limit=torch.ones(B, dtype=torch.int32))
    logits, ids, cache_len = run_args()
    stage.row(1).run(logits[1:2], ids[1:2], cache_len[1:2], advance=False, fuse_stops=False)
    _, _, kw = calls[0]
    sets, con = kw["processor_sets"], kw["slot_constraints"]
    assert sets.row_set.shape == (1,) and sets.row_set.data_ptr() == pick["processor_sets"].row_set[1:2].data_ptr()
    assert sets.sets is pick["processor_sets"].sets and "processors" not in kw
    for name in ("row_base", "row_states", "states"):
        view, parent = getattr(con, name), getattr(pick["slot_constraints"], name)
        assert view.shape[0] == 1 and view.data_ptr() == parent[1:2].data_ptr()
    assert con.pool is pick["slot_constraints"].pool


# ---- the f32 path of generate_many: the pick is torch's, the launches behind it are the same
def test_torch_pick_runs_the_same_tail(calls):
    pick = buffers()
    stage = PickStage(pick, logprob=dict(top_k=0, out_logprob=torch.zeros((B, STEPS)), out_top_ids=None, out_top_logprobs=None),
                      limit=torch.full((B,), STEPS, dtype=torch.int32), torch_pick=True)
    logits = torch.zeros((B, V))
    logits[0, 3], logits[1, 2], logits[2, 7] = 1.0, 1.0, 1.0
    ids, cache_len = torch.zeros(B, dtype=torch.long), torch.zeros(B, dtype=torch.int32)
    stage.run(logits, ids, cache_len, advance=True)
    assert [c[0] for c in calls] == ["token_logprob", "slot_tick"]
    assert ids.tolist() == [3, 2, 7] and pick["tokens"][:, 0].tolist() == [3, 2, 7]
    assert pick["done"].tolist() == [0, 1, 0] and pick["done_at"].tolist() == [-1, 0, -1]      # id 2 is the eos
    calls.clear()
    stage.row(2).run(logits[2:3], ids[2:3], cache_len[2:3], advance=False, fuse_stops=False)
    assert [c[0] for c in calls] == ["token_logprob", "slot_tick"] and calls[0][1][0].shape[0] == 1


def test_decode_graph_wraps_a_plain_dict_into_a_greedy_only_stage(calls):
    class Cache:
        cache_len = torch.zeros(B, dtype=torch.int32)

    pick = dict(pad_token_id=0, eos_ids=None, done=None, tokens=torch.zeros((B, STEPS), dtype=torch.long),
                start_len=torch.zeros(B, dtype=torch.int32), done_at=None)
    graph = DecodeGraph(None, Cache(), greedy=pick)
    stage = graph.greedy
    assert isinstance(stage, PickStage) and not stage.sampling
    assert stage.logprob is None and stage.stops is None and stage.limit is None and stage.embed is None and not stage.torch_pick
    logits, ids, cache_len = run_args()
    stage.run(logits, ids, cache_len, advance=True, embed=False)
    assert [c[0] for c in calls] == ["greedy_pick"]
    want = dict(pick, cache_len=cache_len, advance=True)
    assert calls[0][2].keys() == want.keys() and all(calls[0][2][k] is v for k, v in want.items())
    given = make("rows", tick=True)
    assert DecodeGraph(None, Cache(), greedy=given).greedy is given and DecodeGraph(None, Cache()).greedy is None
