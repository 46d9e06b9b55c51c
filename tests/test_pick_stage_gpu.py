"""pick_stage.PickStage on the GPU, at the smallest shapes at which a row view can go wrong: what row(1).run leaves in row 1 is, bit for
bit, what the same launches issued by hand through ops.* leave on a fresh B = 1 copy, with rows 0 and 2 of every buffer untouched; and the
full-batch run is the hand-issued sequence on cloned buffers.  Both sides run the same kernels on the same inputs: no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, V, BUDGET, EOS, STOP, TOP = 3, 64, 4, 3, 9, 2
HISTORY = (1, 2, 3)            # tokens each row has generated already: the processors' history is not empty, row 2 picks its last token


class State:
    """The buffers of one generation over B rows, pre-filled: live rows with a history (their own most likely columns, so the repetition
    penalty bites), sentinels everywhere a launch on another row must not write."""

    def __init__(self, advance: bool, sampled: bool, rows=slice(0, B)):
        from aki_amd import ops
        from aki_amd.stops import check_stop_sequences
        g = torch.Generator().manual_seed(5)
        logits = torch.randn((B, V), generator=g)
        logits[:, EOS] = logits[:, STOP] = -4.0                 # the other rows pick neither
        logits[1, STOP] = 20.0                                  # row 1 picks the stop token, whatever the sampler draws
        tokens = torch.full((B, BUDGET), -7, dtype=torch.long)
        for b, h in enumerate(HISTORY):
            tokens[b, :h] = logits[b].topk(h + 1).indices[1 if b == 1 else 0:][:h]
        start = torch.tensor([10, 20, 30], dtype=torch.int32)
        n = rows.stop - rows.start
        cut = lambda t: t[rows].clone().to(DEV)
        self.logits = cut(logits.to(torch.bfloat16))
        self.tokens, self.start_len = cut(tokens), cut(start)
        self.cache_len = cut(start + torch.tensor(HISTORY, dtype=torch.int32) - (1 if advance else 0))
        self.ids = cut(torch.tensor([-3, -4, -5]))
        self.done = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.done_at = cut(torch.tensor([-1, -1, -1], dtype=torch.int32))
        self.limit = torch.full((n,), BUDGET, dtype=torch.int32, device=DEV)
        self.eos = torch.tensor([EOS], dtype=torch.long, device=DEV)
        self.lp = dict(top_k=TOP, out_logprob=torch.full((n, BUDGET), 123.0, device=DEV),
                       out_top_ids=torch.full((n, BUDGET, TOP), -5, dtype=torch.long, device=DEV),
                       out_top_logprobs=torch.full((n, BUDGET, TOP), 321.0, device=DEV))
        key = check_stop_sequences("test", [[STOP]])
        self.stops = ops.StopSets(DEV, [key], n)
        self.stops.row_set.fill_(self.stops.index[key])
        self.stops.stop_hit.copy_(cut(torch.tensor([55, 56, 57], dtype=torch.int32)))
        self.proc = ops.LogitsProcessors(V, DEV, repetition_penalty=1.3, eos_ids=[EOS])
        self.rows = None
        if sampled:
            self.rows = dict(temperature=torch.full((n,), 0.7, device=DEV), top_k=torch.full((n,), 5, dtype=torch.int32, device=DEV),
                             top_p=torch.full((n,), 0.9, device=DEV), seed=cut(torch.tensor([11, 12, 13])))
        self.pick = dict(pad_token_id=0, eos_ids=self.eos, done=self.done, tokens=self.tokens, start_len=self.start_len, done_at=self.done_at,
                         processors=self.proc)

    def stage(self):
        from aki_amd import ops
        from aki_amd.pick_stage import PickStage
        return PickStage(self.pick, rows=self.rows, processors_row=ops.LogitsProcessors(V, DEV, repetition_penalty=1.3, eos_ids=[EOS]),
                         logprob=self.lp, stops=self.stops, limit=self.limit)

    def by_hand(self, advance: bool, fuse_stops: bool):
        """The launches of one site, written out."""
        from aki_amd import ops
        if self.rows is not None:
            ops.sample_pick_rows(self.logits, self.ids, cache_len=self.cache_len, advance=advance, **self.rows, **self.pick)
        else:
            ops.greedy_pick(self.logits, self.ids, cache_len=self.cache_len, advance=advance, **self.pick)
        ops.token_logprob(self.logits, tokens=self.tokens, cache_len=self.cache_len, start_len=self.start_len, done_at=self.done_at, **self.lp)
        if fuse_stops:
            ops.slot_tick(self.done, self.done_at, self.cache_len, self.start_len, self.limit, stops=self.stops, tokens=self.tokens)
        else:
            ops.stop_check(self.tokens, self.cache_len, self.start_len, self.done, self.done_at, self.stops)
            ops.slot_tick(self.done, self.done_at, self.cache_len, self.start_len, self.limit)

    def buffers(self):
        out = dict(tokens=self.tokens, done=self.done, done_at=self.done_at, cache_len=self.cache_len, ids=self.ids, start_len=self.start_len,
                   limit=self.limit, stop_hit=self.stops.stop_hit, row_set=self.stops.row_set, lp=self.lp["out_logprob"],
                   top_ids=self.lp["out_top_ids"], top_lp=self.lp["out_top_logprobs"])
        return {k: v.clone() for k, v in out.items()}


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


@pytest.mark.parametrize("sampled", (False, True), ids=("greedy", "rows-sampler"))
def test_row_view_run_is_the_hand_issued_b1_run(sampled):
    full = State(advance=False, sampled=sampled)
    before = full.buffers()
    full.stage().row(1).run(full.logits[1:2], full.ids[1:2], full.cache_len[1:2], advance=False, fuse_stops=False)
    one = State(advance=False, sampled=sampled, rows=slice(1, 2))      # a fresh B = 1 copy of row 1
    one.by_hand(advance=False, fuse_stops=False)
    torch.cuda.synchronize()
    after, want = full.buffers(), one.buffers()
    for name in after:
        for b in (0, 2):
            assert same_bits(after[name][b], before[name][b]), f"{name}: row {b} was touched"
        assert same_bits(after[name][1:2], want[name]), f"{name}: row 1 differs from the hand-issued run"
    # the run did something: row 1 picked the stop token at index HISTORY[1], was scored there and ended by its stop set
    t = HISTORY[1]
    assert int(after["ids"][1]) == STOP and int(after["tokens"][1, t]) == STOP and int(after["done"][1]) == 1 and int(after["done_at"][1]) == t
    assert int(after["stop_hit"][1]) == 0 and float(after["lp"][1, t]) != 123.0 and int(after["top_ids"][1, t, 0]) == STOP


@pytest.mark.parametrize("sampled", (False, True), ids=("greedy", "rows-sampler"))
def test_full_batch_run_is_the_hand_issued_sequence(sampled):
    got, want = State(advance=True, sampled=sampled), State(advance=True, sampled=sampled)
    got.stage().run(got.logits, got.ids, got.cache_len, advance=True)
    want.by_hand(advance=True, fuse_stops=True)
    torch.cuda.synchronize()
    after, ref = got.buffers(), want.buffers()
    for name in after:
        assert same_bits(after[name], ref[name]), f"{name} differs from the hand-issued run"
    assert after["cache_len"].tolist()[0] == 10 + HISTORY[0]            # a live row advanced
    assert after["done"].tolist() == [0, 1, 1] and after["done_at"].tolist() == [-1, HISTORY[1], BUDGET - 1]   # the stop; the budget
    assert after["stop_hit"].tolist() == [55, 0, 57]
