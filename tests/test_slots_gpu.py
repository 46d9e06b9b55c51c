"""In-flight batching on the GPU: ops.kv_slot_admit against torch slice assignment (bit-exact, poison around it), ops.slot_tick against a
torch restatement, and AKI.generate_many end to end on the tiny model - every returned token against the FULL forward over the prompt
extended by the tokens before it (the yardstick of test_generate_matches_full_forward; generate() at another batch size is not one, its
arithmetic differs)."""
import math

import pytest
import torch

from test_model_gpu import build_tiny, batch, DEV
from test_decode_gpu import _tiny_full_width_aki

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


# ---- ops.kv_slot_admit --------------------------------------------------------------------------------------------------------------
FORMATS = {"bf16_192B": (2, 3, 96, torch.bfloat16, "bf16"), "fp32_32B": (2, 3, 8, torch.float32, "bf16"), "bf16_4B": (1, 2, 2, torch.bfloat16, "bf16"),
           "fp8_96B": (2, 3, 96, torch.bfloat16, "fp8_e4m3")}
CASES = [(40, 37, 3, 64, 1), (40, 40, 3, 40, 2), (5, 1, 1, 5, 0), (300, 257, 16, 300, 15)]


def _cache(layers, B, H, Dh, cap, dtype, kv_dtype, seed):
    """An AkiKVCache whose every byte (scales included) is random."""
    from aki_amd.phi3 import AkiKVCache
    c = AkiKVCache(layers, B, H, Dh, cap, dtype, DEV, kv_dtype)
    g = torch.Generator(device=DEV).manual_seed(seed)
    for t_ in c._store:
        if t_ is not None:
            t_.view(torch.uint8).copy_(torch.randint(0, 256, t_.view(torch.uint8).shape, generator=g, device=DEV, dtype=torch.uint8))
    return c


def _tensors(c):
    return list(c.k) + list(c.v) + (list(c.k_scale) + list(c.v_scale) if c.k_scale is not None else [])


def _bytes(t_):
    return t_.contiguous().view(torch.uint8)


def _check_admit(src, dst, slot, n):
    from aki_amd import ops
    want = [t_.clone() for t_ in _tensors(dst)]
    for w, s in zip(want, _tensors(src)):
        w[slot, :, :n] = s[0, :, :n]
    ops.kv_slot_admit(src, dst, slot)
    for i, (got, w) in enumerate(zip(_tensors(dst), want)):
        assert torch.equal(_bytes(got), _bytes(w)), f"tensor {i}: bytes differ from the slice assignment (or a byte outside [slot, :, :len] changed)"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_kv_slot_admit_is_a_slice_assignment(fmt, case):
    layers, H, Dh, dtype, kv = FORMATS[fmt]
    cap_src, n, B, cap_dst, slot = case
    src, dst = _cache(layers, 1, H, Dh, cap_src, dtype, kv, 1), _cache(layers, B, H, Dh, cap_dst, dtype, kv, 2)     # dst: the poison pattern
    src.cache_len.fill_(n)
    src.host_len = n
    _check_admit(src, dst, slot, n)


@pytest.mark.parametrize("fmt", ["bf16_192B", "bf16_4B", "fp32_32B"])
def test_kv_slot_admit_host_bound_above_the_device_length_and_unaligned_destination(fmt):
    """host_len only sizes the grid: the device length decides.  And a destination that is only 4-byte aligned takes the word path."""
    layers, H, Dh, dtype, kv = FORMATS[fmt]
    src, dst = _cache(layers, 1, H, Dh, 40, dtype, kv, 3), _cache(layers, 3, H, Dh, 64, dtype, kv, 4)
    src.cache_len.fill_(23)
    src.host_len = 40
    _check_admit(src, dst, 2, 23)
    off = 4 // dst.k[0].element_size()                          # elements in 4 bytes
    flat = [torch.empty(t_.numel() + 16, dtype=t_.dtype, device=DEV) for t_ in dst.k + dst.v]
    views = [f[off:off + t_.numel()].view(t_.shape).copy_(t_) for f, t_ in zip(flat, dst.k + dst.v)]
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    dst.k, dst.v = views[:layers], views[layers:]
    _check_admit(src, dst, 0, 23)
    guard = [f.clone() for f in flat]
    _check_admit(src, dst, 1, 23)
    for f, g_ in zip(flat, guard):                              # the bytes in front of and behind each view are untouched as well
        assert torch.equal(_bytes(f[:off]), _bytes(g_[:off])) and torch.equal(_bytes(f[off + views[0].numel():]), _bytes(g_[off + views[0].numel():]))


def test_kv_slot_admit_refusals():
    from aki_amd import ops
    from aki_amd.phi3 import AkiKVCache
    mk = lambda layers=2, B=3, H=3, Dh=96, cap=64, dtype=torch.bfloat16, kv="bf16", dev=DEV: AkiKVCache(layers, B, H, Dh, cap, dtype, dev, kv)

    def src(**kw):
        c = mk(B=1, cap=40, **kw)
        c.cache_len.fill_(8)
        c.host_len = 8
        return c

    ops.kv_slot_admit(src(), mk(), 0)                          # the well-formed call
    bad = []
    for slot in (-1, 3):
        bad.append((src(), mk(), slot))                        # slot outside [0, B)
    bad.append((src(layers=1), mk(), 0))                       # layers
    bad.append((src(H=2), mk(), 0))                            # heads
    bad.append((src(Dh=48), mk(), 0))                          # head_dim
    bad.append((src(dtype=torch.float32), mk(), 0))            # element format
    bad.append((src(kv="fp8_e4m3"), mk(), 0))                  # kv_dtype: nothing is converted
    bad.append((src(), mk(kv="fp8_e4m3"), 0))
    s = src()
    s.host_len = 40
    bad.append((s, mk(cap=32), 0))                             # cap_dst < the source's host_len
    s = src()
    s.host_len = 41
    bad.append((s, mk(), 0))                                   # a host_len the source cannot hold
    bad.append((mk(B=2, cap=40), mk(), 0))                     # a source of two sequences
    s = src()
    s.k = [t_.transpose(1, 2) for t_ in s.k]
    bad.append((s, mk(), 0))                                   # not contiguous
    d = mk()
    d.v = [t_[:, :, ::2] for t_ in d.v]
    bad.append((src(), d, 0))
    d = mk()
    d.group = 2
    bad.append((src(), d, 0))                                  # grouped (share_prefix)
    s = src()
    s.group = 2
    bad.append((s, mk(), 0))
    bad.append((src(dev="cpu"), mk(), 0))                      # devices
    bad.append((src(), mk(dev="cpu"), 0))
    bad.append((src(Dh=1), mk(Dh=1), 0))                       # 2-byte rows: no multiple of 4
    for i, (s, d, slot) in enumerate(bad):
        with pytest.raises(ops.AkiError):
            ops.kv_slot_admit(s, d, slot)
            pytest.fail(f"refusal {i} went through")


# ---- ops.slot_tick ------------------------------------------------------------------------------------------------------------------
def _tick_reference(done, done_at, cache_len, start_len, limit):
    done, done_at, cache_len = done.clone(), done_at.clone(), cache_len.clone()
    generated = cache_len - start_len + 1
    hit = (done == 0) & (generated >= limit)
    done_at = torch.where(hit, generated - 1, done_at)
    done = torch.where(hit, torch.ones_like(done), done)
    cache_len = torch.where((done != 0) & (done_at >= 0), start_len + done_at, cache_len)
    return done, done_at, cache_len


@pytest.mark.parametrize("B", [1, 5, 16])
def test_slot_tick_matches_the_torch_restatement(B):
    from aki_amd import ops
    g = torch.Generator(device="cpu").manual_seed(B)
    kinds = ["under", "at", "over", "done", "done_at_0", "limit_1"]
    for rep in range(6):
        start = torch.randint(1, 700, (B,), generator=g, dtype=torch.int32)
        limit = torch.randint(2, 256, (B,), generator=g, dtype=torch.int32)
        gen_ = torch.zeros(B, dtype=torch.int32)
        done = torch.zeros(B, dtype=torch.uint8)
        done_at = torch.full((B,), -1, dtype=torch.int32)
        for b in range(B):
            kind = kinds[(b + rep) % len(kinds)]               # every kind at every B (at B = 1 over the repetitions)
            lim = int(limit[b])
            if kind == "under":
                gen_[b] = int(torch.randint(1, lim, (1,), generator=g))
            elif kind == "at":
                gen_[b] = lim
            elif kind == "over":
                gen_[b] = lim + int(torch.randint(1, 9, (1,), generator=g))
            elif kind == "done":                               # finished earlier, stepped on with a pad token since
                done[b] = 1
                done_at[b] = int(torch.randint(0, lim, (1,), generator=g))
                gen_[b] = int(done_at[b]) + 2
            elif kind == "done_at_0":
                done[b], done_at[b], gen_[b] = 1, 0, 2
            else:
                limit[b], gen_[b] = 1, 1                       # token 0 is the whole budget
        cache_len = start + gen_ - 1
        dev = [x.to(DEV) for x in (done, done_at, cache_len, start, limit)]
        want = _tick_reference(*dev)
        keep = [dev[3].clone(), dev[4].clone()]
        ops.slot_tick(*dev)
        for name, got, w in zip(("done", "done_at", "cache_len"), dev[:3], want):
            assert torch.equal(got, w), (name, rep, got.tolist(), w.tolist())
        assert torch.equal(dev[3], keep[0]) and torch.equal(dev[4], keep[1])
        # the invariants: a done row never sits above start + done_at, a row at or over its budget is done
        assert bool(((dev[0] == 0) | (dev[2] == dev[3] + dev[1])).all())
        assert bool(((dev[2] - dev[3] + 1 < dev[4]) | (dev[0] == 1)).all())


def test_slot_tick_refusals():
    from aki_amd import ops
    mk = lambda n: [torch.zeros(n, dtype=torch.uint8, device=DEV)] + [torch.ones(n, dtype=torch.int32, device=DEV) for _ in range(4)]
    ops.slot_tick(*mk(16))
    with pytest.raises(ops.AkiError):
        ops.slot_tick(*mk(17))                                  # more rows than one tick takes
    a = mk(4)
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a[0], a[1].long(), a[2], a[3], a[4])
    with pytest.raises(ops.AkiError):
        ops.slot_tick(a[0], a[1], a[2][:3], a[3], a[4])
    with pytest.raises(ops.AkiError):
        ops.slot_tick(*[x.cpu() for x in a])


# ---- generate_many on the tiny model --------------------------------------------------------------------------------------------------
BUDGETS = [12, 1, 5, 12, 3, 9, 12]
_MODELS = {}


def tiny(dtype):
    """(model, requests without budgets) - built once per dtype.  Seven prompts of different expanded lengths: golden rows with an <image>,
    row 2 without one (its image is handed over and never spliced), extended rows, and one text-only request (vision_x None)."""
    if dtype not in _MODELS:
        m, g = build_tiny(dtype)
        vx, lx, am, _ = batch(g, dtype)
        real = [lx[b:b + 1, :int(am[b].sum())] for b in range(lx.shape[0])]
        extra = lambda *ids: torch.tensor([ids], dtype=torch.long, device=DEV)
        reqs = [(vx[0:1], real[0]), (vx[1:2], real[1]), (vx[2:3], real[2]), (vx[3:4], real[3]),
                (vx[0:1], torch.cat([real[0], extra(50, 51)], dim=1)),
                (None, extra(1, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39)),
                (vx[1:2], torch.cat([real[1], extra(60, 61, 62)], dim=1))]
        _MODELS[dtype] = (m, reqs)
    return _MODELS[dtype]


def generate_alone(m, vx, lx, **kw):
    """generate() for one request, 1-D.  generate() itself prefills image prompts only: the text-only request is continued from a cache of
    its first T - 1 ids, the form generate() takes for it."""
    if vx is not None:
        return m.generate(vx, lx, **kw)[0]
    cache = m.lang_model(input_ids=lx[:, :-1], use_cache=True, cache_capacity=lx.shape[1] + 32, last_token_logits=True).past_key_values
    return m.generate(None, lx[:, -1:], past_key_values=cache, **kw)[0]


_REFS = {}


def references(dtype):
    """Per dtype, computed once: (eos id, per-request generate() tokens with that EOS and the request's budget, cut behind the EOS).  The EOS
    is the id request 0 emits at step 3 of an EOS-free run, so it fires in the middle of a period of 8 while other slots are mid-sequence."""
    if dtype not in _REFS:
        m, reqs = tiny(dtype)
        free = generate_alone(m, *reqs[0], max_new_tokens=BUDGETS[0], eos_token_id=[])
        eos = int(free[3])
        alone = []
        for (vx, lx), budget in zip(reqs, BUDGETS):
            row = generate_alone(m, vx, lx, max_new_tokens=budget, eos_token_id=[eos]).tolist()
            alone.append(row[:row.index(eos) + 1] if eos in row else row)
        _REFS[dtype] = (eos, alone)
    return _REFS[dtype]


def with_budgets(reqs, budgets=BUDGETS):
    return [(vx, lx, b) for (vx, lx), b in zip(reqs, budgets)]


def check_structure(outs, budgets, eos):
    assert len(outs) == len(budgets)
    for r, (o, budget) in enumerate(zip(outs, budgets)):
        assert o.dim() == 1 and o.dtype == torch.long and o.is_cuda, r
        row = o.tolist()
        assert 1 <= len(row) <= budget, (r, len(row), budget)
        assert eos not in row[:-1], f"request {r}: an EOS inside the sequence {row}"
        assert len(row) == budget or row[-1] == eos, f"request {r}: {len(row)} of {budget} tokens without an EOS at the end"


def check_against_full_forward(m, reqs, outs, dtype):
    """Teacher-force every returned sequence through the full forward: fp32 - every token is its argmax; bf16 - within
    0.05 * max(1, max|logits|) of the best logit (the bar of test_generate_matches_full_forward, for its reason: a near-tie may flip)."""
    for r, ((vx, lx), o) in enumerate(zip(reqs, outs)):
        ids = lx[0]
        for step, tok in enumerate(o.tolist()):
            with torch.no_grad():
                full = m(vx, ids[None], attention_mask=torch.ones_like(ids)[None]).logits[0, -1].float()
            best = int(full.argmax())
            if dtype == torch.float32:
                assert tok == best, f"request {r} step {step}: generate_many chose {tok}, the full forward {best}"
            else:
                assert float(full[best] - full[tok]) <= 0.05 * max(1.0, float(full.abs().max())), (r, step, tok, best)
            ids = torch.cat([ids, o[step:step + 1]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_generate_many_matches_the_full_forward(dtype):
    m, reqs = tiny(dtype)
    eos, alone = references(dtype)
    assert eos in alone[0] and len(alone[0]) == 4, "the EOS was chosen to end request 0 at step 3"
    outs = m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[eos])
    check_structure(outs, BUDGETS, eos)
    assert len(outs[1]) == 1                                    # the budget of one token
    assert len(outs[0]) == 4 and int(outs[0][-1]) == eos        # an EOS in the middle of a period
    st = m.last_many_stats
    assert st["admits"] == 7 and st["slots"] == 3 and st["requests"] == 7
    assert st["live_row_steps"] == sum(len(o) for o in outs) - 7 and st["total_row_steps"] == 3 * st["steps"]
    check_against_full_forward(m, reqs, outs, dtype)
    if dtype == torch.float32:
        assert [o.tolist() for o in outs] == alone


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_generate_many_does_not_depend_on_the_schedule(dtype):
    """The same requests in reversed order, and over 2 slots instead of 3.  fp32: identical per request.  bf16: identical for the reversed
    order - the same batch size, so it holds when every decode kernel computes a row independently of its neighbours and its row index;
    another slot count is another batch size, whose GEMMs may round differently: those sequences are held to the full-forward bar."""
    m, reqs = tiny(dtype)
    eos, _ = references(dtype)
    base = [o.tolist() for o in m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[eos])]
    rev = m.generate_many(with_budgets(reqs)[::-1], slots=3, eos_token_id=[eos])[::-1]
    assert [o.tolist() for o in rev] == base
    two = m.generate_many(with_budgets(reqs), slots=2, eos_token_id=[eos])
    check_structure(two, BUDGETS, eos)
    if dtype == torch.float32:
        assert [o.tolist() for o in two] == base
    else:
        check_against_full_forward(m, reqs, two, dtype)
    # eager steps size the attention grid by the rows in use, the captured step by the capacity: the same tokens in fp32, the bar in bf16
    eager = m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[eos], use_graph=False)
    check_structure(eager, BUDGETS, eos)
    if dtype == torch.float32:
        assert [o.tolist() for o in eager] == base
    else:
        check_against_full_forward(m, reqs, eager, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_generate_many_captures_once_and_never_syncs_per_token(dtype, monkeypatch):
    from aki_amd.phi3 import DecodeGraph
    m, reqs = tiny(dtype)
    eos, _ = references(dtype)
    captures = []
    real = DecodeGraph._capture
    monkeypatch.setattr(DecodeGraph, "_capture", lambda self: (captures.append(1), real(self))[1])
    m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[eos])
    st = m.last_many_stats
    assert len(captures) == 1
    assert st["steps"] > 8 and st["looks"] <= math.ceil(st["steps"] / 8) + st["admits"] + 1, st


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_admit_does_not_disturb_a_neighbour(dtype, monkeypatch):
    """Slot 0 holds request 0 for the whole run while slot 1 is refilled three times; in a second run nothing is refilled.  The K/V rows slot 0
    wrote are bit-identical in both."""
    from aki_amd import ops
    m, reqs = tiny(dtype)
    seen = []
    real = ops.kv_slot_admit
    monkeypatch.setattr(ops, "kv_slot_admit", lambda s, d, slot: (seen.append((d, slot)), real(s, d, slot))[1])

    def slot0(requests, budgets):
        del seen[:]
        outs = m.generate_many(with_budgets(requests, budgets), slots=2, eos_token_id=[])
        cache = seen[0][0]
        assert all(d is cache for d, _ in seen)
        n = int(cache.cache_len[0])
        return outs, [s for _, s in seen], n, [t_[0, :, :n].clone() for t_ in cache.k + cache.v]

    outs_a, slots_a, n_a, kv_a = slot0([reqs[0], reqs[1], reqs[3], reqs[6], reqs[2]], [30, 9, 9, 9, 2])
    outs_b, slots_b, n_b, kv_b = slot0([reqs[0], reqs[1]], [30, 30])
    assert slots_a == [0, 1, 1, 1, 1] and slots_b == [0, 1]
    assert n_a == n_b == 25 + 30 - 1                            # parked on the row of the token it never fed
    assert outs_a[0].tolist() == outs_b[0].tolist()
    for i, (a, b) in enumerate(zip(kv_a, kv_b)):
        assert torch.equal(_bytes(a), _bytes(b)), f"cache tensor {i} of slot 0 differs between the runs"


def test_generate_many_processors_start_a_refilled_row_with_an_empty_history():
    m, reqs = tiny(torch.float32)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    alone = [generate_alone(m, vx, lx, max_new_tokens=b, eos_token_id=[], **kw).tolist() for (vx, lx), b in zip(reqs, BUDGETS)]
    plain = [generate_alone(m, vx, lx, max_new_tokens=b, eos_token_id=[]).tolist() for (vx, lx), b in zip(reqs, BUDGETS)]
    assert alone != plain, "the processors change nothing on these prompts: the test would show nothing"
    outs = m.generate_many(with_budgets(reqs), slots=3, eos_token_id=[], **kw)
    assert [o.tolist() for o in outs] == alone
    m16, reqs16 = tiny(torch.bfloat16)                          # the processed pick kernel, inside the captured step
    outs16 = m16.generate_many(with_budgets(reqs16), slots=3, eos_token_id=[], **kw)
    check_structure(outs16, BUDGETS, -1)
    for o in outs16:                                            # no_repeat_ngram_size = 2: no bigram twice
        row = o.tolist()
        grams = list(zip(row, row[1:]))
        assert len(grams) == len(set(grams))


def test_generate_many_falls_back_to_generate_for_one_slot_or_one_request():
    m, reqs = tiny(torch.float32)
    eos, alone = references(torch.float32)
    outs = m.generate_many(with_budgets(reqs), slots=1, eos_token_id=[eos])
    assert [o.tolist() for o in outs] == alone and m.last_many_stats["per_request_generate"]
    outs = m.generate_many(with_budgets(reqs)[3:4], slots=8, eos_token_id=[eos])
    assert [o.tolist() for o in outs] == alone[3:4]


def test_generate_many_on_an_fp8_kv_cache():
    """The full-width tiny model (head_dim 96) with an fp8_e4m3 KV cache, 4 requests over 2 slots: the batch-1 prefill yields an fp8 cache, admit
    copies its bytes and scales.  Tokens against per-request generate() on the fp8 cache: equal up to the first near-tie - two tokens there
    must both be within the bf16 full-forward bar - and every returned token is within that bar of the full forward's best."""
    m, vx, ids, _ = _tiny_full_width_aki()
    m.lang_model.set_kv_cache_dtype("fp8_e4m3")
    g = torch.Generator(device="cpu").manual_seed(9)
    tail = lambda n: torch.randint(3, 32000, (1, n), generator=g).to(DEV)
    reqs = [(vx, ids), (vx, torch.cat([ids, tail(5)], dim=1)), (vx, torch.cat([ids, tail(9)], dim=1)), (vx, torch.cat([ids, tail(2)], dim=1))]
    budgets = [10, 1, 4, 10]
    free = m.generate(vx, ids, max_new_tokens=10, eos_token_id=[])[0]
    eos = int(free[3])
    alone = []
    for (v, l), b in zip(reqs, budgets):
        row = m.generate(v, l, max_new_tokens=b, eos_token_id=[eos])[0].tolist()
        alone.append(row[:row.index(eos) + 1] if eos in row else row)
    outs = m.generate_many(with_budgets(reqs, budgets), slots=2, eos_token_id=[eos])
    check_structure(outs, budgets, eos)
    assert len(outs[1]) == 1
    check_against_full_forward(m, reqs, outs, torch.bfloat16)
    for r, ((v, l), o, a) in enumerate(zip(reqs, outs, alone)):
        row = o.tolist()
        fork = next((i for i, (x, y) in enumerate(zip(row, a)) if x != y), None)
        if fork is None:
            assert len(row) == len(a), (r, row, a)
            continue
        ctx = torch.cat([l[0], o[:fork]])
        with torch.no_grad():
            full = m(v, ctx[None], attention_mask=torch.ones_like(ctx)[None]).logits[0, -1].float()
        assert abs(float(full[row[fork]] - full[a[fork]])) <= 0.05 * max(1.0, float(full.abs().max())), (r, fork, row, a)
