"""Logits processors on the device (ops.LogitsProcessors, aki_logits_process, aki_greedy_pick_processed) against the installed
transformers' processors, and AKI.generate honouring repetition_penalty / no_repeat_ngram_size / bad_words_ids / min_new_tokens /
suppress_tokens in its greedy (eager, graph, chain), sampling and beam-search modes."""
import numpy as np
import pytest
import torch

from test_decode_gpu import _tiny_full_width_aki

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def hf_processors(penalty=1.0, ngram=0, bad=None, min_new=0, eos=(), suppress=None, begin_suppress=None):
    """The list HF GenerationMixin._get_logits_processor builds for these settings (prompt length 0: inputs_embeds only)."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor)
    out = LogitsProcessorList()
    if penalty != 1.0:
        out.append(RepetitionPenaltyLogitsProcessor(float(penalty)))
    if ngram > 0:
        out.append(NoRepeatNGramLogitsProcessor(ngram))
    if bad:
        out.append(NoBadWordsLogitsProcessor(bad, list(eos) or None))
    if min_new > 0 and eos:
        out.append(MinNewTokensLengthLogitsProcessor(0, min_new, list(eos)))
    if suppress:
        out.append(SuppressTokensLogitsProcessor(suppress))
    if begin_suppress:
        out.append(SuppressTokensAtBeginLogitsProcessor(begin_suppress, 0))
    return out


def assert_scores_equal(got, want, what):
    gi, wi = torch.isneginf(got), torch.isneginf(want)
    assert torch.equal(gi, wi), f"{what}: -inf positions differ at {torch.nonzero(gi != wi)[:8].tolist()}"
    torch.testing.assert_close(got[~gi], want[~wi], rtol=2e-7, atol=0, msg=what)


SETTINGS = [dict(penalty=1.3), dict(penalty=0.7, ngram=2), dict(ngram=1), dict(ngram=3, bad=[[5], [9, 11], [4, 4, 6]]),
            dict(penalty=1.2, ngram=2, bad=[[7, 3]], min_new=6, eos=(2, 31999), suppress=[13, 17], begin_suppress=[19, 20])]


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [32064, 32066])
@pytest.mark.parametrize("si", range(len(SETTINGS)))
def test_kernel_matches_transformers(B, V, si):
    from aki_amd import ops
    s = SETTINGS[si]
    g = torch.Generator().manual_seed(1000 * B + V + si)
    logits = (torch.randn((B, V), generator=g) * 4).to(torch.bfloat16)
    T = 40
    # histories with repeats, matching / non-matching n-grams and the bad words' prefixes: a small alphabet, some rows short or empty
    hist = torch.randint(0, 24, (B, T), generator=g)
    hist[:, 5:8] = torch.tensor([4, 4, 6])
    if B > 1:
        hist[1, 10:12] = hist[1, 20:22]
    lens = torch.tensor([[T, 0, 1, 7, 23, 39, 12, 2][b % 8] for b in range(B)], dtype=torch.int32)
    done = torch.zeros(B, dtype=torch.uint8)
    if B >= 3:
        done[2] = 1                                                     # a finished row: copied unprocessed, picked as pad
    proc = ops.LogitsProcessors(V, DEV, s.get("penalty", 1.0), s.get("ngram", 0), s.get("min_new", 0), s.get("eos", ()), s.get("suppress"),
                                s.get("begin_suppress"), s.get("bad"))
    hf = hf_processors(**s)
    tokens = hist.to(DEV)
    # (1) bf16 in, f32 out; n from the device counters (cache_len - start_len)
    got = proc.apply(logits.to(DEV), tokens=tokens, cache_len=(lens + 100).to(DEV), start_len=torch.full((B,), 100, dtype=torch.int32, device=DEV),
                     done=done.to(DEV)).cpu()
    # (2) f32 in place, n = step for every row: the beam-search call
    f32 = logits.float().to(DEV)
    proc.apply(f32, out=f32, tokens=tokens[:, :lens[0]].contiguous(), step=int(lens[0]))
    want0 = hf(hist[:, :lens[0]], logits.float())
    assert_scores_equal(f32.cpu(), want0, "f32 in place")
    # (3) the processed greedy pick: t = cache_len + 1 - start_len
    ids = torch.zeros(B, dtype=torch.long, device=DEV)
    toks = torch.cat([tokens, torch.full((B, 1), -5, dtype=torch.long, device=DEV)], 1).contiguous()
    cl = (lens + 99).to(DEV)
    ops.greedy_pick(logits.to(DEV), ids, pad_token_id=3, done=done.to(DEV), tokens=toks, cache_len=cl, start_len=torch.full((B,), 100,
                    dtype=torch.int32, device=DEV), advance=True, processors=proc, eos_ids=torch.tensor(s.get("eos", ()) or [31000],
                    dtype=torch.long, device=DEV) if s.get("eos") else None)
    ids = ids.cpu()
    for b in range(B):
        want = hf(hist[b:b + 1, :lens[b]], logits[b:b + 1].float())[0]
        if done[b]:
            assert torch.equal(got[b], logits[b].float()), "a finished row is copied unprocessed"
            assert int(ids[b]) == 3
            continue
        assert_scores_equal(got[b], want, f"row {b} (n = {int(lens[b])})")
        assert int(ids[b]) == int(want.argmax()), f"row {b}: picked {int(ids[b])}, HF's processed argmax {int(want.argmax())}"
        assert int(toks[b, lens[b]]) == int(ids[b])
    assert torch.equal(cl.cpu(), lens + 100)


GEN_KW = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[13, 17])


def _multi(m, vx, ids, am, B):
    g = torch.Generator(device="cpu").manual_seed(9)
    ids_b = [ids]
    for _ in range(B - 1):
        x = torch.randint(3, 32000, (1, ids.shape[1]), generator=g).to(DEV)
        x[0, 0], x[0, 6] = 1, m.media_token_id
        ids_b.append(x)
    return vx.repeat(B, 1, 1, 1, 1, 1), torch.cat(ids_b), am.repeat(B, 1)


def _teacher_forced_check(m, vx, ids, toks, hf, eos=()):
    """Every emitted token against HF's processors on the raw logits of a full forward over prompt + emitted prefix, wherever the processed
    top-2 margin is above the bf16 noise of the logits (the decode path and the full forward sum in different orders)."""
    checked = 0
    for b in range(toks.shape[0]):
        row = toks[b].tolist()
        n = len(row)
        ext = torch.cat([ids[b], toks[b]])
        with torch.no_grad():
            lg = m(vx[b:b + 1], ext[None], attention_mask=torch.ones_like(ext)[None]).logits[0, -(n + 1):-1].float().cpu()
        for s in range(n):
            if s > 0 and row[s - 1] in eos:
                break
            sc = hf(torch.tensor([row[:s]], dtype=torch.long), lg[s:s + 1])[0]
            top = sc.topk(2).values
            if float(top[0] - top[1]) > 0.05 * max(1.0, float(lg[s].abs().max())):
                assert row[s] == int(sc.argmax()), (b, s, row)
                checked += 1
    return checked


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_generate_teacher_forced(use_graph, B):
    m, vx, ids, am = _tiny_full_width_aki()
    vx, ids, am = _multi(m, vx, ids, am, B)
    free = m.generate(vx, ids, attention_mask=am, max_new_tokens=16, eos_token_id=[], use_graph=use_graph)
    eos = [int(free[0, 1])]                                               # the free run would stop at its second token
    bad = [[int(free[0, 3])], [int(free[0, 4]), int(free[0, 5])]]
    kw = dict(GEN_KW, min_new_tokens=5, bad_words_ids=bad)
    toks = m.generate(vx, ids, attention_mask=am, max_new_tokens=16, eos_token_id=eos, pad_token_id=0, use_graph=use_graph, **kw)
    hf = hf_processors(1.3, 2, bad, 5, eos, [13, 17])
    assert toks.shape[1] >= 5
    assert _teacher_forced_check(m, vx, ids, toks, hf, eos) >= toks.shape[0] * 2
    for b in range(B):
        row = toks[b].tolist()
        if eos[0] in row:
            row = row[: row.index(eos[0])]
        assert bad[0][0] not in row and 13 not in row and 17 not in row
        grams = list(zip(row, row[1:]))
        assert len(grams) == len(set(grams)), row


def test_beam_search_applies_the_processors():
    m, vx, ids, am = _tiny_full_width_aki()
    free = m.generate(vx, ids, attention_mask=am, max_new_tokens=12, num_beams=2, eos_token_id=[])
    eos = [int(free[0, 0])]
    toks = m.generate(vx, ids, attention_mask=am, max_new_tokens=12, num_beams=2, eos_token_id=eos, pad_token_id=0, no_repeat_ngram_size=1,
                      min_new_tokens=4, suppress_tokens=[int(free[0, 1])])[0].tolist()
    body = toks[: toks.index(eos[0])] if eos[0] in toks else toks
    assert len(body) >= 4 and len(body) == len(set(body)) and int(free[0, 1]) not in body, toks


def test_beam_search_matches_a_full_forward_beam_search_with_hf_processors():
    """K = 2, no EOS, f32 tiny model: HF's processors on each beam's log-softmax scores with that beam's tokens, then the beam scores."""
    from test_model_gpu import build_tiny, batch
    m, g = build_tiny(torch.float32)
    vx, lx, am, _ = batch(g, torch.float32)
    hf = hf_processors(1.3, 2, None, 0, (), [13, 17])
    got = m.generate(vx, lx, attention_mask=am, max_new_tokens=5, num_beams=2, eos_token_id=[], **GEN_KW)
    for b in range(lx.shape[0]):
        prompt = lx[b, : int(am[b].sum())]
        beams = [(0.0, [])]
        for _ in range(5):
            cand = []
            for sc, tk in beams:
                ext = torch.cat([prompt, torch.tensor(tk, dtype=torch.long, device=DEV)])
                with torch.no_grad():
                    lg = m(vx[b:b + 1], ext[None], attention_mask=torch.ones_like(ext)[None]).logits[0, -1].float().cpu()
                lp = hf(torch.tensor([tk], dtype=torch.long), torch.log_softmax(lg, -1)[None])[0]
                top = lp.topk(4)
                cand += [(sc + float(v), tk + [int(i)]) for v, i in zip(top.values, top.indices)]
            cand.sort(key=lambda c: -c[0])
            beams = cand[:2]
        assert got[b].tolist() == beams[0][1], (b, got[b].tolist(), beams)


@pytest.mark.parametrize("use_graph", [False, True])
def test_must_fail_without_the_feature(use_graph):
    """Both keywords used to be dropped silently."""
    m, vx, ids, am = _tiny_full_width_aki()
    toks = m.generate(vx, ids, attention_mask=am, max_new_tokens=24, eos_token_id=[], no_repeat_ngram_size=1, use_graph=use_graph)[0].tolist()
    assert len(toks) == 24 and len(set(toks)) == 24, toks
    free = m.generate(vx, ids, attention_mask=am, max_new_tokens=24, eos_token_id=[], use_graph=use_graph)[0].tolist()
    eos = sorted(set(free))                                                 # every token the free run picks ends it: argmax forced to EOS
    k = 7
    short = m.generate(vx, ids, attention_mask=am, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, use_graph=use_graph)
    assert short.shape[1] == 1
    out = m.generate(vx, ids, attention_mask=am, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, min_new_tokens=k, use_graph=use_graph)
    assert out.shape[1] > k and not any(t_ in eos for t_ in out[0, :k].tolist()), out.tolist()


def test_unchanged_without_processors(monkeypatch):
    import aki_amd.aki as A
    m, vx, ids, am = _tiny_full_width_aki()
    vx3, ids3, am3 = _multi(m, vx, ids, am, 3)
    for args in ((vx, ids, am), (vx3, ids3, am3)):
        for ug in (False, True):
            plain = m.generate(*args[:2], attention_mask=args[2], max_new_tokens=12, eos_token_id=[], use_graph=ug)
            neutral = m.generate(*args[:2], attention_mask=args[2], max_new_tokens=12, eos_token_id=[], use_graph=ug, repetition_penalty=1.0,
                                 no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=[], bad_words_ids=[])
            assert torch.equal(plain, neutral)
    # seeded sampling: sample_next gets the very same raw logits and generator states, with or without neutral processor keywords, and
    # every draw is sample_next's
    orig = A.sample_next
    seen = []

    def spy(logits, temperature=1.0, top_k=0, top_p=1.0, generator=None):
        state = generator.get_state()
        out = orig(logits, temperature, top_k, top_p, generator)
        again = orig(logits, temperature, top_k, top_p, torch.Generator(device=DEV).set_state(state))
        assert torch.equal(out, again)
        seen[-1].append((logits.clone(), state, out.clone()))
        return out

    monkeypatch.setattr(A, "sample_next", spy)
    outs = []
    for kw in ({}, dict(repetition_penalty=1.0, no_repeat_ngram_size=0)):
        seen.append([])
        g = torch.Generator(device=DEV).manual_seed(11)
        outs.append(m.generate(vx, ids, attention_mask=am, max_new_tokens=6, eos_token_id=[], do_sample=True, top_k=20, temperature=0.8,
                               generator=g, **kw))
    assert torch.equal(outs[0], outs[1]) and len(seen[0]) == len(seen[1]) == 6
    for (l0, s0, o0), (l1, s1, o1) in zip(*seen):
        assert torch.equal(l0, l1) and torch.equal(s0, s1) and torch.equal(o0, o1)


def test_sampling_applies_the_processors():
    m, vx, ids, am = _tiny_full_width_aki()
    g = torch.Generator(device=DEV).manual_seed(3)
    toks = m.generate(vx, ids, attention_mask=am, max_new_tokens=20, eos_token_id=[], do_sample=True, top_k=3, generator=g,
                      no_repeat_ngram_size=1, suppress_tokens=[13])[0].tolist()
    assert len(set(toks)) == 20 and 13 not in toks


@pytest.mark.parametrize("loop", ["greedy", "plain"])
def test_chain_recovery_with_processors(loop):
    from aki_amd import _lib
    m, vx, ids, am = _tiny_full_width_aki()
    kw = dict(max_new_tokens=24, do_sample=False, eos_token_id=[], **GEN_KW)
    if loop == "plain":
        kw["use_graph"] = False
    m.lang_model.model.use_decode_chain = False
    want = m.generate(vx, ids, attention_mask=am, **kw)
    m.lang_model.model.use_decode_chain = True
    with _lib.use_lab(0) as lab:
        clean = m.generate(vx, ids, attention_mask=am, **kw)
        assert torch.equal(clean, want)
        lab.aki_lab_set_chain_fault((1 << 8) | 3, 11)
        with pytest.warns(RuntimeWarning, match="decode chain"):
            got = m.generate(vx, ids, attention_mask=am, **kw)
        lab.aki_lab_set_chain_fault(0, 0)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
