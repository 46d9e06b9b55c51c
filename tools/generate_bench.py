#!/usr/bin/env python3
"""`AKI.generate` end to end, as the reference's callers run it (local_demo.py:76-87, eval_cv_bench/eval.py:99-104: one sample,
`generate(max_new_tokens=256)`, greedy): full AKI-4B (random-init), one 336 px image + 512-token prompt, batch 1.  Reports the time to the
first token (vision tower + connector + splice + MMA prefill into the KV cache) and the time per generated token (one hipGraph replay
each, the greedy pick inside it), with bf16 and with e4m3 weights.  No EOS (random weights never emit one on cue): all 256 tokens.
--repetition-penalty / --no-repeat-ngram: every round also runs with those logits processors on (the processed greedy pick) and reports the
per-token cost they add, measured on the same box in the same process.
--sample: every round also runs `do_sample=True` twice in the same process - with a torch.Generator (the `sample_next` loop) and with a
DeviceGenerator (ops.sample_pick inside the greedy loop) - and reports both per-token times and the device sampler's excess over greedy.
--batch B: B copies of the sample (the batched decode path; a hipGraph replay per token).
--logprobs K (K >= 0; -1 = off, the default): every round also runs with output_logprobs=True, top_logprobs=K (one ops.token_logprob launch
behind each pick), alternating with the plain leg in the same process; reports the per-token cost it adds (median and spread over the
rounds) and merges the result into profiles/logprob_bench.json under "batch<B>_k<K>".
--constraint: every round also runs greedy under a token constraint (on top of --repetition-penalty where given: a penalty composes with a
constraint, a banning processor does not), alternating with the other legs in the same process: a 16-state cycle in which state s allows the
ids v with v % 16 == s (one automaton per sample at --batch B, joined into one table), so every token reads one table row per sequence.
Reports the per-token cost over the processors leg (over the plain leg without one) and merges the result into
profiles/constraint_bench.json under "batch<B>".
--many: in-flight batching (many_bench below): 64 requests at this prompt with budgets 16..256 from a fixed seed, EOS off, at 8 and 16 slots;
generate() over consecutive groups of `slots` requests (max_new_tokens = the group's largest budget) against generate_many, alternating in one
process for at least 3 rounds.  Writes profiles/many_bench.json: returned tokens/s of both legs, the scheduler's counters, the occupancy
the lengths alone predict for the static groups against the scheduler's live / total row-steps, and the share of wall time inside admits.
--many --sample [--temperature T --top-k K --top-p P] [--logprobs K]: the queue with per-request sampling (many_sample_bench below): the same 64
requests, budgets, EOS off and slot counts; the greedy queue leg and the sampled queue leg (every request RequestParams(do_sample=True,
...) with its own seed) alternate in one process, with --logprobs K two more legs (greedy requests with logprobs=True at top_logprobs 0
and K).  Writes profiles/many_sample_bench.json: returned tokens/s and wall ms per decode step of every leg, and each leg's excess per step
over the greedy leg of the same round (the admits are the same work in every leg).
--many --constraint: the queue with per-request token constraints (many_constraint_bench below): the same 64 requests, each with its OWN
16-state cycle object (state s allows the ids v with v % 16 == s: a pool of 64 x 16 states, one table row read per row and step), against
the greedy queue, alternating in one process at 8 and 16 slots.  Writes profiles/many_constraint_bench.json: tokens/s and ms per decode
step of both legs, the microseconds per step the constrained leg adds (median and spread over the rounds).
--many --request-processors: the queue with per-request logits processors (many_processors_bench below): the same 64 requests, their
settings cycling over four distinct sets (the neutral one, --repetition-penalty 1.2 with --no-repeat-ngram 3, and two with id lists), against
the call-wide processors leg (those two keywords for every row) and the plain greedy queue, alternating in one process at 8 and 16 slots.
Writes profiles/many_processors_bench.json: tokens/s and ms per decode step of the three legs, and the per-request leg's difference per
step from the call-wide leg next to that leg's own spread over the rounds.
--many --stop: the queue with per-request stop sequences (many_stop_bench below): the same 64 requests, each with its OWN set of 8 token
sequences of 1 to 4 ids built from ids the greedy queue never emits, so nothing ever matches and the schedules are identical; against the
plain greedy queue, alternating in one process at 8 and 16 slots for at least 3 rounds.  Writes profiles/many_stop_bench.json: tokens/s
and ms per decode step of both legs, and the stop leg's difference per step from the plain leg of the same round next to the plain leg's
own spread between the rounds.
--stop (without --many): every round also runs with stop_sequences= such a set of 8 (one ops.stop_check launch behind each pick),
alternating with the plain leg; reports the per-token cost it adds and merges the result into profiles/stop_bench.json under "batch<B>".
    python tools/generate_bench.py [--many] [--many --sample --temperature 0.8 --top-k 50 --top-p 0.9 --logprobs 8] [--many --constraint]
                                   [--many --request-processors] [--many --stop]
--min-p M / --frequency-penalty F / --presence-penalty P (any of them): the penalty bench instead of the legs above - plain greedy, the
device sampler (--temperature / --top-k / --top-p) without and with min_p, and repetition_penalty (--repetition-penalty, default 1.2)
without and with the two additive penalties, alternating in one process for at least 3 rounds; --long-history N runs the two
repetition legs once more at N new tokens.  With --many the same five legs over generate_many's queue (the values in every request's
RequestParams) at 8 and 16 slots.  Each new leg is reported against its neighbour leg of the same round, beside that neighbour's own
spread over the rounds.  Merges the result into profiles/penalty_bench.json under "static" / "many".

    python tools/generate_bench.py [--new 256] [--fp8] [--txt 64] [--repetition-penalty 1.2] [--no-repeat-ngram 3]
                                   [--sample --temperature 0.8 --top-k 50 --top-p 0.9] [--batch 8] [--logprobs 8 --rounds 4] [--constraint] [--stop]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def many_bench(a, model, dev):
    """--many: 64 requests at the headline prompt, budgets from a fixed seed in 16..256, EOS off (random weights have no EOS behaviour, so the
    budget IS the length distribution), at 8 and 16 slots.  Two legs alternate in one process: today's way - generate() over consecutive
    groups of `slots` requests with max_new_tokens = the group's largest budget - and generate_many.  Writes profiles/many_bench.json."""
    import bench
    from aki_amd import ops
    n_req = a.many_requests
    g = torch.Generator(device="cpu").manual_seed(4242)
    budgets = torch.randint(16, 257, (n_req,), generator=g).tolist()
    reqs = []
    for i in range(n_req):
        vx, ids, _ = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000 + i)
        reqs.append((vx, ids, budgets[i]))
    # GPU time inside admits: an event in front of each batch-1 prefill and one behind the copy into the slot (the pick and the tick
    # behind it are two short launches)
    spans = []
    real_prefill, real_admit = model._prefill_request, ops.kv_slot_admit

    def prefill(vx, lx):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        spans.append([ev, None])
        return real_prefill(vx, lx)

    def admit(src, dst, slot):
        real_admit(src, dst, slot)
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        spans[-1][1] = ev

    def static_leg(slots):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for lo in range(0, n_req, slots):
            grp = reqs[lo:lo + slots]
            vx, ids = torch.cat([r[0] for r in grp]), torch.cat([r[1] for r in grp])
            toks = model.generate(vx, ids, attention_mask=torch.ones_like(ids), max_new_tokens=max(r[2] for r in grp), eos_token_id=[])
            n += sum(min(r[2], toks.shape[1]) for r in grp)       # returned tokens: each row up to its own budget
        torch.cuda.synchronize()
        return time.perf_counter() - t0, n

    def many_leg(slots):
        del spans[:]
        model._prefill_request, ops.kv_slot_admit = prefill, admit
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = model.generate_many(reqs, slots=slots, eos_token_id=[])
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        finally:
            model._prefill_request, ops.kv_slot_admit = real_prefill, real_admit
        assert [o.numel() for o in outs] == budgets
        admit_ms = sum(s.elapsed_time(e) for s, e in spans)
        return wall, sum(budgets), dict(model.last_many_stats), admit_ms

    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {"requests": n_req, "prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV, "budgets": budgets, "budget_seed": 4242,
           "method": "two legs alternating in one process, wall clock around each leg with a device synchronisation on both sides; "
                     "tokens/s = returned tokens / wall time, prefills included", "slots": {}}
    for slots in (8, 16):
        groups = [budgets[lo:lo + slots] for lo in range(0, n_req, slots)]
        predicted = sum(budgets) / sum(slots * max(grp) for grp in groups)
        static_leg(slots), many_leg(slots)                        # warm-up: allocator, folds, capture path
        rounds = []
        for _ in range(max(3, a.rounds)):
            ts, ns = static_leg(slots)
            tm, nm, stats, admit_ms = many_leg(slots)
            rounds.append({"static_tokens_per_s": round(ns / ts, 1), "many_tokens_per_s": round(nm / tm, 1), "static_s": round(ts, 3),
                           "many_s": round(tm, 3), "admit_ms": round(admit_ms, 1), "admit_share_of_wall": round(admit_ms / (tm * 1e3), 4)})
        res["slots"][str(slots)] = {
            "rounds": rounds, "stats": stats,
            "static_tokens_per_s_median": med([r["static_tokens_per_s"] for r in rounds]),
            "many_tokens_per_s_median": med([r["many_tokens_per_s"] for r in rounds]),
            "speedup_median": round(med([r["many_tokens_per_s"] / r["static_tokens_per_s"] for r in rounds]), 3),
            "admit_share_of_wall_median": med([r["admit_share_of_wall"] for r in rounds]),
            "static_occupancy_from_lengths": round(predicted, 4),          # sum of budgets / sum over groups of slots x group maximum
            "many_occupancy_live_over_total": round(stats["live_row_steps"] / stats["total_row_steps"], 4),
            "occupancy_bound_on_speedup": round(stats["live_row_steps"] / stats["total_row_steps"] / predicted, 3)}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "budgets"}))


def many_sample_bench(a, model, dev):
    """--many --sample: generate_many with per-request sampling against the greedy queue, many_bench's requests.  Writes
    profiles/many_sample_bench.json."""
    import aki_amd
    import bench
    n_req = a.many_requests
    g = torch.Generator(device="cpu").manual_seed(4242)
    budgets = torch.randint(16, 257, (n_req,), generator=g).tolist()
    reqs = []
    for i in range(n_req):
        vx, ids, _ = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000 + i)
        reqs.append((vx, ids, budgets[i]))
    sampler = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    legs = {"greedy": [aki_amd.RequestParams()] * n_req,
            "sampled": [aki_amd.RequestParams(seed=0x5EED0000 + i, **sampler) for i in range(n_req)]}
    if a.logprobs >= 0:
        for k in sorted({0, a.logprobs}):
            legs[f"greedy_logprobs_k{k}"] = [aki_amd.RequestParams(logprobs=True, top_logprobs=k)] * n_req

    def leg(name, slots):
        batch = [(vx, ids, b, rp) for (vx, ids, b), rp in zip(reqs, legs[name])]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = model.generate_many(batch, slots=slots, eos_token_id=[])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        toks = [o.tokens if isinstance(o, aki_amd.AkiRequestOutput) else o for o in outs]
        assert [t.numel() for t in toks] == budgets
        return wall, dict(model.last_many_stats)

    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {"requests": n_req, "prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV, "budgets": budgets, "budget_seed": 4242,
           "sampler": dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p), "top_logprobs": a.logprobs,
           "method": "the legs alternate in one process, wall clock around each generate_many call with a device synchronisation on both "
                     "sides; tokens/s = returned tokens / wall time, prefills included; ms_per_step = wall time / decode steps replayed, "
                     "admits included - every leg admits the same 64 prompts, so the excess over the greedy leg of the same round is the "
                     "pick's (and the log-probability launch's) cost per step", "slots": {}}
    for slots in (8, 16):
        for name in legs:
            leg(name, slots)                                          # warm-up: allocator, folds, capture path
        rounds = []
        for _ in range(max(3, a.rounds)):
            r = {}
            for name in legs:
                wall, stats = leg(name, slots)
                r[name] = {"tokens_per_s": round(sum(budgets) / wall, 1), "wall_s": round(wall, 3), "steps": stats["steps"],
                           "ms_per_step": round(wall * 1e3 / stats["steps"], 4)}
            rounds.append(r)
        summary = {}
        for name in legs:
            summary[name] = {"tokens_per_s_median": med([r[name]["tokens_per_s"] for r in rounds]),
                             "tokens_per_s_min_max": [min(r[name]["tokens_per_s"] for r in rounds), max(r[name]["tokens_per_s"] for r in rounds)],
                             "ms_per_step_median": med([r[name]["ms_per_step"] for r in rounds])}
            if name != "greedy":
                ex = [(r[name]["ms_per_step"] - r["greedy"]["ms_per_step"]) * 1e3 for r in rounds]
                summary[name]["excess_us_per_step_over_greedy_median"] = round(med(ex), 1)
                summary[name]["excess_us_per_step_over_greedy_min_max"] = [round(min(ex), 1), round(max(ex), 1)]
        res["slots"][str(slots)] = {"rounds": rounds, "summary": summary}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_sample_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "budgets"}))


def many_constraint_bench(a, model, dev):
    """--many --constraint: generate_many with a token constraint per request against the greedy queue, many_bench's requests.  Writes
    profiles/many_constraint_bench.json."""
    import numpy as np
    import aki_amd
    import bench
    from aki_amd.constraint import TokenConstraint
    n_req = a.many_requests
    g = torch.Generator(device="cpu").manual_seed(4242)
    budgets = torch.randint(16, 257, (n_req,), generator=g).tolist()
    reqs = []
    for i in range(n_req):
        vx, ids, _ = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000 + i)
        reqs.append((vx, ids, budgets[i]))
    head = model.lang_model.get_output_embeddings()              # V': the logits' width
    V = int(head.max_original_id) + 1 + int(head.additional_out_features) if hasattr(head, "max_original_id") else int(head.out_features)
    nxt = np.full((16, V), -1, dtype=np.int32)
    for s_ in range(16):
        nxt[s_, s_::16] = (s_ + 1) % 16
    # one OBJECT per request: the pool stores 64 tables of 16 states (equal objects would be stored once)
    legs = {"greedy": [aki_amd.RequestParams()] * n_req,
            "constrained": [aki_amd.RequestParams(constraint=TokenConstraint.from_table(nxt, np.ones(16, dtype=bool))) for _ in range(n_req)]}

    def leg(name, slots):
        batch = [(vx, ids, b, rp) for (vx, ids, b), rp in zip(reqs, legs[name])]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = model.generate_many(batch, slots=slots, eos_token_id=[])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert [o.numel() for o in outs] == budgets
        if name == "constrained":
            for o in outs:
                assert bool((o % 16 == torch.arange(o.numel(), device=dev) % 16).all()), "not a walk of the cycle"
        return wall, dict(model.last_many_stats)

    def pool_ms():
        """What a constrained call pays once, whatever its length: the pool built on the host and uploaded (the tables' checks are cached
        in the constraint objects after the warm-up)."""
        from aki_amd.constraint import ConstraintPool
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ConstraintPool([], [rp.constraint for rp in legs["constrained"]], V).bind(dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {"requests": n_req, "prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV, "budgets": budgets, "budget_seed": 4242,
           "constraint": "one 16-state cycle object per request (state s allows v with v % 16 == s): a pool of 64 x 16 states",
           "pool_states": 16 * n_req, "pool_bytes": 16 * n_req * ((V + 7) // 8 * 8) * 2,
           "method": "the two legs alternate in one process, wall clock around each generate_many call with a device synchronisation on "
                     "both sides; tokens/s = returned tokens / wall time, prefills and the pool's one upload included; ms_per_step = wall "
                     "time / decode steps replayed - both legs admit the same 64 prompts, so the excess over the greedy leg of the same "
                     "round is the constrained call's cost per step: the pick's, plus the pool's build and upload (once per call, timed "
                     "on its own as pool_ms) spread over the steps; added_us_per_step_without_the_pool takes that share out", "slots": {}}
    for slots in (8, 16):
        for name in legs:
            leg(name, slots)                                          # warm-up: allocator, folds, capture path
        rounds = []
        for _ in range(max(3, a.rounds)):
            r = {}
            for name in legs:
                wall, stats = leg(name, slots)
                r[name] = {"tokens_per_s": round(sum(budgets) / wall, 1), "wall_s": round(wall, 3), "steps": stats["steps"],
                           "ms_per_step": round(wall * 1e3 / stats["steps"], 4)}
            r["pool_ms"] = round(pool_ms(), 2)
            rounds.append(r)
        summary = {}
        for name in legs:
            summary[name] = {"tokens_per_s_median": med([r[name]["tokens_per_s"] for r in rounds]),
                             "tokens_per_s_min_max": [min(r[name]["tokens_per_s"] for r in rounds), max(r[name]["tokens_per_s"] for r in rounds)],
                             "ms_per_step_median": med([r[name]["ms_per_step"] for r in rounds])}
        ex = [(r["constrained"]["ms_per_step"] - r["greedy"]["ms_per_step"]) * 1e3 for r in rounds]
        net = [e - r["pool_ms"] * 1e3 / r["constrained"]["steps"] for e, r in zip(ex, rounds)]
        summary["constrained"]["added_us_per_step_median"] = round(med(ex), 1)
        summary["constrained"]["added_us_per_step_min_max"] = [round(min(ex), 1), round(max(ex), 1)]
        summary["constrained"]["pool_ms_median"] = med([r["pool_ms"] for r in rounds])
        summary["constrained"]["added_us_per_step_without_the_pool_median"] = round(med(net), 1)
        summary["constrained"]["added_us_per_step_without_the_pool_min_max"] = [round(min(net), 1), round(max(net), 1)]
        res["slots"][str(slots)] = {"rounds": rounds, "summary": summary}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_constraint_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "budgets"}))


def never_matching_stops(emitted, V, n_sets):
    """n_sets stop sets of 8 sequences of 1 to 4 ids each (lengths 1, 2, 3, 4, 1, 2, 3, 4), built from the lowest ids >= 3 that are not in
    `emitted`: a run whose tokens all lie in `emitted` never matches one.  Set r starts 20 ids behind set r - 1: the sets are distinct."""
    unused = [i for i in range(3, V) if i not in emitted][:20 * n_sets + 64]
    assert len(unused) >= 20 * n_sets + 20, "too few ids the run never emits"
    sets = []
    for r in range(n_sets):
        ids, seqs = iter(unused[20 * r:20 * r + 20]), []
        for n in (1, 2, 3, 4, 1, 2, 3, 4):
            seqs.append([next(ids) for _ in range(n)])
        sets.append(seqs)
    return sets


def many_stop_bench(a, model, dev):
    """--many --stop: generate_many with a stop set per request that never matches against the plain greedy queue, many_bench's requests.
    Writes profiles/many_stop_bench.json."""
    import aki_amd
    import bench
    n_req = a.many_requests
    g = torch.Generator(device="cpu").manual_seed(4242)
    budgets = torch.randint(16, 257, (n_req,), generator=g).tolist()
    reqs = []
    for i in range(n_req):
        vx, ids, _ = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000 + i)
        reqs.append((vx, ids, budgets[i]))
    legs = {"greedy": [aki_amd.RequestParams()] * n_req}
    ref = {}

    def leg(name, slots):
        batch = [(vx, ids, b, rp) for (vx, ids, b), rp in zip(reqs, legs[name])]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = model.generate_many(batch, slots=slots, eos_token_id=[])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if name == "stops":                                           # nothing matched: the same tokens, the same schedule
            for r, (o, want, hit) in enumerate(zip(outs, ref[slots], model.last_stop_hits)):
                if hit != -1 or not torch.equal(o, want):
                    n = o.numel()
                    raise AssertionError(f"request {r}: {n} of {budgets[r]} tokens, stop_hit {hit}, its set {legs[name][r].stop_sequences}, "
                                         f"last tokens {o[-6:].tolist()}; equal to the plain queue's first {n}: {torch.equal(o, want[:n])}")
        else:
            assert model.last_stop_hits is None
            ref[slots] = outs
        assert [o.numel() for o in outs] == budgets
        return wall, dict(model.last_many_stats)

    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {"requests": n_req, "prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV, "budgets": budgets, "budget_seed": 4242,
           "stops": "one set per request, 8 sequences of 1, 2, 3, 4, 1, 2, 3, 4 ids, from ids the greedy queue never emits: a pool of 64 "
                    "sets that never match",
           "method": "the two legs alternate in one process, wall clock around each generate_many call with a device synchronisation on "
                     "both sides; tokens/s = returned tokens / wall time, prefills and the pool's one upload included; ms_per_step = wall "
                     "time / decode steps replayed - both legs admit the same 64 prompts and replay the same number of steps, so the "
                     "difference from the greedy leg of the same round is what the stops cost per step (the check inside the tick's "
                     "launch, plus the admit's one check launch and the pool's upload spread over the steps); it is to be read next to "
                     "greedy_ms_per_step_spread, the plain leg's own max - min between the rounds", "slots": {}}
    emitted = set()
    for slots in (8, 16):                                             # warm-up: allocator, folds, capture path - and the ids the queue emits
        for _ in range(2):                                            # (another slot count is another batch size: other roundings, other tokens)
            leg("greedy", slots)
            emitted |= set(torch.cat(ref[slots]).tolist())
    legs["stops"] = [aki_amd.RequestParams(stop_sequences=s) for s in never_matching_stops(emitted, model._logits_width(), n_req)]
    for slots in (8, 16):
        leg("greedy", slots), leg("stops", slots)
        rounds = []
        for _ in range(max(3, a.rounds)):
            r = {}
            for name in legs:
                wall, stats = leg(name, slots)
                r[name] = {"tokens_per_s": round(sum(budgets) / wall, 1), "wall_s": round(wall, 3), "steps": stats["steps"],
                           "ms_per_step": round(wall * 1e3 / stats["steps"], 4)}
            assert r["stops"]["steps"] == r["greedy"]["steps"]
            rounds.append(r)
        summary = {}
        for name in legs:
            summary[name] = {"tokens_per_s_median": med([r[name]["tokens_per_s"] for r in rounds]),
                             "tokens_per_s_min_max": [min(r[name]["tokens_per_s"] for r in rounds), max(r[name]["tokens_per_s"] for r in rounds)],
                             "ms_per_step_median": med([r[name]["ms_per_step"] for r in rounds])}
        ex = [(r["stops"]["ms_per_step"] - r["greedy"]["ms_per_step"]) * 1e3 for r in rounds]
        plain = [r["greedy"]["ms_per_step"] * 1e3 for r in rounds]
        summary["stops"]["added_us_per_step_median"] = round(med(ex), 1)
        summary["stops"]["added_us_per_step_min_max"] = [round(min(ex), 1), round(max(ex), 1)]
        summary["greedy"]["us_per_step_spread_between_rounds"] = round(max(plain) - min(plain), 1)
        res["slots"][str(slots)] = {"rounds": rounds, "summary": summary}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_stop_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "budgets"}))


def many_processors_bench(a, model, dev):
    """--many --request-processors: generate_many with per-request logits processors (the settings cycling over four distinct sets) against
    the call-wide processors leg and the plain greedy queue, many_bench's requests.  Writes profiles/many_processors_bench.json."""
    import aki_amd
    import bench
    n_req = a.many_requests
    g = torch.Generator(device="cpu").manual_seed(4242)
    budgets = torch.randint(16, 257, (n_req,), generator=g).tolist()
    reqs = []
    for i in range(n_req):
        vx, ids, _ = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000 + i)
        reqs.append((vx, ids, budgets[i]))
    wide = dict(repetition_penalty=a.repetition_penalty if a.repetition_penalty != 1.0 else 1.2,
                no_repeat_ngram_size=a.no_repeat_ngram if a.no_repeat_ngram > 0 else 3)
    cycle = [{}, dict(wide), dict(repetition_penalty=1.05, suppress_tokens=[11, 12, 13], bad_words_ids=[[21, 22], [23]]),
             dict(no_repeat_ngram_size=2, begin_suppress_tokens=[31, 32])]
    plain = [aki_amd.RequestParams()] * n_req
    legs = {"greedy": (plain, {}), "call_wide": (plain, wide),
            "per_request": ([aki_amd.RequestParams(**cycle[i % len(cycle)]) for i in range(n_req)], {})}

    def leg(name, slots):
        params, kw = legs[name]
        batch = [(vx, ids, b, rp) for (vx, ids, b), rp in zip(reqs, params)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = model.generate_many(batch, slots=slots, eos_token_id=[], **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert [o.numel() for o in outs] == budgets
        if name == "per_request":                                    # the 3-gram ban holds on the requests that carry it, and only there is it asked
            for i, o in enumerate(outs):
                if cycle[i % len(cycle)].get("no_repeat_ngram_size") == 3:
                    row = o.tolist()
                    grams = list(zip(row, row[1:], row[2:]))
                    assert len(grams) == len(set(grams)), f"request {i} repeats a 3-gram"
        return wall, dict(model.last_many_stats)

    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {"requests": n_req, "prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV, "budgets": budgets, "budget_seed": 4242,
           "call_wide": wide, "per_request_cycle": cycle,
           "method": "the three legs alternate in one process, wall clock around each generate_many call with a device synchronisation on "
                     "both sides; tokens/s = returned tokens / wall time, prefills included; ms_per_step = wall time / decode steps replayed. "
                     "All legs admit the same 64 prompts with the same budgets (EOS off), so they replay the same number of steps.  The "
                     "per-request leg is compared with the call-wide leg of the same round (the per-row pick against the processed pick); "
                     "the call-wide leg's own spread over the rounds is the yardstick", "slots": {}}
    for slots in (8, 16):
        for name in legs:
            leg(name, slots)                                          # warm-up: allocator, folds, capture path
        rounds = []
        for _ in range(max(3, a.rounds)):
            r = {}
            for name in legs:
                wall, stats = leg(name, slots)
                r[name] = {"tokens_per_s": round(sum(budgets) / wall, 1), "wall_s": round(wall, 3), "steps": stats["steps"],
                           "ms_per_step": round(wall * 1e3 / stats["steps"], 4)}
            rounds.append(r)
        summary = {}
        for name in legs:
            ms = [r[name]["ms_per_step"] for r in rounds]
            summary[name] = {"tokens_per_s_median": med([r[name]["tokens_per_s"] for r in rounds]),
                             "tokens_per_s_min_max": [min(r[name]["tokens_per_s"] for r in rounds), max(r[name]["tokens_per_s"] for r in rounds)],
                             "ms_per_step_median": med(ms), "ms_per_step_min_max": [min(ms), max(ms)]}
        ex = [(r["per_request"]["ms_per_step"] - r["call_wide"]["ms_per_step"]) * 1e3 for r in rounds]
        cw = summary["call_wide"]["ms_per_step_min_max"]
        summary["per_request"]["us_per_step_over_call_wide_median"] = round(med(ex), 1)
        summary["per_request"]["us_per_step_over_call_wide_min_max"] = [round(min(ex), 1), round(max(ex), 1)]
        summary["call_wide"]["us_per_step_spread_over_rounds"] = round((cw[1] - cw[0]) * 1e3, 1)
        summary["per_request"]["inside_the_call_wide_legs_spread"] = bool(abs(med(ex)) <= (cw[1] - cw[0]) * 1e3)
        res["slots"][str(slots)] = {"rounds": rounds, "summary": summary}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_processors_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "budgets"}))


def _leg_summary(rounds, names, key):
    med = lambda xs: sorted(xs)[len(xs) // 2]
    return {n: {"median": med([r[n][key] for r in rounds]), "min_max": [min(r[n][key] for r in rounds), max(r[n][key] for r in rounds)]}
            for n in names}


def _penalty_deltas(rounds, summary, key, scale):
    """Each new leg against its neighbour leg of the same round, in microseconds, with the neighbour's own spread over the rounds."""
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {}
    for new, base in (("sampled_min_p", "sampled"), ("repetition_penalties", "repetition")):
        d = [(r[new][key] - r[base][key]) * scale for r in rounds]
        lo, hi = summary[base]["min_max"]
        out[f"{new}_over_{base}_us"] = {"median": round(med(d), 2), "min_max": [round(min(d), 2), round(max(d), 2)],
                                        f"{base}_spread_over_rounds_us": round((hi - lo) * scale, 2)}
    return out


def penalty_bench(a, model, dev):
    """--min-p / --frequency-penalty / --presence-penalty: the sampled leg with and without min_p, and the repetition_penalty leg with and
    without the two additive penalties, beside plain greedy, alternating in one process - generate() on one prompt (with --long-history N
    also once at N new tokens: the history the penalties count), or with --many generate_many over many_bench's queue with the values in
    every request's RequestParams.  Merges the result into profiles/penalty_bench.json under "static" / "many"."""
    import aki_amd
    import bench
    pen = {k: v for k, v in (("frequency_penalty", a.frequency_penalty), ("presence_penalty", a.presence_penalty)) if v != 0.0}
    rp = a.repetition_penalty if a.repetition_penalty != 1.0 else 1.2
    samp = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    minp = {"min_p": a.min_p} if a.min_p > 0.0 else {}
    names = ("greedy", "sampled", "sampled_min_p", "repetition", "repetition_penalties")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "penalty_bench.json")
    res = {"values": dict(pen, repetition_penalty=rp, **minp), "sampling": dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p),
           "prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV}
    if a.many:
        n_req = a.many_requests
        g = torch.Generator(device="cpu").manual_seed(4242)
        budgets = torch.randint(16, 257, (n_req,), generator=g).tolist()
        reqs = []
        for i in range(n_req):
            vx, ids, _ = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000 + i)
            reqs.append((vx, ids, budgets[i]))
        P = aki_amd.RequestParams
        legs = {"greedy": (lambda i: P(), {}), "sampled": (lambda i: P(seed=i, **samp), {}),
                "sampled_min_p": (lambda i: P(seed=i, **samp, **minp), {}), "repetition": (lambda i: P(), dict(repetition_penalty=rp)),
                "repetition_penalties": (lambda i: P(**pen), dict(repetition_penalty=rp))}

        def leg(name, slots):
            make, kw = legs[name]
            batch = [(vx, ids, b, make(i)) for i, (vx, ids, b) in enumerate(reqs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = model.generate_many(batch, slots=slots, eos_token_id=[], **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert [o.numel() for o in outs] == budgets
            return wall, dict(model.last_many_stats)

        res.update(requests=n_req, budget_seed=4242, slots={},
                   method="the five legs alternate in one process, wall clock around each generate_many call with a device synchronisation on "
                          "both sides; ms_per_step = wall time / decode steps replayed, prefills included.  All legs admit the same prompts "
                          "with the same budgets (EOS off) and replay the same number of steps; a new leg is compared with its neighbour leg "
                          "of the same round, whose spread over the rounds is the yardstick")
        for slots in (8, 16):
            for name in names:
                leg(name, slots)
            rounds = []
            for _ in range(max(3, a.rounds)):
                r = {}
                for name in names:
                    wall, stats = leg(name, slots)
                    r[name] = {"tokens_per_s": round(sum(budgets) / wall, 1), "steps": stats["steps"], "ms_per_step": round(wall * 1e3 / stats["steps"], 4)}
                rounds.append(r)
            summary = _leg_summary(rounds, names, "ms_per_step")
            res["slots"][str(slots)] = {"rounds": rounds, "ms_per_step": summary, "added_per_step": _penalty_deltas(rounds, summary, "ms_per_step", 1e3)}
    else:
        vx, ids, am = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000)
        kws = {"greedy": {}, "sampled": samp, "sampled_min_p": dict(samp, **minp), "repetition": dict(repetition_penalty=rp),
               "repetition_penalties": dict(pen, repetition_penalty=rp)}

        def run(n_new, name):
            kw = dict(kws[name])
            if kw.get("do_sample"):
                kw["generator"] = aki_amd.DeviceGenerator(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = model.generate(vx, ids, attention_mask=am, max_new_tokens=n_new, eos_token_id=[], **kw)
            torch.cuda.synchronize()
            assert toks.shape == (1, n_new)
            return time.perf_counter() - t0

        def measure(n_new, which, n_rounds):
            rounds = []
            for _ in range(n_rounds):
                r = {}
                for name in which:
                    t1 = run(1, name)
                    r[name] = {"ms_per_new_token_after_the_first": round((run(n_new, name) - t1) * 1e3 / (n_new - 1), 4)}
                rounds.append(r)
            return rounds

        for name in names:
            run(16, name)                                                 # warm-up: allocator, folds, the capture path
        rounds = measure(a.new, names, max(3, a.rounds))
        summary = _leg_summary(rounds, names, "ms_per_new_token_after_the_first")
        res.update(new_tokens=a.new, rounds=rounds, ms_per_token=summary,
                   added_per_token=_penalty_deltas(rounds, summary, "ms_per_new_token_after_the_first", 1e3),
                   method="the five legs alternate in one process; ms per new token after the first = (wall time of a call with new_tokens "
                          "- wall time of a call with one) / (new_tokens - 1), a device synchronisation on both sides of each call")
        if a.long_history > 1:
            two = ("repetition", "repetition_penalties")
            long_rounds = measure(a.long_history, two, 2)
            ls = _leg_summary(long_rounds, two, "ms_per_new_token_after_the_first")
            d = [(r[two[1]][k] - r[two[0]][k]) * 1e3 for r in long_rounds for k in ("ms_per_new_token_after_the_first",)]
            res["long_history"] = {"new_tokens": a.long_history, "rounds": long_rounds, "ms_per_token": ls,
                                   "repetition_penalties_over_repetition_us_mean_over_the_history": [round(x, 2) for x in d],
                                   "note": "the mean over histories of 1 .. new_tokens - 1 tokens; the count is taken over the whole "
                                           "history on every step"}
    book = json.load(open(path)) if os.path.exists(path) else {}
    book["many" if a.many else "static"] = res
    with open(path, "w") as f:
        json.dump(book, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--mxfp4", action="store_true", help="MXFP4 weights for the decode rows (enable_mxfp4; combines with --fp8: prefill e4m3, decode MXFP4)")
    ap.add_argument("--w4-chain", action="store_true", help="with --mxfp4, one sequence: decode on the one-launch chain (Phi3Model.decode_chain_w4, off by default)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--txt", type=int, default=512, help="prompt tokens: 512 = the headline prompt (L = 655), 64 = BASELINE configs[0] (L = 207)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--no-repeat-ngram", type=int, default=0)
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--num-return-sequences", type=int, default=1, help="N sampled continuations per prompt (device sampler): one more leg per round")
    ap.add_argument("--no-share-prompt-kv", action="store_true", help="with --num-return-sequences: replicate the prompt K/V N times (the A/B form; "
                    "without it the leg switches lang_model.share_prompt_kv on)")
    ap.add_argument("--logprobs", type=int, default=-1, help="K >= 0: one more leg per round with output_logprobs=True, top_logprobs=K (-1: off)")
    ap.add_argument("--constraint", action="store_true", help="one more leg per round: greedy under a 16-state token constraint")
    ap.add_argument("--many", action="store_true", help="in-flight batching: generate() over static groups against generate_many, 64 requests with "
                    "budgets 16..256 at 8 and 16 slots -> profiles/many_bench.json (the other legs are skipped); with --sample: the greedy "
                    "queue against the queue with per-request sampling (and --logprobs K) -> profiles/many_sample_bench.json; with "
                    "--constraint: against the queue with one 16-state constraint per request -> profiles/many_constraint_bench.json")
    ap.add_argument("--stop", action="store_true", help="one more leg per round: greedy with a stop set of 8 sequences that never match -> "
                    "profiles/stop_bench.json; with --many: the greedy queue against the queue with one such set per request -> "
                    "profiles/many_stop_bench.json")
    ap.add_argument("--many-requests", type=int, default=64)
    ap.add_argument("--request-processors", action="store_true", help="with --many: per-request logits processors against the call-wide "
                    "processors leg and the greedy queue -> profiles/many_processors_bench.json")
    ap.add_argument("--min-p", type=float, default=0.0, help="with --frequency-penalty / --presence-penalty: the penalty bench - sampled with and "
                    "without min_p, repetition_penalty with and without the two penalties, alternating; with --many over generate_many's "
                    "queue -> profiles/penalty_bench.json")
    ap.add_argument("--frequency-penalty", type=float, default=0.0)
    ap.add_argument("--presence-penalty", type=float, default=0.0)
    ap.add_argument("--long-history", type=int, default=0, help="the penalty bench's static legs once more at this many new tokens (4096)")
    a = ap.parse_args()
    lp_kw =dict(output_logprobs=True, top_logprobs=a.logprobs) if a.logprobs >= 0 else None
    proc_kw = {}
    if a.repetition_penalty != 1.0:
        proc_kw["repetition_penalty"] = a.repetition_penalty
    if a.no_repeat_ngram > 0:
        proc_kw["no_repeat_ngram_size"] = a.no_repeat_ngram
    import bench
    bench.N_TXT = a.txt
    from aki_amd.factory import build_aki
    dev = torch.device("cuda", 0)
    model = build_aki(dtype=torch.bfloat16, device=dev, seed=0).eval()
    if a.fp8:
        model.lang_model.enable_fp8()
    if a.mxfp4:
        model.lang_model.enable_mxfp4()
    model.lang_model.model.decode_chain_w4 = bool(a.w4_chain)
    if a.min_p > 0.0 or a.frequency_penalty != 0.0 or a.presence_penalty != 0.0:
        return penalty_bench(a, model, dev)
    if a.many:
        if a.request_processors:
            return many_processors_bench(a, model, dev)
        if a.constraint:
            return many_constraint_bench(a, model, dev)
        if a.stop:
            return many_stop_bench(a, model, dev)
        return many_sample_bench(a, model, dev) if a.sample else many_bench(a, model, dev)
    vx, ids, am =bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000)
    if a.batch > 1:
        vx, ids, am = vx.repeat(a.batch, 1, 1, 1, 1, 1), ids.repeat(a.batch, 1), am.repeat(a.batch, 1)

    host = [0.0]

    def run(n_new, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(vx, ids, attention_mask=am, max_new_tokens=n_new, eos_token_id=[], **dict({"do_sample": False}, **kw))
        host[0] = time.perf_counter() - t0          # the call has returned; with one new token and no EOS set nothing in it synchronises
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    run(16)                                   # warm-up: allocator, lazily-built folds, the graph capture path
    if proc_kw:
        run(16, **proc_kw)
    if lp_kw:
        run(16, **lp_kw)
    sample_kw = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    if a.sample:
        import aki_amd
        run(16, generator=torch.Generator(device=dev).manual_seed(0), **sample_kw)
        run(16, generator=aki_amd.DeviceGenerator(0), **sample_kw)
    con_kw = None
    if a.constraint:
        import numpy as np
        from aki_amd.constraint import TokenConstraint
        head = model.lang_model.get_output_embeddings()          # V': the logits' width
        V = int(head.max_original_id) + 1 + int(head.additional_out_features) if hasattr(head, "max_original_id") else int(head.out_features)
        nxt = np.full((16, V), -1, dtype=np.int32)
        for s_ in range(16):
            nxt[s_, s_::16] = (s_ + 1) % 16
        cyc = TokenConstraint.from_table(nxt, np.ones(16, dtype=bool))
        con_kw = dict(proc_kw, constraint=cyc if a.batch == 1 else [cyc] * a.batch)
        run(16, **con_kw)
    stop_kw = None
    if a.stop:                                # ids the plain run never emits: nothing matches, all a.new tokens are returned
        emitted = set(run(a.new)[1].flatten().tolist())
        stop_kw = dict(stop_sequences=never_matching_stops(emitted, model._logits_width(), 1)[0])
        run(16, **stop_kw)
    res = {"prompt_tokens_lm_stream": bench.N_TXT - 1 + bench.NV, "new_tokens": a.new, "fp8": bool(a.fp8), "mxfp4": bool(a.mxfp4), "w4_chain": bool(a.w4_chain), "rounds": []}
    if proc_kw:
        res["processors"] = proc_kw
    if a.sample:
        res["sampling"] = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    if a.batch > 1:
        res["batch"] = a.batch
    ref = ref_p = ref_s = None
    for _ in range(a.rounds):
        t1, _ = run(1)                        # prefill + first token
        h1 = host[0]
        tn, toks = run(a.new)
        assert toks.shape == (a.batch, a.new)
        if ref is None:
            ref = toks.clone()
        assert torch.equal(ref, toks), "generate is not reproducible from call to call"
        res["rounds"].append({"first_token_ms": round(t1 * 1e3, 2), "first_token_host_issue_ms": round(h1 * 1e3, 2), "total_ms": round(tn * 1e3, 2),
                              "ms_per_new_token_after_the_first": round((tn - t1) * 1e3 / (a.new - 1), 4),
                              "new_tokens_per_s_end_to_end": round(a.new / tn, 1)})
        if lp_kw:
            t1l, _ = run(1, **lp_kw)
            tnl, out_l = run(a.new, **lp_kw)
            assert torch.equal(out_l.sequences, ref), "generate with logprobs returns other tokens than without"
            assert out_l.logprobs.shape == (a.batch, a.new) and bool(torch.isfinite(out_l.logprobs).all())
            per_l = (tnl - t1l) * 1e3 / (a.new - 1)
            r = res["rounds"][-1]
            r["logprobs_ms_per_new_token_after_the_first"] = round(per_l, 4)
            r["logprobs_added_us_per_token"] = round((per_l - r["ms_per_new_token_after_the_first"]) * 1e3, 2)
        if stop_kw:
            t1s, _ = run(1, **stop_kw)
            tns, toks_s = run(a.new, **stop_kw)
            assert torch.equal(toks_s, ref), "generate with stops that never match returns other tokens than without"
            assert model.last_stop_hits.tolist() == [-1] * a.batch
            per_s = (tns - t1s) * 1e3 / (a.new - 1)
            r = res["rounds"][-1]
            r["stops_ms_per_new_token_after_the_first"] = round(per_s, 4)
            r["stops_added_us_per_token"] = round((per_s - r["ms_per_new_token_after_the_first"]) * 1e3, 2)
        if proc_kw:
            t1p, _ = run(1, **proc_kw)
            tnp, toks_p = run(a.new, **proc_kw)
            assert toks_p.shape == (a.batch, a.new)
            if ref_p is None:
                ref_p = toks_p.clone()
            assert torch.equal(ref_p, toks_p), "generate with processors is not reproducible from call to call"
            per_p = (tnp - t1p) * 1e3 / (a.new - 1)
            r = res["rounds"][-1]
            r["processed_ms_per_new_token_after_the_first"] = round(per_p, 4)
            r["processors_added_us_per_token"] = round((per_p - r["ms_per_new_token_after_the_first"]) * 1e3, 2)
        if con_kw:
            t1c, _ = run(1, **con_kw)
            tnc, toks_c = run(a.new, **con_kw)
            assert toks_c.shape == (a.batch, a.new) and bool((toks_c % 16 == torch.arange(a.new, device=dev)[None, :] % 16).all()), "not a walk of the cycle"
            per_c = (tnc - t1c) * 1e3 / (a.new - 1)
            r = res["rounds"][-1]
            r["constrained_ms_per_new_token_after_the_first"] = round(per_c, 4)
            base = r.get("processed_ms_per_new_token_after_the_first", r["ms_per_new_token_after_the_first"])
            r["constraint_added_us_per_token"] = round((per_c - base) * 1e3, 2)
        if a.sample:
            r = res["rounds"][-1]
            for leg, gen in (("torch_generator", lambda: torch.Generator(device=dev).manual_seed(0)), ("device_generator", lambda: aki_amd.DeviceGenerator(0))):
                t1s, _ = run(1, generator=gen(), **sample_kw)
                tns, toks_s = run(a.new, generator=gen(), **sample_kw)
                assert toks_s.shape == (a.batch, a.new)
                r[f"sample_{leg}_ms_per_new_token_after_the_first"] = round((tns - t1s) * 1e3 / (a.new - 1), 4)
            if ref_s is None:
                ref_s = toks_s.clone()
            assert torch.equal(ref_s, toks_s), "the device sampler is not reproducible from call to call"
            r["device_sampler_excess_over_greedy_us_per_token"] = round(
                (r["sample_device_generator_ms_per_new_token_after_the_first"] - r["ms_per_new_token_after_the_first"]) * 1e3, 2)
            r["device_sampler_faster_than_torch_path"] = bool(
                r["sample_device_generator_ms_per_new_token_after_the_first"] < r["sample_torch_generator_ms_per_new_token_after_the_first"])
    if a.num_return_sequences > 1:
        import aki_amd
        model.lang_model.share_prompt_kv = not a.no_share_prompt_kv
        nkw = dict(sample_kw, num_return_sequences=a.num_return_sequences)
        run(16, generator=aki_amd.DeviceGenerator(0), **nkw)
        res["num_return_sequences"] = {"n": a.num_return_sequences, "share_prompt_kv": not a.no_share_prompt_kv, "rounds": []}
        for _ in range(a.rounds):
            t1n, _ = run(1, generator=aki_amd.DeviceGenerator(0), **nkw)
            tnn, toks_n = run(a.new, generator=aki_amd.DeviceGenerator(0), **nkw)
            assert toks_n.shape == (a.batch * a.num_return_sequences, a.new)
            res["num_return_sequences"]["rounds"].append({"ms_per_new_token_after_the_first": round((tnn - t1n) * 1e3 / (a.new - 1), 4)})
    if a.sample:
        ex = sorted(r["device_sampler_excess_over_greedy_us_per_token"] for r in res["rounds"])
        res["device_sampler_excess_over_greedy_us_per_token_median"] = ex[len(ex) // 2]
    if proc_kw:
        add = sorted(r["processors_added_us_per_token"] for r in res["rounds"])
        res["processors_added_us_per_token_median"] = add[len(add) // 2]
    if lp_kw:
        add = sorted(r["logprobs_added_us_per_token"] for r in res["rounds"])
        plain = sorted(r["ms_per_new_token_after_the_first"] for r in res["rounds"])
        res["logprobs"] = {"top_logprobs": a.logprobs, "added_us_per_token_median": add[len(add) // 2], "added_us_per_token_min": add[0],
                           "added_us_per_token_max": add[-1], "plain_ms_per_token_median": plain[len(plain) // 2],
                           "plain_ms_per_token_min": plain[0], "plain_ms_per_token_max": plain[-1]}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "logprob_bench.json")
        book = json.load(open(path)) if os.path.exists(path) else {}
        book[f"batch{a.batch}_k{a.logprobs}"] = res
        with open(path, "w") as f:
            json.dump(book, f, indent=1, sort_keys=True)
            f.write("\n")
    if stop_kw:
        med = lambda k: sorted(r[k] for r in res["rounds"])[len(res["rounds"]) // 2]
        spread = lambda k: [min(r[k] for r in res["rounds"]), max(r[k] for r in res["rounds"])]
        res["stops"] = {"sequences": 8, "added_us_per_token_median": med("stops_added_us_per_token"),
                        "added_us_per_token_min_max": spread("stops_added_us_per_token"),
                        "plain_ms_per_token_median": med("ms_per_new_token_after_the_first"),
                        "plain_ms_per_token_min_max": spread("ms_per_new_token_after_the_first")}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stop_bench.json")
        book = json.load(open(path)) if os.path.exists(path) else {}
        book[f"batch{a.batch}"] = res
        with open(path, "w") as f:
            json.dump(book, f, indent=1, sort_keys=True)
            f.write("\n")
    if con_kw:
        med = lambda k: sorted(r[k] for r in res["rounds"])[len(res["rounds"]) // 2]
        spread = lambda k: [min(r[k] for r in res["rounds"]), max(r[k] for r in res["rounds"])]
        res["constraint"] = {"states": 16 * a.batch, "over": "processors" if proc_kw else "plain",
                             "added_us_per_token_median": med("constraint_added_us_per_token"),
                             "added_us_per_token_min_max": spread("constraint_added_us_per_token"),
                             "plain_ms_per_token_median": med("ms_per_new_token_after_the_first"),
                             "plain_ms_per_token_min_max": spread("ms_per_new_token_after_the_first")}
        if proc_kw:
            res["constraint"]["processed_ms_per_token_median"] = med("processed_ms_per_new_token_after_the_first")
            res["constraint"]["processed_ms_per_token_min_max"] = spread("processed_ms_per_new_token_after_the_first")
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "constraint_bench.json")
        book = json.load(open(path)) if os.path.exists(path) else {}
        book[f"batch{a.batch}"] = res
        with open(path, "w") as f:
            json.dump(book, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
