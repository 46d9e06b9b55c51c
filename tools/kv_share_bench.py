#!/usr/bin/env python3
"""Shared against replicated prompt K/V for N sampled continuations per prompt, on one MI355X.  Full AKI-4B (random-init).  For every
N x prompt length L one prompt of the language model (Phi-3.5-mini, random prompt embeddings) is prefilled, its cache is expanded to N rows
either with AkiKVCache.share_prefix (one copy of the prompt rows, decode_attn_group_kernel) or with select_rows (N copies, the fused
split-KV kernel), the decode step is captured with DecodeGraph and replayed.  The two forms alternate round by round in ONE process; before
anything is timed their first-step logits are compared within the bf16 decode bar.  Reported: ms per replayed step (median of the rounds,
and every round, so the run-to-run spread is in the file), cache bytes, and `AKI.generate(num_return_sequences=N)` ms per token.
    python tools/kv_share_bench.py [--steps 32] [--rounds 3] [--ns 2,4,8,16] [--prompts 655,4096] [--new 128] [--out profiles/kv_share_bench.json]
Every GPU step under its own time limit, chained, then merged into the committed file (`--merge` touches no GPU):
    timeout -k 10 600 python tools/kv_share_bench.py --no-generate --out /tmp/kvs_steps.json && \
    timeout -k 10 600 python tools/kv_share_bench.py --prompts "" --out /tmp/kvs_gen.json && \
    python tools/kv_share_bench.py --merge /tmp/kvs_steps.json /tmp/kvs_gen.json --out profiles/kv_share_bench.json
One sweep point per process:  --ns 16 --prompts 4096 --no-generate  (also the form to put after `rocprofv3 --kernel-trace --stats --`)."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ns", default="2,4,8,16")
    ap.add_argument("--prompts", default="655,4096")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", nargs="+", default=None, help="JSON files written by earlier runs: their decode_step / generate rows are joined")
    a = ap.parse_args()
    if a.merge:
        res = {}
        for f in a.merge:
            part = json.load(open(f))
            for k, v in part.items():
                if isinstance(v, list) and isinstance(res.get(k), list):
                    res[k] = res[k] + v
                else:
                    res.setdefault(k, v)
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    import bench
    import aki_amd
    from aki_amd import ops
    from aki_amd.factory import build_aki
    from aki_amd.phi3 import DecodeGraph
    dev = torch.device("cuda", 0)
    model = build_aki(dtype=torch.bfloat16, device=dev, seed=0).eval()
    lm = model.lang_model
    d = lm.config.hidden_size
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "decode_step": [],
           "timed": "hipGraph replay of one decode step (no pick) at batch N, host wall clock over the timed steps; median of the rounds, "
                    "the forms alternating; caches sized L + steps + 16"}

    def prefilled(N, L, shared):
        g = torch.Generator(device=dev).manual_seed(N * 7919 + L)
        x = (torch.randn(1, L, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)
        table = ops.MaskTable.from_host([[(0, 0, 0, 0)]], np.ones((1, L), dtype=bool), None, dev)
        out = lm(inputs_embeds=x, attention_mask=table, use_cache=True, cache_capacity=L + a.steps + 16, last_token_logits=True)
        cache = out.past_key_values
        if shared:
            cache.share_prefix(N)
        else:
            cache.select_rows(torch.zeros(N, dtype=torch.long, device=dev))
        ids = (out.logits[:, -1].float().argmax(-1) + torch.arange(N, device=dev)) % (out.logits.shape[-1] - 1)     # N different first tokens
        return cache, ids

    def step_ms(N, L, shared):
        with torch.no_grad():
            cache, ids = prefilled(N, L, shared)
            st = DecodeGraph(lm, cache)
            first = st.step(ids).float().clone()
            ids = first.argmax(-1)
            for _ in range(2):
                ids = st.step(ids).argmax(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ids = st.step(ids).argmax(-1)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
        nbytes = cache.nbytes()
        del st, cache
        torch.cuda.empty_cache()
        return ms, nbytes, first

    def first_logits(N, L, shared):
        with torch.no_grad():
            cache, ids = prefilled(N, L, shared)
            lg = lm.decode_step(input_ids=ids, past_key_values=cache).float().clone()
        del cache
        torch.cuda.empty_cache()
        return lg

    for L in [int(v) for v in a.prompts.split(",") if v]:
        for N in [int(v) for v in a.ns.split(",")]:
            runs, mem = {"shared": [], "replicated": []}, {}
            ls, lr = first_logits(N, L, True), first_logits(N, L, False)      # checked against each other before anything is timed
            err, bar = (ls - lr).abs().max().item(), 2e-2 * max(1.0, lr.abs().max().item())
            assert err <= bar, f"N {N} L {L}: the two forms' logits differ by {err:.3g} (bar {bar:.3g})"
            for _ in range(a.rounds):
                for name in ("shared", "replicated"):
                    ms, nb, lg = step_ms(N, L, name == "shared")
                    runs[name].append(ms)
                    mem[name] = nb
            med = {k: statistics.median(v) for k, v in runs.items()}
            row = {"n": N, "prompt": L, "ms_per_step": {k: round(v, 4) for k, v in med.items()},
                   "ms_per_step_rounds": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                   "spread_ms": round(max(max(v) - min(v) for v in runs.values()), 4),
                   "cache_GB": {k: round(v / 1e9, 3) for k, v in mem.items()}, "shared_speedup": round(med["replicated"] / med["shared"], 3)}
            res["decode_step"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)

    if not a.no_generate:
        vx, ids, am = bench.synth_batch(1, dev, torch.bfloat16, model.media_token_id, seed=1000)
        res["generate"] = []
        for N in [int(v) for v in a.ns.split(",")]:
            def gen_s(n_new):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks = model.generate(vx, ids, attention_mask=am, max_new_tokens=n_new, do_sample=True, temperature=1.0, top_k=50,
                                      generator=aki_amd.DeviceGenerator(0), num_return_sequences=N, eos_token_id=[])
                torch.cuda.synchronize()
                assert toks.shape == (N, n_new)
                return time.perf_counter() - t0
            runs = {"shared": [], "replicated": []}
            for name in runs:
                lm.share_prompt_kv = name == "shared"
                gen_s(16)
            for _ in range(a.rounds):
                for name in runs:
                    lm.share_prompt_kv = name == "shared"
                    t1, tn = gen_s(1), gen_s(a.new)
                    runs[name].append((tn - t1) * 1e3 / (a.new - 1))
            lm.share_prompt_kv = type(lm).share_prompt_kv
            res["generate"].append({"n": N, "new_tokens": a.new, "lm_stream_length": int(bench.N_TXT - 1 + bench.NV),
                                    "ms_per_token": {k: round(statistics.median(v), 4) for k, v in runs.items()},
                                    "ms_per_token_rounds": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
