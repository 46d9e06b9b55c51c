#!/usr/bin/env python3
"""bf16 vs fp8 (e4m3) KV cache on one MI355X, one JSON line.  Full AKI-4B (random-init); for every batch B x prompt length L the decode
step of the language model (Phi-3.5-mini, random prompt embeddings) is captured with DecodeGraph and replayed, on the five-launch-per-layer
path, with a bf16 cache and with an fp8_e4m3 cache, the two alternating round by round; batch 1 also times the bf16 cache on the one-launch
decode chain (what an fp8 cache gives up there).  Then `AKI.generate(max_new_tokens=256)` at batch 16 and L = 655 (bench.py's batch: one
image per sample), both formats, timed as generate(256) - generate(1): the time of 255 decode tokens.
    python tools/kv_fp8_bench.py [--steps 32] [--rounds 2] [--batches 1,8,16] [--prompts 655,4096] [--new 256]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--prompts", default="655,4096")
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--gen-batch", type=int, default=16)
    a = ap.parse_args()
    import bench
    from aki_amd import ops
    from aki_amd.factory import build_aki
    from aki_amd.phi3 import DecodeGraph
    dev = torch.device("cuda", 0)
    model = build_aki(dtype=torch.bfloat16, device=dev, seed=0).eval()
    lm = model.lang_model
    d = lm.config.hidden_size
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "decode_step": [], "timed": "hipGraph replay of one "
           "decode step (no pick), host wall clock over the timed steps, best of the rounds; caches sized L + steps + 16"}

    def step_ms(B, L, kv, chain):
        lm.model.use_decode_chain = chain
        lm.set_kv_cache_dtype(kv)
        g = torch.Generator(device=dev).manual_seed(B * 7919 + L)
        x = (torch.randn(B, L, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)
        table = ops.MaskTable.from_host([[(0, 0, 0, 0)]] * B, np.ones((B, L), dtype=bool), None, dev)
        with torch.no_grad():
            out = lm(inputs_embeds=x, attention_mask=table, use_cache=True, cache_capacity=L + a.steps + 16, last_token_logits=True)
            cache = out.past_key_values
            ids = out.logits[:, -1].float().argmax(-1)
            st = DecodeGraph(lm, cache)
            for _ in range(3):
                ids = st.step(ids).argmax(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ids = st.step(ids).argmax(-1)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
        used_chain = getattr(cache, "chain", None) is not None
        nbytes = cache.nbytes()
        del st, cache, out
        lm.set_kv_cache_dtype("bf16")
        lm.model.use_decode_chain = True
        torch.cuda.empty_cache()
        return ms, nbytes, used_chain

    for L in [int(v) for v in a.prompts.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            modes = [("bf16", "bf16", False), ("fp8_e4m3", "fp8_e4m3", False)] + ([("bf16_chain", "bf16", True)] if B == 1 else [])
            best, mem = {}, {}
            for _ in range(a.rounds):
                for name, kv, chain in modes:
                    ms, nb, used = step_ms(B, L, kv, chain)
                    assert used == chain, (name, used)
                    best[name] = min(best.get(name, float("inf")), ms)
                    mem[name] = nb
            row = {"batch": B, "prompt": L, "ms_per_step": {k: round(v, 4) for k, v in best.items()},
                   "cache_GB": {k: round(mem[k] / 1e9, 3) for k in ("bf16", "fp8_e4m3")},
                   "fp8_speedup": round(best["bf16"] / best["fp8_e4m3"], 3)}
            if B == 1:
                row["fp8_vs_bf16_chain"] = round(best["bf16_chain"] / best["fp8_e4m3"], 3)
            res["decode_step"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)

    # AKI.generate, greedy, no EOS: 255 decode tokens = generate(new) - generate(1)
    vx, ids, am = bench.synth_batch(a.gen_batch, dev, torch.bfloat16, model.media_token_id, seed=1000)

    def gen_s(n_new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(vx, ids, attention_mask=am, max_new_tokens=n_new, do_sample=False, eos_token_id=[])
        torch.cuda.synchronize()
        assert toks.shape == (a.gen_batch, n_new)
        return time.perf_counter() - t0

    gen = {}
    for kv in ("bf16", "fp8_e4m3"):
        lm.set_kv_cache_dtype(kv)
        gen_s(16)                                   # warm-up: capture path, allocator
        lm.set_kv_cache_dtype("bf16")
    for _ in range(a.rounds):
        for kv in ("bf16", "fp8_e4m3"):
            lm.set_kv_cache_dtype(kv)
            t1, tn = gen_s(1), gen_s(a.new)
            lm.set_kv_cache_dtype("bf16")
            ms_tok = (tn - t1) * 1e3 / (a.new - 1)
            gen[kv] = min(gen.get(kv, float("inf")), ms_tok)
    res["generate"] = {"batch": a.gen_batch, "new_tokens": a.new, "lm_stream_length": int(bench.N_TXT - 1 + bench.NV),
                       "ms_per_token": {k: round(v, 4) for k, v in gen.items()}, "fp8_speedup": round(gen["bf16"] / gen["fp8_e4m3"], 3),
                       "timed": "(generate(new) - generate(1)) / (new - 1), host wall clock, best of the rounds"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
