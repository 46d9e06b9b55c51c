#!/usr/bin/env python3
"""Chunked against sequential continuation of a cached sequence, on one MI355X.  Full AKI-4B language model (Phi-3.5-mini, random-init,
random prompt embeddings).  For every case a prompt of `cache` tokens is prefilled with room for T more, then T random tokens are
appended with Phi3ForCausalLM._continue - once with chunked_continue = True (one pass over the weights, ops.chunk_attn), once as T
teacher-forced decode steps.  Every timed call starts from the prompt's state (cache_len / host_len rewound: the K/V rows are simply
overwritten).  The two forms alternate inside ONE process; before anything is timed their logits are compared within the bf16 bar of two
routes of one step.  Timing: best of 5 x 10 calls (--groups x --calls; 5 x 2 for the sequential form at T >= 128), host wall clock around
synchronised groups.
    python tools/continue_bench.py [--cases 1:655:8,1:655:32,1:655:128,1:655:512,8:655:32] [--out profiles/continue_bench.json]
Under a time limit:  timeout -k 10 900 python tools/continue_bench.py --out profiles/continue_bench.json"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1:655:8,1:655:32,1:655:128,1:655:512,8:655:32", help="batch:cache:T, comma separated")
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from aki_amd import ops
    from aki_amd.factory import build_aki
    dev = torch.device("cuda", 0)
    model = build_aki(dtype=torch.bfloat16, device=dev, seed=0).eval()
    lm = model.lang_model
    d = lm.config.hidden_size
    res = {"device": torch.cuda.get_device_name(0), "rows": [],
           "timed": f"Phi3ForCausalLM._continue of T tokens from a cache, host wall clock, best of {a.groups} groups of {a.calls} calls "
                    "(sequential form at T >= 128: groups of 2), the two forms alternating group by group"}

    def run(cache, ids, start, host, flag, n):
        lm.chunked_continue = flag
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            cache.cache_len.copy_(start)
            cache.host_len = host
            out = lm._continue(ids, None, cache).logits
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, out

    with torch.no_grad():
        for spec in a.cases.split(","):
            B, L, T = (int(x) for x in spec.split(":"))
            g = torch.Generator(device=dev).manual_seed(B * 7919 + L + T)
            x = (torch.randn(B, L, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)
            table = ops.MaskTable.from_host([[(0, 0, 0, 0)]] * B, np.ones((B, L), dtype=bool), None, dev)
            cache = lm(inputs_embeds=x, attention_mask=table, use_cache=True, cache_capacity=L + T + 16, last_token_logits=True).past_key_values
            ids = torch.randint(3, 30000, (B, T), device=dev, generator=g)
            start, host = cache.cache_len.clone(), cache.host_len
            _, seq = run(cache, ids, start, host, False, 1)
            _, chk = run(cache, ids, start, host, True, 1)
            err = (chk.float() - seq.float()).abs().max().item()
            bar = 2e-2 * max(1.0, seq.float().abs().max().item())
            n_seq = a.calls if T < 128 else 2
            best = {True: float("inf"), False: float("inf")}
            for _ in range(a.groups):
                for flag in (True, False):
                    best[flag] = min(best[flag], run(cache, ids, start, host, flag, a.calls if flag else n_seq)[0])
            row = {"batch": B, "cache": L, "T": T, "chunked_ms": round(best[True], 3), "sequential_ms": round(best[False], 3),
                   "speedup": round(best[False] / best[True], 2), "logits_err": err, "logits_bar": bar, "within_bar": err <= bar}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
            del cache
            torch.cuda.empty_cache()
    lm.chunked_continue = False
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
