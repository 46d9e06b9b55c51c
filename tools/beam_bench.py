#!/usr/bin/env python3
"""Beam search: the host loop (AKI._beam_search) against the device path (AKI._beam_search_device, lang_model.device_beam_search), on
one MI355X.  Full AKI-4B (random-init), the benchmark's prompt (a language-model stream of 655), 64 new tokens, no EOS.  The two forms
alternate round by round in ONE process (boxes differ by up to 5 %); ms per token is (generate(new) - generate(1)) / (new - 1), so the
prefill and the expansion to K beams cancel.  Also timed, with events around the launch alone: ops.kv_beam_reorder over a cache of the
same shape with `--suffix` rows written since the prefill and a random parent map with repeats.
    python tools/beam_bench.py [--rounds 3] [--new 64] [--settings 4x1,4x4,2x8] [--suffix 32] [--out profiles/beam_bench.json]
A setting is KxB.  One setting per process:  --settings 4x1  (also the form to put after `rocprofv3 --kernel-trace --stats --`)."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--settings", default="4x1,4x4,2x8")
    ap.add_argument("--suffix", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bench
    from aki_amd import ops
    from aki_amd.factory import build_aki
    dev = torch.device("cuda", 0)
    model = build_aki(dtype=torch.bfloat16, device=dev, seed=0).eval()
    lm = model.lang_model
    cfg = lm.config
    H, Dh, n_layers = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads, cfg.num_hidden_layers
    L = int(bench.N_TXT - 1 + bench.NV)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "new_tokens": a.new, "lm_stream_length": L, "settings": [],
           "timed": "AKI.generate(num_beams=K, eos_token_id=[]) host wall clock, (new tokens - 1 token) / (new - 1), median of the rounds, the "
                    "forms alternating; reorder: HIP events around ops.kv_beam_reorder alone, median of 20 launches"}

    def gen_s(vx, ids, am, K, n_new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(vx, ids, attention_mask=am, max_new_tokens=n_new, num_beams=K, eos_token_id=[])
        torch.cuda.synchronize()
        assert toks.shape == (ids.shape[0], n_new)
        return time.perf_counter() - t0

    def reorder_ms(K, B):
        cap = L + a.new
        tensors = [torch.zeros((B * K, H, cap, Dh), dtype=torch.bfloat16, device=dev) for _ in range(2 * n_layers)]
        table = ops.KVBeamTable(tensors)
        start = torch.full((B * K,), L, dtype=torch.int32, device=dev)
        length = start + a.suffix
        g = torch.Generator().manual_seed(K * 100 + B)
        parent = (torch.arange(B * K) // K * K + torch.randint(0, K, (B * K,), generator=g)).to(torch.int32).to(dev)
        times = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.kv_beam_reorder(table, parent, start, length, K, L, L + a.suffix)
            e1.record()
            e1.synchronize()
            if i >= 3:
                times.append(e0.elapsed_time(e1))
        del tensors, table
        torch.cuda.empty_cache()
        return statistics.median(times)

    for setting in [s for s in a.settings.split(",") if s]:
        K, B = (int(v) for v in setting.split("x"))
        vx, ids, am = bench.synth_batch(B, dev, torch.bfloat16, model.media_token_id, seed=1000)
        runs = {"host": [], "device": []}
        for name in runs:                                   # warm-up: allocator pools, lazily-set kernel attributes
            lm.device_beam_search = name == "device"
            gen_s(vx, ids, am, K, 9)
        for _ in range(a.rounds):
            for name in runs:
                lm.device_beam_search = name == "device"
                t1, tn = gen_s(vx, ids, am, K, 1), gen_s(vx, ids, am, K, a.new)
                runs[name].append((tn - t1) * 1e3 / (a.new - 1))
        lm.device_beam_search = type(lm).device_beam_search
        med = {k: statistics.median(v) for k, v in runs.items()}
        row = {"num_beams": K, "batch": B, "ms_per_token": {k: round(v, 4) for k, v in med.items()},
               "ms_per_token_rounds": {k: [round(x, 4) for x in v] for k, v in runs.items()},
               "device_speedup": round(med["host"] / med["device"], 3),
               "reorder_ms": round(reorder_ms(K, B), 4), "reorder_suffix_rows": a.suffix}
        res["settings"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
