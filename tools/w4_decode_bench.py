#!/usr/bin/env python3
"""Decode step time with bf16, e4m3 (enable_fp8) and MXFP4 (enable_mxfp4) weights on one MI355X -> profiles/w4_decode_bench.json.

Phi-3.5-mini's dimensions, 32 layers, random-init N(0, 0.02), random prompt embeddings.  For every (batch, prompt) shape ONE child process
builds the model once and alternates the weight formats round by round (boxes differ by up to 5 %, so formats are only compared inside a
process): the decode step is captured with DecodeGraph and replayed, host wall clock over the timed steps, best of the rounds.  All formats
run the five-launch-per-layer path; batch 1 also runs the one-launch chain where one exists (bf16, e4m3) - the honest comparisons for MXFP4
are against e4m3 on five launches AND against the e4m3 chain.  One more child records the quality figure once: relative L2 of the
last-token decode logits with MXFP4 (and, for scale, e4m3) weights against bf16 weights at full depth, prompt 655, from identical bf16
prefills.  Every child runs under its own time limit; the first one that fails ends the run.
    python tools/w4_decode_bench.py [--steps 32] [--rounds 3] [--shapes 1x655,8x655,16x655,16x4096] [--out profiles/w4_decode_bench.json]
--chain: the batch-1 question only -> profiles/w4_chain_bench.json.  One child alternates FOUR legs at batch 1, prompt 655: the bf16 chain, the
e4m3 chain, MXFP4 on five launches per layer and the MXFP4 chain (Phi3Model.decode_chain_w4); the logits of the MXFP4 chain's first steps are
checked against MXFP4 on five launches, bit for bit.
    python tools/w4_decode_bench.py --chain [--steps 32] [--rounds 3]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_lm(layers):
    import torch
    from aki_amd.phi3 import Phi3ForCausalLM, make_phi3_config
    torch.manual_seed(0)
    with torch.device("cuda"):
        lm = Phi3ForCausalLM(make_phi3_config(num_hidden_layers=layers))
    for p in lm.parameters():
        p.data.normal_(0, 0.02)
    return lm.to(torch.bfloat16).eval()


def set_format(lm, fmt):
    lm.enable_mxfp4(fmt == "mxfp4")
    lm.enable_fp8(fmt == "e4m3")


def prefill(lm, B, L, capacity):
    import numpy as np
    import torch
    from aki_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B * 7919 + L)
    x = (torch.randn(B, L, lm.config.hidden_size, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    table = ops.MaskTable.from_host([[(0, 0, 0, 0)]] * B, np.ones((B, L), dtype=bool), None, torch.device("cuda", 0))
    return lm(inputs_embeds=x, attention_mask=table, use_cache=True, cache_capacity=capacity, last_token_logits=True)


def child_shape(a, B, L):
    import torch
    from aki_amd.phi3 import DecodeGraph
    lm = build_lm(a.layers)
    modes = [("bf16", "bf16", False), ("e4m3", "e4m3", False), ("mxfp4", "mxfp4", False)]
    if B == 1:
        modes += [("bf16_chain", "bf16", True), ("e4m3_chain", "e4m3", True)]
    best = {}
    with torch.no_grad():
        for _ in range(a.rounds):
            for name, fmt, chain in modes:
                set_format(lm, None)
                lm.model.use_decode_chain = chain
                out = prefill(lm, B, L, L + a.steps + 16)              # always the bf16 prefill: the same cache content for every format
                cache = out.past_key_values
                ids = out.logits[:, -1].float().argmax(-1)
                set_format(lm, fmt)
                st = DecodeGraph(lm, cache)
                for _ in range(3):
                    ids = st.step(ids).argmax(-1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ids = st.step(ids).argmax(-1)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
                assert (getattr(cache, "chain", None) is not None) == chain, name
                best[name] = min(best.get(name, float("inf")), ms)
                del st, cache, out
                torch.cuda.empty_cache()
    row = {"batch": B, "prompt": L, "ms_per_step": {k: round(v, 4) for k, v in best.items()},
           "mxfp4_vs_e4m3_five_launches": round(best["e4m3"] / best["mxfp4"], 3), "mxfp4_vs_bf16_five_launches": round(best["bf16"] / best["mxfp4"], 3)}
    if B == 1:
        row["mxfp4_vs_e4m3_chain"] = round(best["e4m3_chain"] / best["mxfp4"], 3)
    print("ROW " + json.dumps(row), flush=True)


def child_chain(a):
    """Batch 1, prompt 655: bf16 chain | e4m3 chain | MXFP4 on five launches | MXFP4 chain, alternating."""
    import torch
    from aki_amd.phi3 import DecodeGraph
    B, L = 1, a.prompt
    lm = build_lm(a.layers)
    legs = [("bf16_chain", "bf16", True, False), ("e4m3_chain", "e4m3", True, False), ("mxfp4", "mxfp4", False, False),
            ("mxfp4_chain", "mxfp4", True, True)]
    best, first = {}, {}
    with torch.no_grad():
        for _ in range(a.rounds):
            for name, fmt, chain, w4c in legs:
                set_format(lm, None)
                lm.model.use_decode_chain = True
                lm.model.decode_chain_w4 = w4c
                out = prefill(lm, B, L, L + a.steps + 16)              # always the bf16 prefill: the same cache content for every leg
                cache = out.past_key_values
                ids = out.logits[:, -1].float().argmax(-1)
                set_format(lm, fmt)
                st = DecodeGraph(lm, cache)
                head = []
                for _ in range(3):
                    lg = st.step(ids)
                    head.append(lg.clone())
                    ids = lg.argmax(-1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ids = st.step(ids).argmax(-1)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
                assert (getattr(cache, "chain", None) is not None) == chain, name
                if chain:
                    cache.chain.check()
                    assert cache.chain.fmt == {"bf16": "bf16", "e4m3": "w8", "mxfp4": "w4"}[fmt], name
                first.setdefault(name, torch.stack(head))
                best[name] = min(best.get(name, float("inf")), ms)
                del st, cache, out
                torch.cuda.empty_cache()
    bad = {k: int((v != first["mxfp4"]).sum()) for k, v in first.items() if k.startswith("mxfp4_chain")}
    assert not any(bad.values()), f"MXFP4 chain logits differ from MXFP4 on five launches: {bad}"
    row = {"batch": B, "prompt": L, "ms_per_step": {k: round(v, 4) for k, v in best.items()},
           "library": "product",
           "mxfp4_chain_logits_differing_from_five_launches": bad,
           "mxfp4_chain_vs_mxfp4_five_launches": round(best["mxfp4"] / best["mxfp4_chain"], 3),
           "mxfp4_chain_vs_e4m3_chain": round(best["e4m3_chain"] / best["mxfp4_chain"], 3),
           "mxfp4_chain_beats_e4m3_chain": bool(best["mxfp4_chain"] < best["e4m3_chain"])}
    print("ROW " + json.dumps(row), flush=True)


def child_quality(a):
    import torch
    lm = build_lm(a.layers)
    lm.model.use_decode_chain = False
    logits = {}
    with torch.no_grad():
        for fmt in ("bf16", "e4m3", "mxfp4"):
            set_format(lm, None)
            out = prefill(lm, 1, 655, 655 + 16)
            ids = out.logits[:, -1].float().argmax(-1)
            set_format(lm, fmt)
            logits[fmt] = lm.decode_step(input_ids=ids, past_key_values=out.past_key_values)[0].float()
    ref = logits["bf16"]
    row = {"layers": a.layers, "prompt": 655, "weights": "random-init N(0, 0.02): the worst case for 4-bit rounding",
           "rel_l2_mxfp4_vs_bf16": round(float((logits["mxfp4"] - ref).norm() / ref.norm()), 4),
           "rel_l2_e4m3_vs_bf16": round(float((logits["e4m3"] - ref).norm() / ref.norm()), 4),
           "argmax_agrees": {k: bool(logits[k].argmax() == ref.argmax()) for k in ("e4m3", "mxfp4")}}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--shapes", default="1x655,8x655,16x655,16x4096")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w4_decode_bench.json"))
    ap.add_argument("--chain", action="store_true", help="batch 1 only: bf16 chain, e4m3 chain, MXFP4 on five launches, MXFP4 chain -> profiles/w4_chain_bench.json")
    ap.add_argument("--prompt", type=int, default=655, help="with --chain: the prompt length")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three rounds")
    if a.child == "quality":
        return child_quality(a)
    if a.child == "chain":
        return child_chain(a)
    if a.chain:
        return main_chain(a)
    if a.child:
        B, L = (int(v) for v in a.child.split("x"))
        return child_shape(a, B, L)
    res = {"steps": a.steps, "rounds": a.rounds, "layers": a.layers, "timed": "hipGraph replay of one decode step (no pick), host wall clock over "
           "the timed steps, best of the rounds, formats alternating inside one process per shape; five launches per layer unless the name says chain",
           "decode_step": [], "quality": None}
    for job in a.shapes.split(",") + ["quality"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", job, "--steps", str(a.steps), "--rounds", str(a.rounds), "--layers", str(a.layers)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{job}: no result within {a.limit} s - stopping")
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"{job}: exit status {r.returncode} - stopping")
        row = json.loads(rows[-1])
        print(json.dumps(row), file=sys.stderr, flush=True)
        if job == "quality":
            res["quality"] = row
        else:
            res["decode_step"].append(row)
        with open(a.out, "w") as f:                       # after every child: what was measured so far survives a later failure
            json.dump(res, f, indent=1)
            f.write("\n")
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main_chain(a):
    out = a.out if a.out != os.path.join(ROOT, "profiles", "w4_decode_bench.json") else os.path.join(ROOT, "profiles", "w4_chain_bench.json")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "chain", "--steps", str(a.steps), "--rounds", str(a.rounds), "--layers", str(a.layers),
           "--prompt", str(a.prompt)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"chain: no result within {a.limit} s - stopping")
    rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
    if r.returncode != 0 or not rows:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"chain: exit status {r.returncode} - stopping")
    import torch
    res = {"steps": a.steps, "rounds": a.rounds, "layers": a.layers, "timed": "hipGraph replay of one decode step (no pick), host wall clock over the "
           "timed steps, best of the rounds, all legs alternating inside ONE process", "device": torch.cuda.get_device_name(0), "batch_1": json.loads(rows[-1])}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
