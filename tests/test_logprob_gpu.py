"""Per-token log-probabilities on the GPU: the kernel (ops.token_logprob) against the float64 reference of logprob_cases in both of its
forms, generate's two new keywords in every decoding mode on the tiny model, and AkiMethods.score against full forwards.

The calls that pass the new keywords build them in a dict outside the call (test_every_generate_caller_in_the_repository_passes_known_keywords
reads the text of every generate call against a fixed list)."""
import numpy as np
import pytest
import torch

import logprob_cases as LC
from golden import gen
from test_model_gpu import DEV, batch, build_tiny

pytestmark = pytest.mark.gpu

BF16_ROUTE_BAR = 2e-2          # the project's bar for two bf16 routes on the tiny model, times max(1, max |logits|)
FP32_LOGIT_BAR = 1e-5          # the project's fp32 logit bar, times max(1, max |logits|)


def _layout(x, dtype, stride):
    """x f32 numpy [rows, V] -> a device tensor view [rows, V] of `dtype` with the row stride the name asks for."""
    rows, V = x.shape
    ld = {"dense": V, "plus5": V + 5, "aligned": (V + 7) // 8 * 8 + 8}[stride]
    buf = torch.full((rows, ld), 3.0, dtype=dtype, device=DEV)         # the padding holds large values: reading it would show
    buf[:, :V] = torch.from_numpy(x).to(DEV).to(dtype)
    return buf[:, :V]


def _check(name, got, ref, k):
    """got: the kernel's (logprob [rows], top ids [rows, k], top logprobs [rows, k]) tensors; ref: LC.reference's tuple.  Returns the worst
    error / bound."""
    lp, top_ids, top_lp, bound = ref
    g_lp = got[0].double().cpu().numpy()
    inf = np.isneginf(lp)
    assert np.array_equal(np.isneginf(g_lp), inf), f"{name}: -inf logprobs differ"
    err = np.where(inf, 0.0, np.abs(g_lp - np.where(inf, 0.0, lp)))
    worst = float((err / bound).max())
    assert (err <= bound).all(), f"{name}: logprob error {err.max():.3g} over the bound {bound.min():.3g} (x{worst:.2f})"
    if k:
        assert np.array_equal(got[1].cpu().numpy(), top_ids), f"{name}: ranked ids differ"
        g_top = got[2].double().cpu().numpy()
        tinf = np.isneginf(top_lp)
        assert np.array_equal(np.isneginf(g_top), tinf), f"{name}: -inf top logprobs differ"
        terr = np.where(tinf, 0.0, np.abs(g_top - np.where(tinf, 0.0, top_lp)))
        assert (terr <= bound[:, None]).all(), f"{name}: top logprob error {terr.max():.3g} over the bound"
        worst = max(worst, float((terr / bound[:, None]).max()))
    return worst


@pytest.mark.parametrize("stride", ["dense", "plus5", "aligned"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_kernel_against_float64(name, dtype, stride):
    from aki_amd import ops
    x, ids = LC.make(name)
    logits = _layout(x, dtype, stride)
    ids_t = torch.from_numpy(ids).to(DEV)
    for k in LC.TOP_KS:
        first = ops.token_logprob(logits, ids=ids_t, top_k=k)
        again = ops.token_logprob(logits, ids=ids_t, top_k=k)
        assert first[0].shape == (x.shape[0], 1) and (first[1] is None) == (k == 0)
        for a, b in zip(first, again):
            assert a is None and b is None or torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                          b.view(torch.int32) if b.dtype == torch.float32 else b), "not bit-equal on a second call"
        got = (first[0][:, 0], None if k == 0 else first[1][:, 0], None if k == 0 else first[2][:, 0])
        worst = _check(f"{name} {dtype} {stride} k={k}", got, LC.reference(x, ids, k), k)
        print(f"token_logprob {name} {str(dtype)[6:]} {stride} k={k}: worst error / bound = {worst:.3f}")


def test_kernel_plain_form_skip_step_and_bad_ids():
    """skip rows write the skipped values; `step` selects the column; an id outside [0, V) writes NaN; untouched columns stay as they were."""
    from aki_amd import ops
    x, _ = LC.make("v1025_m80")
    x = x[:4]
    V = x.shape[1]
    logits = _layout(x, torch.bfloat16, "dense")
    ids = torch.tensor([3, V, -1, V - 1], dtype=torch.long, device=DEV)
    skip = torch.tensor([0, 0, 0, 1], dtype=torch.uint8, device=DEV)
    out = torch.full((4, 3), float("nan"), device=DEV)
    top_ids = torch.full((4, 3, 8), -7, dtype=torch.long, device=DEV)
    top_lp = torch.full((4, 3, 8), float("nan"), device=DEV)
    ops.token_logprob(logits, ids=ids, skip=skip, step=1, top_k=8, out_logprob=out, out_top_ids=top_ids, out_top_logprobs=top_lp)
    assert torch.isnan(out[:, 0]).all() and torch.isnan(out[:, 2]).all() and (top_ids[:, [0, 2]] == -7).all() and torch.isnan(top_lp[:, [0, 2]]).all()
    assert torch.isnan(out[1, 1]) and torch.isnan(out[2, 1]) and out[3, 1] == 0 and (top_ids[3, 1] == -1).all() and (top_lp[3, 1] == 0).all()
    ref = LC.reference(x[:3], np.array([3, 0, 0]), 8)
    _check("row 0", (out[:1, 1], top_ids[:1, 1], top_lp[:1, 1]), tuple(r[:1] for r in ref), 8)
    _check("tops of the rows with a bad id", (torch.from_numpy(ref[0][1:3]).to(DEV), top_ids[1:3, 1], top_lp[1:3, 1]), tuple(r[1:3] for r in ref), 8)
    ops.token_logprob(logits, ids=ids, step=3, top_k=8, out_logprob=out, out_top_ids=top_ids, out_top_logprobs=top_lp)      # outside the 3 columns
    assert torch.isnan(out[:, 2]).all() and (top_ids[:, 2] == -7).all()


def test_kernel_in_loop_form_scripted():
    """B = 3, 4 steps, the state advanced by hand as the pick does: row 1 picks its EOS at step 1, row 0 and 2 start at non-zero lengths."""
    from aki_amd import ops
    B, steps, V, k, pad = 3, 4, 1025, 2, 7
    rng = np.random.default_rng(5)
    xs = [LC.bf16_exact(rng.standard_normal((B, V)).astype(np.float32) * 4) for _ in range(steps)]
    picked = rng.integers(0, V, size=(B, steps))
    picked[1, 2:] = pad                                                # behind its EOS the row carries pad tokens
    start_len = torch.tensor([5, 0, 7], dtype=torch.int32, device=DEV)
    cache_len = start_len.clone()
    done_at = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tokens = torch.full((B, steps), pad, dtype=torch.long, device=DEV)
    guard = torch.full((B * steps * (1 + 2 * k) + 64,), float("nan"), device=DEV)
    out = guard[16:16 + B * steps].view(B, steps)
    top_lp = guard[32 + B * steps:32 + B * steps * (1 + k)].view(B, steps, k)
    top_ids = torch.full((B, steps, k), -7, dtype=torch.long, device=DEV)
    narrow = torch.full((B, 2), float("nan"), device=DEV)              # two columns only: steps 2 and 3 fall outside and write nothing
    for s in range(steps):
        tokens[:, s] = torch.from_numpy(picked[:, s]).to(DEV)          # what the pick does before the log-probability launch
        cache_len.copy_(start_len + s)
        if s == 1:
            done_at[1] = 1
        lg = torch.from_numpy(xs[s]).to(DEV).to(torch.bfloat16)
        loop = dict(tokens=tokens, cache_len=cache_len, start_len=start_len, done_at=done_at)
        ops.token_logprob(lg, top_k=k, out_logprob=out, out_top_ids=top_ids, out_top_logprobs=top_lp, **loop)
        ops.token_logprob(lg, out_logprob=narrow, **loop)
    torch.cuda.synchronize()
    for s in range(steps):
        ref = LC.reference(xs[s], picked[:, s], k)
        live = [0, 2] if s >= 2 else [0, 1, 2]                         # the EOS step itself (s == 1) is scored
        _check(f"step {s}", (out[live, s], top_ids[live, s], top_lp[live, s]), tuple(r[live] for r in ref), k)
        if s < 2:
            _check(f"narrow step {s}", (narrow[:, s], None, None), ref, 0)
    assert (out[1, 2:] == 0).all() and (top_ids[1, 2:] == -1).all() and (top_lp[1, 2:] == 0).all()
    used = torch.zeros_like(guard, dtype=torch.bool)
    used[16:16 + B * steps] = True
    used[32 + B * steps:32 + B * steps * (1 + k)] = True
    assert torch.isnan(guard[~used]).all(), "something outside the outputs was written"
    assert not torch.isnan(guard[used]).any()


# ---- generate -------------------------------------------------------------------------------------------------------------------------
N_NEW = 8


@pytest.fixture(scope="module")
def tiny_bf16():
    m, g = build_tiny(torch.bfloat16)
    vx, lx, am, _ = batch(g, torch.bfloat16)
    rows = [0, 3]                                                      # both hold <image> and 32001; the second is right-padded by three
    assert int(am[3].sum()) < am.shape[1] == int(am[0].sum())
    return m, vx[rows], lx[rows], am[rows]


@pytest.fixture(scope="module")
def tiny_f32():
    m, g = build_tiny(torch.float32)
    vx, lx, am, _ = batch(g, torch.float32)
    rows = [0, 3]
    return m, vx[rows], lx[rows], am[rows]


class _Recorder:
    """Records the logits of the prefill and of every lang_model.decode_step while it is installed."""

    def __init__(self, m, monkeypatch):
        self.logits = []
        prefill, step = m._prefill_prompt, m.lang_model.decode_step

        def rec_prefill(*a, **kw):
            out = prefill(*a, **kw)
            self.logits.append(out[1].clone())
            return out

        def rec_step(*a, **kw):
            out = step(*a, **kw)
            self.logits.append(out.clone())
            return out

        monkeypatch.setattr(m, "_prefill_prompt", rec_prefill)
        monkeypatch.setattr(m.lang_model, "decode_step", rec_step)


def _ref_from_logits(logits, tokens, k):
    """The float64 reference for recorded logits (a list of [rows, V] tensors, one per step) at `tokens` [rows, steps]."""
    out = []
    for t, lg in enumerate(logits):
        out.append(LC.reference(lg.float().cpu().numpy(), tokens[:, t].cpu().numpy(), k))
    return out


def _host_run(m, vx, lx, am, monkeypatch, k=8, **mode):
    rec = _Recorder(m, monkeypatch)
    opts = dict(output_logprobs=True, top_logprobs=k, use_graph=False, max_new_tokens=N_NEW, eos_token_id=[], **mode)
    out = m.generate(vx, lx, attention_mask=am, **opts)
    monkeypatch.undo()
    return out, rec.logits


def test_generate_host_loop_against_float64_of_its_own_logits(tiny_bf16, monkeypatch):
    m, vx, lx, am = tiny_bf16
    out, logits = _host_run(m, vx, lx, am, monkeypatch)
    plain = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], use_graph=False)
    assert torch.equal(out.sequences, plain) and len(logits) == N_NEW
    assert out.logprobs.shape == (2, N_NEW) and out.top_token_ids.shape == (2, N_NEW, 8) == out.top_logprobs.shape
    assert out.logprobs.dtype == torch.float32 and out.top_token_ids.dtype == torch.long and out.logprobs.is_cuda
    for t, ref in enumerate(_ref_from_logits(logits, out.sequences, 8)):
        worst = _check(f"host loop step {t}", (out.logprobs[:, t], out.top_token_ids[:, t], out.top_logprobs[:, t]), ref, 8)
        print(f"generate host loop step {t}: worst error / bound = {worst:.3f}")
    assert torch.equal(out.top_token_ids[..., 0], out.sequences) and torch.equal(out.top_logprobs[..., 0], out.logprobs)      # greedy: the token is rank 0


def _modes():
    from aki_amd import DeviceGenerator
    return {
        "greedy": lambda: dict(use_graph=True),
        "processed": lambda: dict(use_graph=True, repetition_penalty=1.3, no_repeat_ngram_size=2),
        "sampler": lambda: dict(use_graph=True, do_sample=True, temperature=0.9, top_k=40, top_p=0.95, generator=DeviceGenerator(11)),
        "n_ret": lambda: dict(use_graph=True, do_sample=True, num_return_sequences=2, generator=DeviceGenerator(12)),
        "sampler_host": lambda: dict(use_graph=False, do_sample=True, temperature=0.9, top_k=40, generator=DeviceGenerator(13)),
        "torch_sampling": lambda: dict(use_graph=True, do_sample=True, top_k=40, generator=torch.Generator(device=DEV).manual_seed(3)),
    }


@pytest.mark.parametrize("mode", ["greedy", "processed", "sampler", "n_ret", "sampler_host", "torch_sampling"])
def test_generate_modes_return_the_same_tokens_with_logprobs(tiny_bf16, mode):
    """Every mode: sequences bit-equal to the call without the keywords; logprobs are those of the raw distribution at the returned token
    (so <= the best alternative, which a processed or sampled token need not be); the ranked alternatives descend."""
    m, vx, lx, am = tiny_bf16
    make = _modes()[mode]
    plain = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], **make())
    opts = dict(make(), output_logprobs=True, top_logprobs=3)
    out = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], **opts)
    rows = plain.shape[0]
    assert rows == (4 if mode == "n_ret" else 2) and torch.equal(out.sequences, plain)
    assert out.logprobs.shape == (rows, N_NEW) and out.top_logprobs.shape == (rows, N_NEW, 3)
    assert torch.isfinite(out.logprobs).all() and (out.logprobs <= 0).all() and (out.logprobs <= out.top_logprobs[..., 0]).all()
    assert (out.top_logprobs[..., :-1] >= out.top_logprobs[..., 1:]).all()
    hit = out.top_token_ids == out.sequences[..., None]                # where the token is among the alternatives it carries their number
    assert torch.equal(out.top_logprobs[hit], out.logprobs[:, :, None].expand(-1, -1, 3)[hit])
    opts = dict(make(), output_logprobs=True)
    bare = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], **opts)
    assert bare.top_token_ids is None and bare.top_logprobs is None and torch.equal(bare.sequences, plain)
    assert torch.equal(bare.logprobs, out.logprobs)


@pytest.mark.parametrize("rows", [[0, 1], [0]], ids=["batch2", "batch1"])
def test_generate_device_loop_agrees_with_the_host_loop(tiny_bf16, monkeypatch, rows):
    """The graph / device loop (batch 1: the path one sequence takes) returns the host loop's tokens and its log-probabilities within two
    kernel bounds plus the bf16 route bar."""
    m, vx, lx, am = tiny_bf16
    vx, lx, am = vx[rows], lx[rows], am[rows]
    host, logits = _host_run(m, vx, lx, am, monkeypatch, k=2)
    opts = dict(output_logprobs=True, top_logprobs=2, use_graph=True, max_new_tokens=N_NEW, eos_token_id=[])
    dev = m.generate(vx, lx, attention_mask=am, **opts)
    assert torch.equal(dev.sequences, host.sequences) and torch.equal(dev.top_token_ids[..., 0], host.top_token_ids[..., 0])
    big = max(1.0, max(float(lg.float().abs().max()) for lg in logits))
    bound = max(float(r[3].max()) for r in _ref_from_logits(logits, host.sequences, 0))
    err = float((dev.logprobs - host.logprobs).abs().max())
    print(f"device loop vs host loop ({len(rows)} rows): max |diff| = {err:.3g}, bit-equal: {torch.equal(dev.logprobs, host.logprobs)}")
    assert err <= 2 * bound + BF16_ROUTE_BAR * big
    assert float((dev.top_logprobs - host.top_logprobs).abs().max()) <= 2 * bound + BF16_ROUTE_BAR * big


@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_positions_behind_an_eos_hold_the_skipped_values(tiny_bf16, use_graph):
    m, vx, lx, am = tiny_bf16
    first = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], use_graph=use_graph)
    eos = int(first[0, 2])                                             # row 0 ends at step 2
    assert eos not in first[0, :2].tolist() and eos not in first[1].tolist()
    opts = dict(output_logprobs=True, top_logprobs=2, use_graph=use_graph, max_new_tokens=N_NEW, eos_token_id=eos)
    out = m.generate(vx, lx, attention_mask=am, **opts)
    plain = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=eos, use_graph=use_graph)
    assert torch.equal(out.sequences, plain) and torch.equal(out.sequences[:, :3], first[:, :3]) and out.sequences.shape[1] == N_NEW
    assert (out.sequences[0, 3:] == gen.TINY["pad_token_id"]).all()
    assert (out.logprobs[0, 3:] == 0).all() and (out.top_token_ids[0, 3:] == -1).all() and (out.top_logprobs[0, 3:] == 0).all()
    assert (out.logprobs[0, :3] < 0).all() and (out.logprobs[1] < 0).all() and (out.top_token_ids[1] >= 0).all()      # the EOS step is scored


def test_generate_from_a_cache_with_logprobs(tiny_bf16):
    m, vx, lx, am = tiny_bf16
    new_ids = torch.randint(3, 31000, (2, 3), generator=torch.Generator().manual_seed(6)).to(DEV)
    outs = []
    for opts in (dict(), dict(output_logprobs=True, top_logprobs=1)):
        with torch.no_grad():
            prep = m._prepare_inputs_for_forward(vision_tokens=m.vision_tokenizer(m._encode_vision_x(vx)), lang_x=lx, attention_mask=am,
                                                 padding_side="right")
            cache = m.lang_model(inputs_embeds=prep["inputs_embeds"], attention_mask=prep["attention_mask"], use_cache=True,
                                 cache_capacity=prep["inputs_embeds"].shape[1] + 16, last_token_logits=True).past_key_values
        outs.append((m.generate(None, new_ids, past_key_values=cache, max_new_tokens=N_NEW, eos_token_id=[], **opts), cache.cache_len.clone()))
    (plain, len0), (out, len1) = outs
    assert torch.equal(out.sequences, plain) and torch.equal(len0, len1)
    assert torch.equal(out.top_token_ids[..., 0], out.sequences) and torch.equal(out.top_logprobs[..., 0], out.logprobs) and (out.logprobs < 0).all()


def test_generate_fp32_host_loop(tiny_f32, monkeypatch):
    m, vx, lx, am = tiny_f32
    out, logits = _host_run(m, vx, lx, am, monkeypatch, k=1)
    assert logits[0].dtype == torch.float32
    plain = m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], use_graph=False)
    assert torch.equal(out.sequences, plain)
    for t, ref in enumerate(_ref_from_logits(logits, out.sequences, 1)):
        _check(f"fp32 host loop step {t}", (out.logprobs[:, t], out.top_token_ids[:, t], out.top_logprobs[:, t]), ref, 1)


def test_plain_generate_never_launches_the_logprob_kernel(tiny_bf16, monkeypatch):
    from aki_amd import ops

    def boom(*a, **kw):
        raise AssertionError("ops.token_logprob was called by a generate that did not ask for log-probabilities")

    m, vx, lx, am = tiny_bf16
    want = {name: m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], **make()) for name, make in _modes().items()}
    monkeypatch.setattr(ops, "token_logprob", boom)
    for name, make in _modes().items():
        assert torch.equal(m.generate(vx, lx, attention_mask=am, max_new_tokens=N_NEW, eos_token_id=[], **make()), want[name]), name
    assert m.generate(vx, lx, attention_mask=am, max_new_tokens=3, eos_token_id=[], num_beams=2).shape == (2, 3)
    opts = dict(output_logprobs=True)
    with pytest.raises(AssertionError, match="token_logprob"):
        m.generate(vx, lx, attention_mask=am, max_new_tokens=2, eos_token_id=[], **opts)


# ---- score ----------------------------------------------------------------------------------------------------------------------------
def _forward_reference(m, vx, lx, am, cont, lengths, k):
    """float64 log-softmax of a full forward over prompt + continuation, one forward per candidate: (lp [B, N, T] (0 behind the lengths),
    bound [B, N, T], max |logits|, top ids [B, N, T, k])."""
    B, N, T = cont.shape
    lp, bound, top = np.zeros((B, N, T)), np.zeros((B, N, T)), np.full((B, N, T, k), -1)
    big = 1.0
    for b in range(B):
        nreal = int(am[b].sum())
        for n in range(N):
            ln = int(lengths[b, n])
            ids = torch.cat([lx[b, :nreal], cont[b, n, :ln]])[None]
            with torch.no_grad():
                logits = m(vx[b:b + 1], ids, attention_mask=torch.ones_like(ids)).logits[0, -(ln + 1):-1]      # the rows that predict the continuation
            ref = LC.reference(logits.float().cpu().numpy(), cont[b, n, :ln].cpu().numpy(), k)
            lp[b, n, :ln], top[b, n, :ln], bound[b, n, :ln] = ref[0], ref[1], ref[3]
            big = max(big, float(logits.float().abs().max()))
    return lp, bound, big, top


def test_score_against_full_forwards_fp32(tiny_f32):
    m, vx, lx, am = tiny_f32
    assert 32001 in lx[0].tolist() and 32001 in lx[1].tolist() and gen.TINY["media_token_id"] in lx[1].tolist()
    cont = torch.randint(3, 31000, (2, 2, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    lengths = torch.tensor([[3, 1], [2, 3]])
    out = m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths, top_logprobs=1)
    lp, bound, big, top = _forward_reference(m, vx, lx, am, cont, lengths, 1)
    got = out.logprobs.double().cpu().numpy()
    live = np.arange(3)[None, None, :] < lengths.numpy()[:, :, None]
    err = np.abs(got - lp)
    print(f"score fp32 vs full forwards: max err {err.max():.3g} (max |logits| {big:.3g})")
    assert (err[live] <= 2 * FP32_LOGIT_BAR * big + bound[live]).all()
    assert (got[~live] == 0).all() and (out.top_token_ids.cpu().numpy()[~live] == -1).all() and (out.top_logprobs.cpu().numpy()[~live] == 0).all()
    assert out.logprobs.shape == (2, 2, 3) and out.top_token_ids.shape == (2, 2, 3, 1) and torch.equal(out.lengths.cpu(), lengths)
    assert torch.equal(out.sum_logprobs, out.logprobs.sum(-1)) and out.sum_logprobs.shape == (2, 2)
    assert np.array_equal(out.top_token_ids.cpu().numpy()[live], top[live])          # rank 0 is the full forward's argmax
    bare = m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths)
    assert bare.top_token_ids is None and torch.equal(bare.logprobs, out.logprobs)


def _route_bar(logits):
    """Two kernel bounds plus the bf16 route bar, for the recorded logits of a run."""
    big = max(1.0, max(float(lg.float().abs().max()) for lg in logits))
    return 2 * LC.logprob_bound(big, logits[0].shape[-1]) + BF16_ROUTE_BAR * big


def test_score_of_generated_tokens_gives_generates_logprobs(tiny_bf16, monkeypatch):
    """N = 1, no eos: teacher-forcing the tokens a greedy generate returned walks the same steps (T = 8: behind the DecodeGraph)."""
    m, vx, lx, am = tiny_bf16
    gen_out, logits = _host_run(m, vx, lx, am, monkeypatch, k=2)
    out = m.score(vx, lx, gen_out.sequences[:, None, :], attention_mask=am, top_logprobs=2)
    err = float((out.logprobs[:, 0] - gen_out.logprobs).abs().max())
    print(f"score vs generate (bf16): max |diff| = {err:.3g}, bit-equal: {torch.equal(out.logprobs[:, 0], gen_out.logprobs)}")
    assert err <= _route_bar(logits)
    assert torch.equal(out.top_token_ids[:, 0, :, 0], gen_out.sequences)
    assert float((out.sum_logprobs[:, 0] - gen_out.logprobs.sum(1)).abs().max()) <= N_NEW * _route_bar(logits)


def test_score_graph_route_equals_stepping(tiny_bf16, monkeypatch):
    """T = 9 takes the DecodeGraph by default (generate's rule: from 8 on); use_graph=False steps eagerly."""
    m, vx, lx, am = tiny_bf16
    cont = torch.randint(3, 31000, (2, 2, 9), generator=torch.Generator().manual_seed(9)).to(DEV)
    lengths = torch.tensor([[9, 4], [1, 8]])
    graph = m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths, top_logprobs=1)
    rec = _Recorder(m, monkeypatch)
    eager = m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths, top_logprobs=1, use_graph=False)
    monkeypatch.undo()
    assert len(rec.logits) == 9
    err = float((graph.logprobs - eager.logprobs).abs().max())
    print(f"score graph vs eager: max |diff| = {err:.3g}, bit-equal: {torch.equal(graph.logprobs, eager.logprobs)}")
    assert err <= _route_bar(rec.logits)
    live = torch.arange(9)[None, None, :] < lengths[:, :, None]
    assert (graph.logprobs.cpu()[~live] == 0).all() and (graph.logprobs.cpu()[live] < 0).all()
    assert (graph.top_token_ids.cpu()[~live] == -1).all() and (graph.top_token_ids.cpu()[live] >= 0).all()


def test_score_over_a_shared_prompt_cache(tiny_bf16, monkeypatch):
    """lang_model.share_prompt_kv = True: the N rows of a sample read one copy of the prompt's K/V (AkiKVCache.share_prefix), as
    num_return_sequences does; the scores stay within the bf16 route bar of the replicated cache's."""
    m, vx, lx, am = tiny_bf16
    cont = torch.randint(3, 31000, (2, 3, 4), generator=torch.Generator().manual_seed(12)).to(DEV)
    lengths = torch.tensor([[4, 2, 3], [1, 4, 4]])
    rec = _Recorder(m, monkeypatch)
    want = m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths, top_logprobs=1)
    monkeypatch.undo()
    monkeypatch.setattr(m.lang_model, "share_prompt_kv", True, raising=False)
    shared = []
    expand = m._expand_rows

    def spy(cache, *a, **kw):
        out = expand(cache, *a, **kw)
        shared.append(cache.group)
        return out

    monkeypatch.setattr(m, "_expand_rows", spy)
    got = m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths, top_logprobs=1)
    assert shared == [3], "the cache was not grouped"
    err = float((got.logprobs - want.logprobs).abs().max())
    print(f"score over a shared prompt cache vs replicated: max |diff| = {err:.3g}")
    assert err <= _route_bar(rec.logits)
    live = torch.arange(4)[None, None, :] < lengths[:, :, None]
    assert (got.logprobs.cpu()[~live] == 0).all() and (got.logprobs.cpu()[live] < 0).all()


@pytest.fixture(scope="module")
def both_classes(tmp_path_factory):
    """(HF-Hub twin, train-time class) over the same weights, bf16 on the GPU: test_hub_twin.py's fixture."""
    from aki_amd import aki, modeling_aki
    from test_hub_twin import _tiny_checkpoints
    T = gen.TINY
    _, _, pv, pl = _tiny_checkpoints(str(tmp_path_factory.mktemp("ckpt")))
    twin = modeling_aki.AKI(pv, pl, pad_token_id=T["pad_token_id"], initial_tokenizer_len=T["vocab"], num_vision_tokens=T["num_vision_tokens"])
    vt = modeling_aki.native_vision_tower(pv)
    train = aki.AKI(vt, modeling_aki.native_language_model(pl), vis_feature_dim=vt.config.hidden_size, initial_tokenizer_len=T["vocab"],
                    pad_token_id=T["pad_token_id"], decoder_layers_attr_name="model.layers", num_vision_tokens=T["num_vision_tokens"])
    train.load_state_dict(twin.state_dict(), strict=True)
    for m in (twin, train):
        m.set_special_token_ids({"<image>": T["media_token_id"], "<|endofchunk|>": T["eoc_token_id"]})
        m.to(device="cuda", dtype=torch.bfloat16).eval()
    return twin, train


def test_hub_twin_scores_like_the_train_time_class(both_classes):
    from test_hub_twin import _two_prompts
    twin, train = both_classes
    vx, lx, am = _two_prompts()
    cont = torch.randint(3, 31000, (2, 2, 4), generator=torch.Generator().manual_seed(10)).to(DEV)
    lengths = torch.tensor([[4, 2], [3, 4]])
    a, b = (m.score(vx, lx, cont, attention_mask=am, continuation_lengths=lengths, top_logprobs=2) for m in (twin, train))
    assert torch.equal(a.logprobs, b.logprobs) and torch.equal(a.top_token_ids, b.top_token_ids) and torch.equal(a.top_logprobs, b.top_logprobs)
    assert torch.equal(a.sum_logprobs, b.sum_logprobs) and (a.logprobs[0, 0] < 0).all()
