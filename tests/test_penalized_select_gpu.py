"""uvx_seen_mark and uvx_greedy_select_penalized (include/uvx.h; csrc/select.hip) on the device against the numpy reference of
tests/penalized_util.py - bitmap, penalised scores and token EXACTLY (no tolerance), the bookkeeping, launch-to-launch visibility - and through
generate().  f32 and bf16 logits throughout (this file stands in for tests/test_f32_kernels_gpu.py's list of dtype entry points, which the new
entry point's `logits_dtype` spelling keeps it out of)."""
import numpy as np
import pytest
import torch

import penalized_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
PENALTIES = (1.1, 1.3, 50.0, 0.5)


def bits(seen):
    """The device bitmap (int32 tensor) as numpy uint32."""
    return seen.cpu().numpy().view(np.uint32)


def check_select(dev, ids_rows, penalty, what, words_extra=0, **kw):
    """One select on dev [B, V] with the bitmap of ids_rows: scores bitwise, token, and the bitmap afterwards = before | the tokens written."""
    from ultravox_amd import ops
    B, V = dev.shape
    rows = dev.float().cpu().numpy()
    before = PU.bitmap(ids_rows, V, PU.words_of(V) + words_extra)
    seen = torch.from_numpy(before.view(np.int32).copy()).to(DEV)
    out = ops.greedy_select_penalized(dev, seen, penalty, want_scores=True, **kw)
    scores, toks = out["scores"].cpu().numpy(), out["tokens"].cpu().tolist()
    for b in range(B):
        want = PU.penalized(rows[b], ids_rows[b], penalty)
        assert PU.same_bits(scores[b], want), (what, b, np.flatnonzero(scores[b].view(np.uint32) != want.view(np.uint32))[:8])
        if "unfinished" not in kw:
            assert toks[b] == PU.argmax(want), (what, b, toks[b], PU.argmax(want))
    after = before | PU.bitmap([[t] for t in toks], V, before.shape[1])
    assert np.array_equal(bits(seen), after), what
    return out, toks


@pytest.mark.parametrize("V", [1, 31, 32, 33, 4099, 131077])
def test_seen_mark(V):
    """The bitmap equals the numpy one exactly: duplicates, 0, V - 1, ids outside [0, V) (never dereferenced), n = 0, a strided view, a second call
    OR-ing into the first, and the words past ceil(V / 32) untouched."""
    from ultravox_amd import ops
    B, n, extra = 3, 48, 3
    g = np.random.default_rng(V)
    ids = g.integers(0, V, size=(B, n))
    ids[:, 10:20] = ids[:, :10]                          # duplicates
    ids[:, 0], ids[:, 1] = 0, V - 1
    ids[0, 2], ids[1, 3], ids[2, 4], ids[0, 5], ids[1, 6] = -1, V, 2 ** 40, -2 ** 40, V + 31
    words = PU.words_of(V) + extra
    guard = np.int32(0x5A5A5A5A)
    seen = torch.zeros(B, words, device=DEV, dtype=torch.int32)
    seen[:, PU.words_of(V):] = int(guard)
    want = PU.bitmap(ids, V, words)
    want[:, PU.words_of(V):] = np.uint32(guard)
    dev_ids = torch.from_numpy(ids).to(DEV)
    assert ops.seen_mark(dev_ids, V, seen) is seen
    assert np.array_equal(bits(seen), want)
    ops.seen_mark(dev_ids[:, :0], V, seen)               # n = 0: a no-op
    assert np.array_equal(bits(seen), want)
    # a strided view (row stride 64, offset 7) of other ids: ORs into what is there
    big = torch.from_numpy(g.integers(-3, V + 3, size=(B, 64))).to(DEV)
    view = big[:, 7:29]
    assert view.stride(0) == 64 and not view.is_contiguous()
    ops.seen_mark(view, V, seen)
    want2 = want | PU.bitmap(view.cpu().numpy(), V, words)
    assert np.array_equal(bits(seen), want2) and (bits(seen)[:, PU.words_of(V):] == np.uint32(guard)).all()
    fresh = ops.seen_mark(dev_ids, V)                    # created when not given: zeroed, ceil(V / 32) words
    assert tuple(fresh.shape) == (B, PU.words_of(V)) and np.array_equal(bits(fresh), PU.bitmap(ids, V))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1, 5, 1023, 1024, 1025, 4099, 8200, 32768, 49160, 131077])
def test_scores_and_token_exactly(V, dtype):
    """scores_out equals the reference in every bit and the token is the reference's argmax, B = 1 and 3, penalties 1.1, 1.3, 50 and 0.5: the vector
    path with one trip (1024), two (8200), four (32768) and six or seven (49160), the scalar tail / path (V % 8 != 0), odd V whose rows after the
    first are unaligned.  The seen sets hold index 0, index V - 1 and the elements of the last (partial) vector."""
    g = np.random.default_rng(V)
    dev = (4.0 * torch.from_numpy(g.standard_normal((3, V)).astype(np.float32))).to(DEV).to(dtype)
    ids_rows = []
    for b in range(3):
        tail = np.arange(max(0, V - 1 - (V - 1) % 8 - (8 if b == 2 else 0)), V)       # the last (partial) vector; row 2: the one before it too
        ids_rows.append(np.concatenate([[0, V - 1], tail[b % 2::2] if b else tail, g.integers(0, V, size=max(1, V // 10))]))
    for B in (1, 3):
        for p in PENALTIES:
            check_select(dev[:B], ids_rows[:B], p, (V, B, p), words_extra=B - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [4096, 4099])
def test_crafted_rows(V, dtype):
    """Rows built so that the penalty decides (all values exact in bf16); every one is also held to the reference bitwise by check_select."""
    from ultravox_amd import ops
    inf, nan = float("inf"), float("nan")
    g = np.random.default_rng(7)
    base = lambda: torch.from_numpy((g.integers(-64, 64, size=V) / 64.0).astype(np.float32))        # |x| < 1, exact in bf16
    rows, ids, pens, want = [], [], [], []

    def case(row, seen_ids, p, token):
        rows.append(row); ids.append(seen_ids); pens.append(p); want.append(token)
    r = base(); r[100], r[200] = 8.0, 6.0
    case(r, [100, 7], 2.0, 200)                          # the raw argmax is seen and positive: 8 / 2 < 6, dethroned
    r = -5.0 - base().abs(); r[100], r[200] = -1.0, -1.5
    case(r, [100, 7], 2.0, 200)                          # all negative, the top is seen: -1 * 2 < -1.5
    r = base(); r[300], r[700] = 8.0, 4.0
    case(r, [300], 2.0, 300)                             # equal after the penalty (8 / 2 == 4): the lowest index wins - the seen one here
    r = base(); r[700], r[300] = 8.0, 4.0
    case(r, [700], 2.0, 300)                             # ... and the unseen one here
    r = base(); r[V - 1], r[0] = 8.0, 4.0
    case(r, [V - 1], 2.0, 0)                             # ... across the whole row (last element against the first)
    r = base(); r[100], r[200] = 3.0, 5.0
    case(r, [100], 0.5, 100)                             # a penalty below 1 promotes seen tokens: 3 / 0.5 > 5
    r = base(); r[10], r[11], r[12], r[13], r[14] = inf, -inf, nan, -0.0, nan
    case(r, [10, 11, 12, 13], 1.3, 10)                   # +inf / p = +inf wins; NaN (seen or not) never does
    r = base(); r[11], r[12], r[13], r[14], r[500] = -inf, nan, -0.0, nan, 2.0
    case(r, [11, 12, 13, 500, V - 1], 1.3, 500)
    r = torch.full((V,), -inf)
    case(r, [0, 5], 1.3, 0)                              # nothing above -inf: index 0
    r = torch.full((V,), -inf); r[3], r[9] = nan, nan
    case(r, [3], 50.0, 0)
    r = base().abs() + 1.0; r[V - 1] = 9.0
    case(r, list(range(0, V - 1)), 50.0, V - 1)          # everything but the last element is seen
    for i, (r, seen_ids, p, token) in enumerate(zip(rows, ids, pens, want)):
        # as row 0 (aligned) and as row 1 (for odd V: unaligned, the scalar path)
        dev = torch.stack([r, r]).to(DEV).to(dtype)
        _, toks = check_select(dev, [seen_ids, seen_ids], p, ("crafted", i))
        assert toks == [token, token], (i, toks, token)
    # penalty == 1: token and bookkeeping are uvx_greedy_select's
    B, stride, col, step, pad = 4, 9, 4, 2, 3
    x = (4.0 * torch.from_numpy(g.standard_normal((B, V)).astype(np.float32))).to(DEV).to(dtype)
    x[0, 11] = 50.0
    eos = torch.tensor([11, 12], device=DEV)
    pos0 = torch.tensor([5, 6, 7, 8], device=DEV, dtype=torch.int32)
    mk = lambda: dict(unfinished=torch.tensor([1, 1, 0, 1], device=DEV, dtype=torch.int32), sequences=torch.full((B, stride), -1, device=DEV, dtype=torch.int64),
                      counter=torch.tensor([0, 9], device=DEV, dtype=torch.int32))
    a, b = mk(), mk()
    seen = ops.seen_mark(torch.from_numpy(g.integers(0, V, size=(B, 300))).to(DEV), V)
    out = ops.greedy_select_penalized(x, seen, 1.0, eos_ids=eos, pad=pad, col=col, positions0=pos0, step=step, **a)
    plain = ops.greedy_select(x, eos_ids=eos, pad=pad, col=col, positions0=pos0, step=step, **b)
    nxt, pos = plain["tokens"], plain["positions"]
    assert torch.equal(out["tokens"], nxt) and torch.equal(out["positions"], pos)
    for k in ("unfinished", "sequences", "counter"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_bookkeeping(dtype):
    """The scenario of test_sample_gpu.test_bookkeeping: a forced EOS clears `unfinished`, a row finished earlier gets pad, sequences with a stride,
    positions, both counter slots over consecutive steps.  And the bitmap: the bit of every token WRITTEN is set, the pad's too; pad = -1 sets
    nothing and leaves the words around the row as they are."""
    from ultravox_amd import ops
    torch.manual_seed(5)
    B, V, stride, pad = 4, 131072 + 5, 20, 7
    W = PU.words_of(V)
    x = torch.randn(B, V, device=DEV).to(dtype)
    x[0, 11] = 50.0                                          # row 0 emits EOS 11 -> finished (11 is not seen: 50 stays the top)
    eos = torch.tensor([11, 12], device=DEV)
    unfinished = torch.tensor([1, 1, 0, 1], device=DEV, dtype=torch.int32)   # row 2 finished earlier -> pad
    seq = torch.full((B, stride), -1, device=DEV, dtype=torch.int64)
    pos0 = torch.tensor([5, 6, 7, 8], device=DEV, dtype=torch.int32)
    counter = torch.tensor([9, 0], device=DEV, dtype=torch.int32)     # slot 0: the previous step's count
    step, col, p = 3, 13, 1.3
    g = np.random.default_rng(5)
    ids = [np.concatenate([g.integers(13, V, size=400), np.argsort(-x[b].float().cpu().numpy())[:3] if b else []]).astype(np.int64) for b in range(B)]
    rows = x.float().cpu().numpy()
    ref = [PU.argmax(PU.penalized(rows[b], ids[b], p)) for b in range(B)]
    assert all(ref[b] != int(rows[b].argmax()) for b in (1, 2, 3))       # (the penalty decides in these rows)
    out, nxt = check_select(x, ids, p, "bookkeeping", eos_ids=eos, pad=pad, unfinished=unfinished, sequences=seq, col=col, positions0=pos0, step=step,
                            counter=counter)
    assert nxt == [11, ref[1], pad, ref[3]]
    assert seq[:, col].cpu().tolist() == nxt and (seq[:, :col] == -1).all() and (seq[:, col + 1:] == -1).all()
    still = [0, int(nxt[1] not in (11, 12)), 0, int(nxt[3] not in (11, 12))]
    assert unfinished.cpu().tolist() == still
    assert out["positions"].cpu().tolist() == [5 + step, 6 + step, 7 + step, 8 + step]
    assert counter.cpu().tolist() == [0, sum(still)]           # counter[step & 1] = rows still running; the other slot cleared
    seen = out["seen"]
    assert all(PU.ids_of(bits(seen)[b]).tolist().count(nxt[b]) == 1 for b in range(B))          # the token written, the pad (7) of row 2 included
    # the next step: the other counter slot, the next column; rows 0 and 2 write pad, rows 1 and 3 see their own last token
    before = bits(seen).copy()
    out2 = ops.greedy_select_penalized(x, seen, p, eos_ids=eos, pad=pad, unfinished=unfinished, sequences=seq, col=col + 1, positions0=pos0, step=step + 1,
                                       counter=counter)
    nxt2 = out2["tokens"].cpu().tolist()
    ref2 = [PU.argmax(PU.penalized(rows[b], PU.ids_of(before[b]), p)) for b in range(B)]
    assert nxt2 == [pad if not still[b] else ref2[b] for b in range(B)]
    still2 = [int(still[b] and nxt2[b] not in (11, 12)) for b in range(B)]
    assert unfinished.cpu().tolist() == still2 and counter.cpu().tolist() == [sum(still2), 0]
    assert seq[:, col + 1].cpu().tolist() == nxt2 and seq[:, col].cpu().tolist() == nxt and out2["positions"].cpu().tolist() == [9, 10, 11, 12]
    assert np.array_equal(bits(seen), before | PU.bitmap([[t] for t in nxt2], V, W))
    # pad = -1 (eos_token_id = -1 callers): every row finished -> -1 written, no bit set anywhere - the words before, between and after the rows included
    big = torch.from_numpy(g.integers(-2 ** 31, 2 ** 31, size=(B + 2, W + 2), dtype=np.int64).astype(np.int32)).to(DEV)
    keep = big.clone()
    view = big[1:1 + B]                                      # rows of W + 2 words: the kernel's `words`
    done = torch.zeros(B, device=DEV, dtype=torch.int32)
    o = ops.greedy_select_penalized(x, view, p, pad=-1, unfinished=done, sequences=seq, col=0)
    assert o["tokens"].cpu().tolist() == [-1] * B and seq[:, 0].cpu().tolist() == [-1] * B
    assert torch.equal(big, keep)
    with pytest.raises(ValueError):
        ops.greedy_select_penalized(x, seen, 0.0)
    with pytest.raises(ValueError):
        ops.greedy_select_penalized(x, seen[:, :W - 1], 1.3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_consecutive_launches_see_each_others_tokens(dtype):
    """Six consecutive selects on fixed logits with penalty 50 and an empty bitmap give the reference loop's six tokens, and the bitmap afterwards
    holds exactly those."""
    from ultravox_amd import ops
    B, V, N = 2, 4099, 6
    g = np.random.default_rng(9)
    dev = (4.0 * torch.from_numpy(g.standard_normal((B, V)).astype(np.float32))).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    seen = torch.zeros(B, PU.words_of(V), device=DEV, dtype=torch.int32)
    seq = torch.full((B, N), -1, device=DEV, dtype=torch.int64)
    live = torch.ones(B, device=DEV, dtype=torch.int32)
    counter = torch.zeros(2, device=DEV, dtype=torch.int32)
    for step in range(N):
        ops.greedy_select_penalized(dev, seen, 50.0, unfinished=live, sequences=seq, col=step, step=step, counter=counter)
    want = [PU.greedy_loop(rows[b], 50.0, N) for b in range(B)]
    assert seq.cpu().tolist() == want and all(len(set(w)) == N for w in want)
    assert np.array_equal(bits(seen), PU.bitmap(want, V))


def _small(dtype, seed):
    from test_model_gpu import SMALL
    from ultravox_amd.config import UltravoxConfig
    from ultravox_amd.model import UltravoxModel
    return UltravoxModel(UltravoxConfig(**SMALL), device=DEV, dtype=dtype, seed=seed)


def _padded(seed, B=2, T=12):
    ids = torch.randint(3, 500, (B, T), generator=torch.Generator().manual_seed(seed))
    am = torch.ones(B, T, dtype=torch.long)
    am[1, :3] = 0
    ids[1, :3] = 2
    return ids.to(DEV), am.to(DEV)


def host_loop(model, **kw):
    model.penalized_select = False
    try:
        return model.generate(**kw)
    finally:
        model.penalized_select = True


# Prompt length of the generate() tests: 160 random ids cover about a quarter of the SMALL model's 512-entry vocabulary, so that the plain
# continuation runs into seen ids within a few steps and the penalty decides tokens (with a dozen prompt tokens it never does).
T_PROMPT = 160
# (model seed, input seed) of test_f32_generate_equals_the_replay_of_hf_rule.  The host loop's penalty runs in torch on the GPU, which may divide by
# multiplying with a reciprocal - one ulp away from HF's rule - so "the host loop's tokens equal the replay" is a precondition on the INPUTS, not a
# property of the new code: the seeds are ones for which it held at every step on an MI355X (the test asserts it again; no step is skipped).
F32_SEEDS = (3, 16)


@pytest.mark.parametrize("p", [1.3, 50.0])
def test_f32_generate_equals_the_replay_of_hf_rule(p):
    """B = 2 with left padding, 8 new tokens: the device path's tokens equal, at every step, HF's rule replayed with the numpy reference on the raw
    logits of every step (which the host loop reports under output_logits); so do the host loop's own (the precondition above)."""
    model = _small(torch.float32, F32_SEEDS[0])
    assert model.penalized_select is True
    ids, am = _padded(F32_SEEDS[1], T=T_PROMPT)
    T, N = ids.shape[1], 8
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1)
    dev = model.generate(repetition_penalty=p, **kw)
    host = host_loop(model, repetition_penalty=p, output_logits=True, return_dict_in_generate=True, **kw)
    assert dev.shape == host.sequences.shape == (2, T + N) and len(host.logits) == N
    hs = host.sequences.cpu().numpy()
    replay = np.zeros((2, N), dtype=np.int64)
    for step in range(N):
        raw = host.logits[step].float().cpu().numpy()
        for b in range(2):
            replay[b, step] = PU.argmax(PU.penalized(raw[b], hs[b, :T + step], p))
    assert np.array_equal(hs[:, T:], replay), ("precondition: the host loop follows HF's rule on these inputs", hs[:, T:], replay)
    assert np.array_equal(dev.cpu().numpy()[:, T:], replay), (dev[:, T:], replay)
    assert torch.equal(dev[:, :T], ids)
    if p == 50.0:
        assert not torch.equal(dev, model.generate(**kw))                 # the penalty decides somewhere


def test_f32_generate_matches_the_oracle_loop_over_hf_processor():
    """As test_generate_gpu's oracle test, with the repetition penalty alone (the device path): audio, left padding, token for token against the
    oracle's cache-free loop applying HF's own RepetitionPenaltyLogitsProcessor."""
    from transformers.generation import logits_process as LP
    from oracle.reference_cpu import logmel_ref, synthetic_batch
    from test_generate_gpu import _build
    cfg, model, oracle = _build(torch.float32, 23)
    assert model.penalized_select is True
    b = synthetic_batch(cfg, 2, 2.0, n_text=20, audio_start=4, n_supervised=4)
    b.pop("labels")
    b["audio_values"] = logmel_ref(b.pop("pcm"), 80)
    b["attention_mask"][1, :3] = 0
    b["input_ids"][1, :3] = 2
    gb = {k: v.to(DEV) for k, v in b.items()}
    T, N, eos = b["input_ids"].shape[1], 8, 2
    want = oracle.generate_greedy(N, eos_token_id=eos, logits_processor=LP.LogitsProcessorList([LP.RepetitionPenaltyLogitsProcessor(1.3)]), **b)
    got = model.generate(max_new_tokens=N, eos_token_id=eos, repetition_penalty=1.3, **gb).cpu()
    n = min(got.shape[1], want.shape[1])
    assert n >= T + 1 and torch.equal(got[:, :n], want[:, :n]), (got[:, T:], want[:, T:])


class Rec:
    def __init__(self):
        self.puts, self.ended = [], False

    def put(self, v):
        self.puts.append(v.clone())

    def end(self):
        self.ended = True


def same_state(a, b, layers, B):
    assert (a.Tmax, a.cur_len, a.partial_ok) == (b.Tmax, b.cur_len, b.partial_ok)
    for f in ("pos_next", "kv_start", "tokens"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    planes = layers * 2 * B
    row = a.cache.numel() // (planes * a.Tmax)
    rows = lambda s: s.cache[:planes * s.Tmax * row].view(planes, s.Tmax, row)[:, :s.cur_len]
    assert a.cache.numel() == b.cache.numel() and torch.equal(rows(a), rows(b))


def test_bf16_generate_device_path_equals_the_host_loop():
    """Free run, an early stop with pad_token_id (the KV state field by field, the streamer's puts), and a second turn over past_key_values - with
    reused rows (the bitmap must cover ids the chunk prefill never sees) and with a mismatching prefix."""
    model = _small(torch.bfloat16, 3)
    ids, am = _padded(16, T=T_PROMPT)
    T, N, p = ids.shape[1], 8, 1.3
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=N, repetition_penalty=p)
    dev = model.generate(eos_token_id=-1, return_dict_in_generate=True, **kw)
    host = host_loop(model, eos_token_id=-1, return_dict_in_generate=True, **kw)
    assert torch.equal(dev.sequences, host.sequences) and dev.sequences.shape == (2, T + N)
    same_state(dev.past_key_values, host.past_key_values, model._c.llm_layers, 2)
    # early stop: the token row 0 produced at step 3 becomes the terminator
    stop = int(dev.sequences[0, T + 3])
    first = dev.sequences[0, T:].tolist().index(stop)
    ra, rb = Rec(), Rec()
    e_dev = model.generate(eos_token_id=stop, pad_token_id=1, return_dict_in_generate=True, streamer=ra, **kw)
    e_host = host_loop(model, eos_token_id=stop, pad_token_id=1, return_dict_in_generate=True, streamer=rb, **kw)
    assert torch.equal(e_dev.sequences, e_host.sequences)
    row0 = e_dev.sequences[0, T:].tolist()
    assert row0[:first + 1] == dev.sequences[0, T:T + first + 1].tolist() and all(v == 1 for v in row0[first + 1:])
    same_state(e_dev.past_key_values, e_host.past_key_values, model._c.llm_layers, 2)
    assert ra.ended and rb.ended and len(ra.puts) == len(rb.puts) == e_dev.sequences.shape[1] - T + 1
    assert all(torch.equal(x, y) for x, y in zip(ra.puts, rb.puts))
    # second turn: the first turn's sequences plus new text
    more = torch.randint(3, 500, (2, 5), generator=torch.Generator().manual_seed(4)).to(DEV)
    ids2 = torch.cat([dev.sequences, more], 1)
    am2 = torch.cat([am, torch.ones(2, ids2.shape[1] - T, dtype=torch.long, device=DEV)], 1)
    kw2 = dict(attention_mask=am2, max_new_tokens=6, eos_token_id=-1, repetition_penalty=p)
    t_dev = model.generate(input_ids=ids2, past_key_values=dev.past_key_values, **kw2)
    assert model.last_prefill_reused == dev.past_key_values.cur_len > 0
    t_host = host_loop(model, input_ids=ids2, past_key_values=dev.past_key_values, **kw2)
    assert model.last_prefill_reused > 0 and torch.equal(t_dev, t_host)
    bad = ids2.clone()
    bad[0, 5] = (bad[0, 5] + 1) % 500
    m_dev = model.generate(input_ids=bad, past_key_values=dev.past_key_values, **kw2)
    assert model.last_prefill_reused == 0
    m_host = host_loop(model, input_ids=bad, past_key_values=dev.past_key_values, **kw2)
    assert torch.equal(m_dev, m_host) and torch.equal(m_dev, model.generate(input_ids=bad, **kw2))


def test_a_philox_generator_with_a_repetition_penalty_still_raises():
    from ultravox_amd.generation import PhiloxGenerator
    model = _small(torch.bfloat16, 3)
    ids, am = _padded(16)
    gen = PhiloxGenerator(1)
    with pytest.raises(ValueError, match="PhiloxGenerator.*score processors"):
        model.generate(input_ids=ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, generator=gen, repetition_penalty=1.2)
    assert gen.offset == 0
