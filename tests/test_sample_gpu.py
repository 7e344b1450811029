"""uvx_sample_select (include/uvx.h; csrc/select.hip) on the device against the float64 reference of tests/sample_util.py - kept set, probabilities,
the draw, the Philox stream, the bookkeeping - and through generate() / LocalInference.  f32 and bf16 logits throughout (this file stands in for
tests/test_f32_kernels_gpu.py's list of dtype entry points, which the new entry point's `logits_dtype` spelling keeps it out of)."""
import itertools

import numpy as np
import pytest
import torch

import sample_util as SU

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = [1, 5, 1023, 1024, 1025, 4099, 131077]
# seeds of sample_util.peaked_rows for which every boundary of the reference clears twice the bound over the whole grid (found on the CPU:
# tests/test_sample_cpu.py does not need them, the tests below assert the margins again)
SEEDS = {(V, 3, dt): 5 if V == 131077 else 0 for V in VS for dt in (torch.float32, torch.bfloat16)}       # key: (V, rows, dtype)
SEEDS.update({(4099, 24, torch.float32): 2, (4099, 24, torch.bfloat16): 0, ("special", 4, torch.float32): 0, ("special", 4, torch.bfloat16): 0})


def grid(V):
    return itertools.product((1.0, 0.7), (0, 1, 5, V, V + 3), (1.0, 0.9, 1e-6), (0.0, 0.1), (1, 3))


def rows_for(V, dtype, B=3):
    """-> (f32 numpy rows as the kernel reads them, the device tensor in `dtype`)."""
    rows = torch.from_numpy(SU.peaked_rows(V, B, SEEDS[(V, B, dtype)]))
    dev = rows.to(DEV).to(dtype)
    return dev.float().cpu().numpy(), dev


def check_probs(p, ref, what):
    kept, want = ref["kept"], ref["probs"]
    assert np.array_equal(p > 0, kept), (what, np.flatnonzero((p > 0) != kept)[:8])
    err = np.abs(p.astype(np.float64) - want)
    tol = SU.bound(int(kept.sum())) * want + 2.0 ** -126
    assert (err <= tol).all(), (what, int(np.argmax(err - tol)), float((err / np.maximum(tol, 1e-300)).max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", VS)
def test_kept_set_and_probabilities_over_the_grid(V, dtype):
    """probs_out > 0 is EXACTLY the reference's kept set and every probability is within (n_kept + 96) * 2^-24 of the reference's, relatively, for
    every setting of the grid, B = 1 and 3; the token drawn for a random uniform is acceptable (sample_util.token_ok)."""
    from ultravox_amd import ops
    rows, dev = rows_for(V, dtype)
    refs = {(b, t): SU.RowRef(SU.x_of(rows[b], t)) for b in range(3) for t in (1.0, 0.7)}
    us = np.random.default_rng(V).random(3).astype(np.float32)
    u_dev = torch.from_numpy(us).to(DEV)
    warped = {}
    for B in (1, 3):
        for t, k, p, mp, keep in grid(V):
            out = ops.sample_select(dev[:B], temperature=t, top_k=k, top_p=p, min_p=mp, min_keep=keep, uniforms=u_dev, want_probs=True)
            probs, toks = out["probs"].cpu().numpy(), out["tokens"].cpu().tolist()
            for b in range(B):
                key = (b, t, k, p, mp, keep)
                if key not in warped:
                    warped[key] = refs[(b, t)].warp(k, p, mp, keep)
                    assert SU.margins_ok(warped[key]), ("precondition: the reference's boundary margins", key, warped[key]["margins"])
                check_probs(probs[b], warped[key], (B,) + key)
                assert SU.token_ok(toks[b], float(us[b]), warped[key]), ((B,) + key, toks[b], float(us[b]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_special_rows(dtype):
    """A tied maximum under top_k = 1 (both stay), -inf entries (never kept, never drawn), a row of nothing but -inf (index 0, no probability), the
    maximum in the last column."""
    from ultravox_amd import ops
    V = 4099
    g = np.random.default_rng(3)
    rows = SU.peaked_rows(V, 4, SEEDS[("special", 4, dtype)])
    top = rows[0].argmax()
    rows[0, (top + 1000) % V] = rows[0, top]                          # a second maximum
    rows[1, g.random(V) < 0.4] = -np.inf
    rows[2] = -np.inf
    rows[3, V - 1] = rows[3].max() + 1.5
    dev = torch.from_numpy(rows).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    us = np.array([0.3, 0.6, 0.9, 1 - 2.0 ** -24], dtype=np.float32)
    for t, k, p, mp, keep in ((1.0, 1, 1.0, 0.0, 1), (0.7, 1, 0.9, 0.1, 1), (1.0, 0, 1.0, 0.0, 1), (0.7, 0, 0.9, 0.0, 1), (1.0, 5, 1.0, 0.1, 1), (1.0, 0, 1e-6, 0.0, 1)):
        out = ops.sample_select(dev, temperature=t, top_k=k, top_p=p, min_p=mp, min_keep=keep, uniforms=torch.from_numpy(us).to(DEV), want_probs=True)
        probs, toks = out["probs"].cpu().numpy(), out["tokens"].cpu().tolist()
        for b in range(4):
            ref = SU.RowRef(SU.x_of(rows[b], t)).warp(k, p, mp, keep)
            assert SU.margins_ok(ref), (b, t, k, p, mp, keep, ref["margins"])
            check_probs(probs[b], ref, (b, t, k, p, mp, keep))
            assert SU.token_ok(toks[b], float(us[b]), ref), (b, t, k, p, mp, keep, toks[b])
        assert toks[2] == 0 and not probs[2].any()
        if k == 1:
            assert sorted(np.flatnonzero(probs[0]).tolist()) == sorted([int(top), int((top + 1000) % V)]) and abs(probs[0].max() - 0.5) < 1e-6
        assert np.isfinite(rows[1][toks[1]])
    assert ops.sample_select(dev, top_k=1, uniforms=torch.zeros(4, device=DEV))["tokens"][3].item() == V - 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [1025, 131077])
def test_the_draw_for_given_uniforms(V, dtype):
    """uniforms = 0, 2^-24, 0.5, 1 - 2^-24 and random ones, one per row of a batch of equal rows: every token is kept and its cumulative interval holds
    u * total.  With everything kept the last kept index is V - 1; under top_k = 5 with the head in low columns it is far below: u = 1 - 2^-24
    must give exactly that index in both cases (the top token is put there), never V and never a dropped token."""
    from ultravox_amd import ops
    g = np.random.default_rng(V + 1)
    us = np.concatenate([[0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24], g.random(12)]).astype(np.float32)
    B = len(us)
    row = (g.standard_normal(V) * 0.5).astype(np.float32)
    head = [3, 17, 100, 500, 777]
    row[head] = [12.0, 13.1, 11.2, 10.4, 14.0]                      # the top token is the LAST kept one under top_k = 5 (column 777)
    dev = torch.from_numpy(np.tile(row, (B, 1))).to(DEV).to(dtype)
    x = dev[0].float().cpu().numpy()
    u_dev = torch.from_numpy(us).to(DEV)
    for t, k in ((1.0, 0), (0.7, 0), (1.0, 5), (0.7, 5)):
        ref = SU.RowRef(SU.x_of(x, t)).warp(top_k=k)
        toks = ops.sample_select(dev, temperature=t, top_k=k, uniforms=u_dev)["tokens"].cpu().tolist()
        for b in range(B):
            assert SU.token_ok(toks[b], float(us[b]), ref), (t, k, b, float(us[b]), toks[b])
        last = int(np.flatnonzero(ref["kept"])[-1])
        assert last == (777 if k else V - 1)
        if k:
            assert toks[3] == 777                                     # u * total lies inside the top token's interval, which ends the kept set
    # the end of the row: a last kept token less likely than 2^-24, at V / 2 and at V - 1
    row2 = np.full(V, -np.inf, dtype=np.float32)
    row2[[5, V // 2]] = [10.0, -7.0]                                  # p(last) = e^-17 = 4e-8 < 2^-24: either kept token is acceptable, nothing else is
    row3 = row2.copy()
    row3[V - 1] = -7.0
    dev2 = torch.from_numpy(np.stack([row2, row3])).to(DEV).to(dtype)
    u2 = torch.full((2,), 1 - 2.0 ** -24, device=DEV)
    toks = ops.sample_select(dev2, uniforms=u2)["tokens"].cpu().tolist()
    for b, r in enumerate((row2, row3)):
        ref = SU.RowRef(dev2[b].float().cpu().numpy()).warp()
        assert SU.token_ok(toks[b], 1 - 2.0 ** -24, ref) and ref["kept"][toks[b]], (b, toks[b])
    one = torch.ones(2, device=DEV)                                   # a uniform of 1 (outside Philox's range): the last kept index, never V
    assert ops.sample_select(dev2, uniforms=one)["tokens"].cpu().tolist() == [V // 2, V - 1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_philox_stream(dtype):
    """uniforms = NULL: the tokens are acceptable for u from the numpy Philox with key (seed_lo, seed_hi) and counter (offset_lo, offset_hi, b, 0);
    seeds and offsets beyond 32 bits; two equal launches give equal tokens, another offset gives other tokens somewhere."""
    from ultravox_amd import ops
    V, B = 4099, 24
    rows, dev = rows_for(V, dtype, B)
    refs = [SU.RowRef(SU.x_of(rows[b], 0.7)).warp(top_p=0.9) for b in range(B)]
    flat = [SU.RowRef(SU.x_of(rows[b], 1.0)).warp() for b in range(B)]
    seen = []
    for seed, offset in ((1, 0), ((7 << 32) | 5, 3), (12345, (1 << 32) + 9), (2 ** 64 - 1, 2 ** 64 - 1)):
        us = SU.philox_uniform(seed, offset, B)
        a = ops.sample_select(dev, temperature=0.7, top_p=0.9, seed=seed, offset=offset)["tokens"].cpu().tolist()
        again = ops.sample_select(dev, temperature=0.7, top_p=0.9, seed=seed, offset=offset)["tokens"].cpu().tolist()
        assert a == again
        f = ops.sample_select(dev, seed=seed, offset=offset)["tokens"].cpu().tolist()
        for b in range(B):
            assert SU.margins_ok(refs[b]), (b, refs[b]["margins"])
            assert SU.token_ok(a[b], float(us[b]), refs[b]), (seed, offset, b, a[b], float(us[b]))
            assert SU.token_ok(f[b], float(us[b]), flat[b]), (seed, offset, b, f[b], float(us[b]))
        seen.append(tuple(f))
    assert len(set(seen)) == len(seen)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bookkeeping(dtype):
    """The scenario of test_f32_greedy_select_bookkeeping: a forced EOS (one logit at +50 under top_k = 1) clears `unfinished`, a row finished earlier
    gets pad, sequences / positions / both counter slots."""
    from ultravox_amd import ops
    torch.manual_seed(5)
    B, V, stride, pad = 4, 131072 + 5, 20, 7
    x = torch.randn(B, V, device=DEV).to(dtype)
    x[0, 11] = 50.0                                          # row 0 emits EOS 11 -> finished
    eos = torch.tensor([11, 12], device=DEV)
    unfinished = torch.tensor([1, 1, 0, 1], device=DEV, dtype=torch.int32)   # row 2 finished earlier -> pad
    seq = torch.full((B, stride), -1, device=DEV, dtype=torch.int64)
    pos0 = torch.tensor([5, 6, 7, 8], device=DEV, dtype=torch.int32)
    counter = torch.tensor([9, 0], device=DEV, dtype=torch.int32)     # slot 0: the previous step's count
    step, col = 3, 13
    xf = x.float().cpu()
    out = ops.sample_select(x, top_k=1, seed=4, offset=2, eos_ids=eos, pad=pad, unfinished=unfinished, sequences=seq, col=col, positions0=pos0, step=step,
                            counter=counter)
    nxt = out["tokens"].cpu().tolist()
    assert nxt[0] == 11 and nxt[2] == pad
    for b in (1, 3):                                         # top_k = 1: one of the (possibly tied, in bf16) maxima
        assert xf[b, nxt[b]] == xf[b].max()
    assert seq[:, col].cpu().tolist() == nxt and (seq[:, :col] == -1).all() and (seq[:, col + 1:] == -1).all()
    still = [0, int(nxt[1] not in (11, 12)), 0, int(nxt[3] not in (11, 12))]
    assert unfinished.cpu().tolist() == still
    assert out["positions"].cpu().tolist() == [5 + step, 6 + step, 7 + step, 8 + step]
    assert counter.cpu().tolist() == [0, sum(still)]           # counter[step & 1] = rows still running; the other slot cleared
    with pytest.raises(ValueError):
        ops.sample_select(x, top_p=0.0)
    with pytest.raises(ValueError):
        ops.sample_select(x, temperature=0.0)


def _small(dtype, seed):
    from test_model_gpu import SMALL
    from ultravox_amd.config import UltravoxConfig
    from ultravox_amd.model import UltravoxModel
    return UltravoxModel(UltravoxConfig(**SMALL), device=DEV, dtype=dtype, seed=seed)


def test_f32_generate_with_top_k_1_equals_greedy():
    from ultravox_amd.generation import PhiloxGenerator
    model = _small(torch.float32, 3)
    ids = torch.randint(3, 500, (2, 12), generator=torch.Generator().manual_seed(16)).to(DEV)
    greedy = model.generate(input_ids=ids, max_new_tokens=8, eos_token_id=-1)
    gen = PhiloxGenerator(5)
    k1 = model.generate(input_ids=ids, max_new_tokens=8, eos_token_id=-1, do_sample=True, top_k=1, temperature=0.7, generator=gen)
    assert torch.equal(greedy, k1) and gen.offset == 8


def test_bf16_generate_under_a_philox_generator():
    """Mirrors test_generate_gpu.test_sampling_policies (model seed 3, input seed 16): the same seed replays the sequences, another seed gives others,
    every token under top_k = 5 is among the teacher-forced top 5 (up to the 5e-2 of bf16 decode-against-forward noise that
    test_bf16_decode_is_consistent_with_teacher_forced_forward allows); then the early stop, the KV state and the offset."""
    from ultravox_amd.generation import PhiloxGenerator
    from ultravox_amd.model import KVState
    model = _small(torch.bfloat16, 3)
    T, N = 12, 8
    ids = torch.randint(3, 500, (2, T), generator=torch.Generator().manual_seed(16)).to(DEV)
    kw = dict(input_ids=ids, max_new_tokens=N, do_sample=True, top_k=5, top_p=0.95)
    gen = PhiloxGenerator(1)
    a = model.generate(eos_token_id=-1, generator=gen, **kw)
    assert gen.offset == N and a.shape == (2, T + N)
    b = model.generate(eos_token_id=-1, generator=PhiloxGenerator(1), **kw)
    c = model.generate(eos_token_id=-1, generator=PhiloxGenerator(2), **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    cont = model.generate(eos_token_id=-1, generator=gen, **kw)      # the stream goes on: offsets 8.. draw other numbers
    assert gen.offset == 2 * N and not torch.equal(a, cont)
    logits = model.forward(input_ids=a[:, :-1]).logits.float()
    for t in range(T, a.shape[1]):
        fifth = torch.topk(logits[:, t - 1], 5, dim=-1).values[:, -1]
        got = logits[:, t - 1].gather(1, a[:, t:t + 1])[:, 0]
        assert bool((got >= fifth - 5e-2).all()), (t, got, fifth)
    # early stop: the token row 0 drew at step 3 becomes the terminator
    stop = int(a[0, T + 3])
    first = a[0, T:].tolist().index(stop)
    gen = PhiloxGenerator(1)
    out = model.generate(eos_token_id=stop, pad_token_id=1, generator=gen, return_dict_in_generate=True, **kw)
    row0 = out.sequences[0, T:].tolist()
    assert row0[:first + 1] == a[0, T:T + first + 1].tolist() and all(v == 1 for v in row0[first + 1:])
    n = out.sequences.shape[1] - T
    assert gen.offset == n
    if stop not in a[1, T:].tolist():                                 # the other row runs on, drawing what it drew before
        assert n == N and torch.equal(out.sequences[1], a[1])
    st = out.past_key_values
    greedy = model.generate(input_ids=ids, max_new_tokens=n, eos_token_id=-1, return_dict_in_generate=True).past_key_values
    assert isinstance(st, KVState) and st.cur_len == greedy.cur_len == T + n - 1 and torch.equal(st.pos_next, greedy.pos_next)
    assert torch.equal(st.tokens, out.sequences[:, :st.cur_len])
    for bad in (dict(repetition_penalty=1.2), dict(num_beams=2), dict(stopping_criteria=[lambda i, s: False])):
        with pytest.raises(ValueError, match="PhiloxGenerator"):
            model.generate(eos_token_id=-1, generator=gen, **kw, **bad)
    assert gen.offset == n


def test_local_inference_round_trip_with_a_sampler_seed():
    from fake_tokenizer import FakeChatTokenizer
    from oracle.reference_cpu import FeatureExtractorRef
    from ultravox_amd.inference import LocalInference, VoiceSample
    from ultravox_amd.processing import UltravoxProcessor

    class SmallVocabTokenizer(FakeChatTokenizer):
        """FakeChatTokenizer folded into the 512-token vocabulary of the SMALL model; terminator 2."""
        eos_token_id = 2
        added_tokens_encoder = {"<|eot_id|>": 2}

        def __init__(self):
            super().__init__()
            self._vocab = {self.eos_token: 2}

        def _tok(self, text):
            return [t if t == 2 else 10 + t % 400 for t in super()._tok(text)]
    model = _small(torch.bfloat16, 3)
    texts = []
    for seed in (9, 9, 10):
        tok = SmallVocabTokenizer()
        inf = LocalInference(model, UltravoxProcessor(FeatureExtractorRef(80), tokenizer=tok), tok, dtype=torch.bfloat16, sampler_seed=seed)
        out = inf.infer(VoiceSample.from_prompt("Tell me a long story"), max_tokens=12, temperature=1.0)
        assert 1 <= inf.sampler.offset <= 12 and inf.sampler.seed == seed
        first = inf.sampler.offset
        inf.infer(VoiceSample.from_prompt("Tell me a long story"), max_tokens=12, temperature=1.0)
        assert inf.sampler.offset > first                           # one stream per instance: the second call goes on where the first ended
        texts.append(out.text)
    assert texts[0] == texts[1] and texts[0] != texts[2]
