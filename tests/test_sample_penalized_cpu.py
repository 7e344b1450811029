"""Sampling under a repetition penalty on the device, without a GPU: the composed reference of tests/test_sample_penalized_gpu.py against [3P] HF's own
processor and warpers in HF's order, generate()'s routing on the simulated device of tests/test_generate_host_cpu.py, UltravoxPipeline over a stub
model (and its preprocess against the reference's recorded one), the new entry point's argument checks and the kernels' resources (the kernel
itself: tests/test_sample_penalized_gpu.py)."""
import ctypes as C
import json
import logging
import os
import types

import numpy as np
import pytest
import torch

import penalized_util as PU
import sample_util as SU
import ultravox_amd.model as M
from test_generate_host_cpu import D, V, left_padded
from test_penalized_select_cpu import PenalizedFakeLib
from test_sample_cpu import SamplingFakeLib, grid
from ultravox_amd import _lib
from ultravox_amd.generation import PhiloxGenerator
from ultravox_amd.model import KVState, UltravoxModel


@pytest.mark.parametrize("Vv", [5, 1025])
def test_reference_keeps_what_hf_keeps_in_hf_order(Vv):
    """RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper of the installed
    transformers on tie-free f32 rows keep exactly RowRef's set over penalized_util.penalized + sample_util.x_of, and the kept scores agree to
    sample_util.bound, relatively (they are the same two f32 operations; torch may divide by multiplying with a reciprocal, one ulp away).
    This holds the test files' ORACLE to HF, not the kernel: it runs no code of the package and passes without the feature.  A setting whose
    reference boundary is closer than f32 resolves says nothing about either side and is left out; at least two thirds of the 360 settings of
    every (V, penalty) have to remain."""
    from transformers.generation import logits_process as LP
    g = np.random.default_rng(Vv)
    n = {1.3: 0, 0.75: 0}
    for row in range(3):
        logits = (g.standard_normal(Vv) * 3).astype(np.float32)
        ids = g.choice(Vv, size=max(2, Vv // 4), replace=False)
        ids = np.concatenate([ids, ids[:2], [int(logits.argmax())]])            # duplicates; the top token is seen
        for pen in (1.3, 0.75):
            scored = PU.penalized(logits, ids, pen)
            assert len(np.unique(scored)) == Vv, "precondition: a tie-free row behind the penalty"
            refs = {t: SU.RowRef(SU.x_of(scored, t)) for t in (1.0, 0.7)}
            for t, k, p, mp, keep in grid(Vv):
                s = LP.RepetitionPenaltyLogitsProcessor(pen)(torch.from_numpy(ids)[None], torch.from_numpy(logits)[None].clone())
                if t != 1.0:
                    s = LP.TemperatureLogitsWarper(t)(None, s)
                if k > 0:
                    s = LP.TopKLogitsWarper(k, min_tokens_to_keep=keep)(None, s)
                if p < 1.0:
                    s = LP.TopPLogitsWarper(p, min_tokens_to_keep=keep)(None, s)
                if mp > 0.0:
                    s = LP.MinPLogitsWarper(mp, min_tokens_to_keep=keep)(None, s)
                ref = refs[t].warp(k, p, mp, keep)
                if not SU.margins_ok(ref):          # (f32 HF against f64 at a boundary closer than f32 resolves: not a statement about either)
                    continue
                n[pen] += 1
                kept = ref["kept"]
                assert np.array_equal(kept, torch.isfinite(s[0]).numpy()), (row, pen, t, k, p, mp, keep)
                x = refs[t].x[kept]
                assert (np.abs(s[0].numpy().astype(np.float64)[kept] - x) <= SU.bound(int(kept.sum())) * np.abs(x)).all(), (row, pen, t, k, p, mp, keep)
                want = torch.softmax(s[0].double(), -1).numpy()
                assert (np.abs(ref["probs"] - want) <= SU.bound(int(kept.sum())) * want).all(), (row, pen, t, k, p, mp, keep)
    assert min(n.values()) >= 240, n            # the margins hold almost everywhere on such rows


def _buf(n=64):
    return C.cast((C.c_uint8 * n)(), C.c_void_p)


def test_argument_errors_without_a_gpu():
    """The checks of both parents, null pointers first; nothing is launched."""
    lib = _lib.lib()
    a = _buf()        # one address that is never dereferenced: every call below returns before a launch

    def sel(logits=a, B=2, Vv=100, penalty=1.3, seen=a, words=4, t=0.7, k=0, p=0.9, mp=0.0, keep=1, eos=None, n_eos=0, live=a, nxt=a, seq=a, stride=8,
            col=3, pos0=None, pos=None, step=0, counter=a, code=_lib.F32):
        return lib.uvx_sample_select_penalized(None, code, logits, B, Vv, penalty, seen, words, t, k, p, mp, keep, 1, 0, None, None, eos, n_eos, 0, live,
                                               nxt, seq, stride, col, pos0, pos, step, counter)
    for kw in (dict(logits=None), dict(seen=None), dict(live=None), dict(nxt=None), dict(seq=None), dict(counter=None), dict(n_eos=1), dict(pos=a)):
        assert sel(**kw) == -1 and b"sample_select_penalized: null" in lib.uvx_last_error(), kw
    assert sel(logits=None, penalty=-1.0, words=0, t=0.0) == -1 and b"null" in lib.uvx_last_error()        # the null check answers first
    assert sel(code=7) == -1 and b"logits_dtype=7" in lib.uvx_last_error()
    for kw in (dict(words=3), dict(col=8), dict(col=-1), dict(Vv=0), dict(Vv=1 << 23, words=1 << 18), dict(B=-1), dict(step=-1), dict(n_eos=-1, eos=a)):
        assert sel(**kw) == -2 and b"sample_select_penalized: B=" in lib.uvx_last_error(), kw
    for pen in (0.0, -1.3, float("inf"), float("nan")):
        assert sel(penalty=pen) == -1 and b"penalty" in lib.uvx_last_error(), pen
    for kw in (dict(t=0.0), dict(k=-1), dict(p=0.0), dict(p=1.5), dict(mp=-0.1), dict(mp=1.5), dict(keep=0)):
        assert sel(**kw) == -1 and b"sample_select_penalized: temperature=" in lib.uvx_last_error(), kw
    assert sel(B=0) == 0
    with pytest.raises(ValueError, match="uvx_sample_select_penalized"):
        _lib.check(sel(penalty=0.0), "uvx_sample_select_penalized")


class Fake(PenalizedFakeLib, SamplingFakeLib):
    """The simulated device with uvx_seen_mark, both greedy selects and uvx_sample_select, plus a stand-in for uvx_sample_select_penalized that
    records its arguments and picks the penalised arg-max (include/uvx.h for the rest)."""

    def uvx_sample_select_penalized(self, st, code, logits, B, Vv, penalty, seen, words, temperature, top_k, top_p, min_p, min_keep, seed, offset,
                                    uniforms, probs, *book):
        self.calls.append(("psample", dict(penalty=penalty, words=words, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                                           min_keep=min_keep, seed=seed, offset=offset, col=int(book[7].value))))
        assert uniforms is None and probs is None and tuple(seen.shape) == (B, words)
        n = len(self.calls)
        rc = self.uvx_greedy_select_penalized(st, code, logits, B, Vv, penalty, seen, words, None, *book)
        del self.calls[n:]            # (the inner stand-in's own record)
        return rc


@pytest.fixture()
def model(monkeypatch):
    fake = Fake()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(M, "ptr", lambda t: t)
    monkeypatch.setattr(M, "stream_ptr", lambda: None)
    monkeypatch.setattr(M, "check", lambda rc, what="": None)
    monkeypatch.setattr(M.C, "byref", lambda x: x)
    monkeypatch.setattr(M.C, "c_size_t", lambda x: x)
    m = UltravoxModel.__new__(UltravoxModel)
    m.device, m.dtype, m.code, m.text_lora_r = torch.device("cpu"), torch.float32, 0, 0
    m.config = types.SimpleNamespace(vocab_size=V, text_config=types.SimpleNamespace(eos_token_id=2, hidden_size=D))
    table = (torch.arange(V, dtype=torch.float32)[:, None] + 1.0).repeat(1, D)
    m._llm = {"rope_len": 4096, "embed": table}
    m._c = types.SimpleNamespace(llm_layers=1)
    m._lw, m._ws = None, {}
    m._embed_merge = lambda emb, ids, *a: table[ids]
    m.penalized_select = True
    m.fake = fake
    return m


def names(model):
    return [c[0] for c in model.fake.calls]


def test_generate_routes_a_flagged_generator_and_a_penalty_to_the_new_entry_point(model):
    """One uvx_seen_mark over the WHOLE input_ids, one uvx_sample_select_penalized per token with the penalty, the words and offsets o, o + 1, ..,
    the generator advanced, the KVState of the greedy loop."""
    ids, am = left_padded(2, 9, [0, 3])
    N, p = 5, 50.0
    gen = PhiloxGenerator(77, penalty_on_device=True).advance(10)
    kw = dict(attention_mask=am, max_new_tokens=N, eos_token_id=-1, repetition_penalty=p, return_dict_in_generate=True)
    out = model.generate(ids, do_sample=True, temperature=0.6, top_p=0.9, generator=gen, **kw)
    calls = list(model.fake.calls)
    assert [c for c in calls if c[0] == "mark"] == [("mark", 9, (2, 9))]
    ps = [c[1] for c in calls if c[0] == "psample"]
    assert [c["offset"] for c in ps] == [10, 11, 12, 13, 14] and gen.offset == 15 and {c["seed"] for c in ps} == {77}
    assert [c["col"] for c in ps] == list(range(9, 9 + N)) and {c["words"] for c in ps} == {(V + 31) // 32}
    assert all(abs(c["penalty"] - p) < 1e-12 and abs(c["temperature"] - 0.6) < 1e-7 and c["top_k"] == 0 and abs(c["top_p"] - 0.9) < 1e-7
               and c["min_p"] == 0.0 and c["min_keep"] == 1 for c in ps)
    assert not {"sample", "select", "argmax"} & set(names(model)) and names(model).count("decode") == N - 1
    model.fake.calls.clear()
    greedy = model.generate(ids, **kw)                            # the greedy penalised device loop; the stand-in above picks the same arg-max
    assert "select" in names(model) and "psample" not in names(model)
    assert torch.equal(out.sequences, greedy.sequences) and not torch.equal(out.sequences, model.generate(ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1))
    st, sg = out.past_key_values, greedy.past_key_values
    assert isinstance(st, KVState) and (st.cur_len, st.Tmax) == (sg.cur_len, sg.Tmax) == (13, 14)
    assert torch.equal(st.pos_next, sg.pos_next) and torch.equal(st.kv_start, sg.kv_start) and torch.equal(st.tokens, sg.tokens)
    # an early stop: fewer steps run, the offset follows them
    stop = int(out.sequences[0, 9 + 1])
    early = model.generate(ids[:1], max_new_tokens=N, eos_token_id=stop, do_sample=True, top_k=3, min_p=0.05, generator=gen, repetition_penalty=p)
    n = early.shape[1] - 9
    assert n < N and gen.offset == 15 + n
    assert [c[1] for c in model.fake.calls if c[0] == "psample"][-1]["top_k"] == 3
    # a second turn over past_key_values: the chunk prefill sees the new tokens only, the mark the whole row
    ids2 = torch.cat([out.sequences, torch.randint(3, V, (2, 6), generator=torch.Generator().manual_seed(1))], 1)
    am2 = torch.cat([am, torch.ones(2, ids2.shape[1] - 9, dtype=torch.long)], 1)
    T2 = ids2.shape[1]
    model.fake.calls.clear()
    model.generate(ids2, attention_mask=am2, max_new_tokens=4, eos_token_id=-1, do_sample=True, generator=gen, repetition_penalty=p, past_key_values=st)
    assert model.last_prefill_reused == 13 and model.fake.calls[0] == ("chunk", 13, T2 - 13)
    assert [c for c in model.fake.calls if c[0] == "mark"] == [("mark", T2, (2, T2))] and names(model).count("psample") == 4


def test_the_other_calls_never_reach_the_new_entry_point(model):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    kw = dict(attention_mask=am, max_new_tokens=3, eos_token_id=-1)
    flagged = PhiloxGenerator(3, penalty_on_device=True)
    model.generate(ids, do_sample=True, top_k=5, generator=flagged, **kw)                                   # the flag without a penalty: uvx_sample_select
    model.generate(ids, do_sample=True, top_k=5, generator=flagged, repetition_penalty=1.0, **kw)           # 1.0 is no penalty
    assert names(model).count("sample") == 6 and flagged.offset == 6 and "mark" not in names(model)
    model.generate(ids, do_sample=True, top_k=5, generator=PhiloxGenerator(3), **kw)                        # a plain PhiloxGenerator
    model.generate(ids, do_sample=True, top_k=5, generator=torch.Generator().manual_seed(0), repetition_penalty=1.3, **kw)    # torch's sampler
    model.generate(ids, do_sample=True, top_k=5, repetition_penalty=1.3, **kw)
    model.generate(ids, repetition_penalty=1.3, **kw)                                                       # greedy + penalty: its own select
    model.generate(ids, repetition_penalty=1.3, generator=flagged, **kw)                                    # greedy: the generator is not consulted
    model.generate(ids, **kw)
    assert "psample" not in names(model) and flagged.offset == 6
    plain = PhiloxGenerator(1)
    with pytest.raises(ValueError, match="PhiloxGenerator.*score processors"):                              # without the flag nothing changes
        model.generate(ids, do_sample=True, generator=plain, repetition_penalty=1.3, **kw)
    assert plain.offset == 0 and "psample" not in names(model)


@pytest.mark.parametrize("kw, name", [(dict(repetition_penalty=1.3, no_repeat_ngram_size=2), "score processors"),
                                      (dict(repetition_penalty=1.3, logits_processor=[lambda i, s: s]), "score processors"),
                                      (dict(repetition_penalty=1.3, suppress_tokens=[4]), "score processors"),
                                      (dict(no_repeat_ngram_size=2), "score processors"),
                                      (dict(repetition_penalty=1e39), "score processors"),                  # not a finite f32
                                      (dict(repetition_penalty=1.3, stopping_criteria=[lambda i, s: False]), "stopping_criteria"),
                                      (dict(repetition_penalty=1.3, output_logits=True, return_dict_in_generate=True), "output_logits"),
                                      (dict(repetition_penalty=1.3, num_beams=2), "num_beams")])
def test_a_flagged_generator_refuses_what_the_kernel_does_not_do(model, kw, name):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    gen = PhiloxGenerator(1, penalty_on_device=True)
    with pytest.raises(ValueError, match=f"PhiloxGenerator.*{name}"):
        model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, generator=gen, **kw)
    assert gen.offset == 0 and not model.fake.calls
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, generator=torch.Generator().manual_seed(0), **kw)    # the torch path takes them
    assert "psample" not in names(model)


def test_philox_generator_flag():
    assert PhiloxGenerator(5).penalty_on_device is False and PhiloxGenerator().penalty_on_device is False
    g = PhiloxGenerator(5, penalty_on_device=True)
    assert g.penalty_on_device is True and (g.seed, g.offset) == (5, 0)
    assert g.manual_seed(7).penalty_on_device is True and g.advance(3).offset == 3


# ---- UltravoxPipeline over a stub model ----

class StubModel:
    device = torch.device("cpu")
    config = types.SimpleNamespace(stack_factor=8)
    audio_tower_context_length = 3000

    def __init__(self, dtype=torch.float32):
        self.dtype, self.seen = dtype, []

    def generate(self, **kw):
        self.seen.append(kw)
        ids = kw["input_ids"]
        new = torch.tensor([[4242, 77, 128009], [1, 2, 3]])
        return torch.cat([torch.cat([ids, ids + 1]), new], 1)       # two rows: only row 0's new tokens may come back


class RecordingProcessor:
    """What preprocess hands to the processor."""

    def __init__(self, tokenizer):
        self.tokenizer, self.calls = tokenizer, []

    def __call__(self, **kw):
        self.calls.append(kw)
        return {"input_ids": torch.tensor([[5, 6, 7]]), "attention_mask": torch.ones(1, 3, dtype=torch.long), "audio_values": torch.zeros(1, 80, 8)}


def _pipe(dtype=torch.float32, recording=False, **kw):
    from fake_tokenizer import FakeChatTokenizer
    from oracle.reference_cpu import FeatureExtractorRef
    from ultravox_amd.pipeline import UltravoxPipeline
    tok = FakeChatTokenizer()
    tok.pad_token_id = tok.eos_token_id
    extra = dict(processor=RecordingProcessor(tok)) if recording else dict(audio_processor=FeatureExtractorRef(80))
    return UltravoxPipeline(StubModel(dtype), tok, **extra, **kw)


def test_pipeline_constructor():
    from ultravox_amd.processing import UltravoxProcessor
    pipe = _pipe(chat_template="TEMPLATE")
    assert isinstance(pipe.processor, UltravoxProcessor) and pipe.processor.tokenizer is pipe.tokenizer
    assert pipe.processor.stack_factor == 8 and pipe.processor.audio_context_size == 3000
    assert pipe.tokenizer.chat_template == "TEMPLATE" and pipe.sampler is None
    assert not hasattr(_pipe().tokenizer, "chat_template")
    given = _pipe(recording=True, sampler_seed=4)
    assert isinstance(given.processor, RecordingProcessor)
    assert isinstance(given.sampler, PhiloxGenerator) and given.sampler.seed == 4 and given.sampler.penalty_on_device


def test_pipeline_audio_conversions_are_exact():
    """float64 -> float32; int16 / 32768; int32 / 2147483648, each one f32 operation; float32 and tensors pass as they are; the sampling rate
    defaults to 16000; audio_values takes the model's dtype."""
    pipe = _pipe(torch.bfloat16, recording=True)
    g = np.random.default_rng(0)
    f64 = g.standard_normal(100)
    i16 = g.integers(-32768, 32768, 100).astype(np.int16)
    i32 = g.integers(-2 ** 31, 2 ** 31, 100).astype(np.int32)
    f32 = f64.astype(np.float32)
    for audio, want in ((f64, f64.astype(np.float32)), (i16, i16.astype(np.float32) / np.float32(32768.0)),
                        (i32, i32.astype(np.float32) / np.float32(2147483648.0)), (f32, f32)):
        out = pipe.preprocess({"audio": audio, "sampling_rate": 8000})
        got = pipe.processor.calls[-1]
        assert got["audio"].dtype == np.float32 and np.array_equal(got["audio"].view(np.uint32), want.view(np.uint32)) and got["sampling_rate"] == 8000
        assert out["audio_values"].dtype == torch.bfloat16
    assert np.array_equal(pipe.processor.calls[1]["audio"], i16 / 32768.0) and pipe.processor.calls[1]["audio"].min() >= -1.0
    t = torch.zeros(50)
    pipe.preprocess({"audio": t})
    assert pipe.processor.calls[-1]["audio"] is t and pipe.processor.calls[-1]["sampling_rate"] == 16000
    pipe.preprocess({"turns": [{"role": "user", "content": "Hi"}]})
    assert pipe.processor.calls[-1]["audio"] is None and pipe.processor.calls[-1]["sampling_rate"] == 16000


def test_pipeline_turn_prompt_and_placeholder_rules(caplog):
    pipe = _pipe(recording=True)
    audio = np.zeros(400, dtype=np.float32)
    text = lambda: pipe.processor.calls[-1]["text"]
    template = pipe.tokenizer.apply_chat_template
    NO_PH, NO_SR = "Prompt does not contain '<|audio|>'", "No sampling rate provided"
    with caplog.at_level(logging.WARNING):
        turns = []
        pipe.preprocess({"audio": audio, "turns": turns, "sampling_rate": 16000})          # no turns: one user turn holding the placeholder
        assert turns == [{"role": "user", "content": "<|audio|>"}] and text() == template(turns, add_generation_prompt=True)
        assert text().endswith("<|start_header_id|>assistant<|end_header_id|>\n\n") and not caplog.records
        turns = [{"role": "user", "content": "Hello"}, {"role": "assistant", "content": "Hi"}]
        pipe.preprocess({"audio": audio, "turns": turns, "prompt": "Transcribe <|audio|> now", "sampling_rate": 16000})
        assert turns[-1] == {"role": "user", "content": "Transcribe <|audio|> now"} and len(turns) == 3 and not caplog.records
        turns = [{"role": "system", "content": "S"}, {"role": "user", "content": "Hear <|audio|>"}]
        pipe.preprocess({"audio": audio, "turns": turns, "prompt": "ignored", "sampling_rate": 16000})       # the last turn is the user's: nothing added
        assert len(turns) == 2 and "ignored" not in text() and not caplog.records
        turns = []
        pipe.preprocess({"audio": audio, "turns": turns, "prompt": "What is said ?", "sampling_rate": 16000})
        assert turns == [{"role": "user", "content": "What is said ? <|audio|>"}]
        assert [r.getMessage() for r in caplog.records if NO_PH in r.getMessage()] and not [r for r in caplog.records if NO_SR in r.getMessage()]
        caplog.clear()
        pipe.preprocess({"audio": audio})                                                                 # no sampling rate with audio: the second warning
        assert len(caplog.records) == 1 and NO_SR in caplog.records[0].getMessage()
        caplog.clear()
        turns = [{"role": "user", "content": "Only text"}]
        pipe.preprocess({"turns": turns, "prompt": "unused"})                                             # no audio: no turn added, no warning
        assert len(turns) == 1 and text() == template(turns, add_generation_prompt=True) and not caplog.records


def test_pipeline_sanitize_parameters_and_generate_keywords():
    pipe = _pipe(recording=True)
    pre, fwd, post = pipe._sanitize_parameters(temperature=0.5, max_new_tokens=7, repetition_penalty=1.3, top_k=5, do_sample=True, foo=1)
    assert pre == {} and post == {} and fwd == dict(temperature=0.5, max_new_tokens=7, repetition_penalty=1.3)
    assert pipe._sanitize_parameters() == ({}, {}, {})
    inputs = lambda: {"turns": [{"role": "user", "content": "Hi"}]}
    seen = pipe.model.seen
    # no temperature: greedy under the default penalty; max_new_tokens left out, so that generate()'s own default applies
    reply = pipe(inputs(), top_k=5)
    kw = seen[-1]
    assert kw["do_sample"] is False and kw["repetition_penalty"] == 1.1 and kw["eos_token_id"] == [128009]                   # eos and <|eot_id|> are one id here: listed once
    assert not {"temperature", "generator", "max_new_tokens", "top_k"} & set(kw)
    assert set(kw) == {"input_ids", "attention_mask", "audio_values", "do_sample", "repetition_penalty", "eos_token_id"}
    assert isinstance(reply, str) and reply == pipe.tokenizer.decode([4242, 77, 128009], skip_special_tokens=True) == "<4242><77>"      # row 0's new tokens
    pipe(inputs(), temperature=0, max_new_tokens=30)                  # temperature 0 is no temperature
    assert seen[-1]["do_sample"] is False and seen[-1]["max_new_tokens"] == 30 and "temperature" not in seen[-1]
    # a temperature without a sampler seed: torch's sampler
    pipe(inputs(), temperature=0.7, repetition_penalty=1.0)
    assert seen[-1]["do_sample"] is True and seen[-1]["temperature"] == 0.7 and seen[-1]["repetition_penalty"] == 1.0 and "generator" not in seen[-1]
    # with one: the pipeline's own flagged generator, on sampled calls only
    seeded = _pipe(recording=True, sampler_seed=11)
    seeded(inputs(), temperature=0.7)
    seeded(inputs(), temperature=0.7)
    seeded(inputs())
    a, b, c = seeded.model.seen
    assert a["generator"] is b["generator"] is seeded.sampler and a["do_sample"] and a["repetition_penalty"] == 1.1
    assert "generator" not in c and c["do_sample"] is False
    # <|eot_id|> as an id of its own joins the eos; a tokenizer without it: its eos alone
    pipe.tokenizer.added_tokens_encoder = {"<|eot_id|>": 128001}
    pipe(inputs())
    assert seen[-1]["eos_token_id"] == [128009, 128001]
    pipe.tokenizer.added_tokens_encoder = {}
    pipe(inputs())
    assert seen[-1]["eos_token_id"] == [128009]


def test_pipeline_preprocess_agrees_with_the_recorded_reference(golden_dir):
    """The reference's own UltravoxPipeline.preprocess ran on the cases of tests/golden/make_pipeline_golden.py; its integer outputs, the shape,
    dtype and every 97th value of audio_values, the turns it left in the caller's list and its warnings are recorded in
    pipeline_preprocess_reference.json (the recorded form of a comparison against the live reference: it runs where the reference is not at
    hand).  Integers, turns and warnings exactly; audio_values to the 2e-4 that tests/test_processing_live_reference.py allows between this
    package's feature extractor and the HF WhisperFeatureExtractor the reference ran."""
    from golden.make_pipeline_golden import cases, record
    with open(os.path.join(golden_dir, "pipeline_preprocess_reference.json")) as f:
        want = json.load(f)
    pipe = _pipe(torch.float32)
    made = cases()
    assert set(made) == set(want) and len(want) == 9
    for name, inputs in made.items():
        got = record(pipe.preprocess, inputs)
        assert got["turns"] == want[name]["turns"] and got["warnings"] == want[name]["warnings"], name
        assert set(got["out"]) == set(want[name]["out"]), (name, sorted(got["out"]), sorted(want[name]["out"]))
        for k, w in want[name]["out"].items():
            g = got["out"][k]
            if k == "audio_values":
                assert (g["dtype"], g["shape"]) == (w["dtype"], w["shape"]) and len(w["sampled"]) >= 40, name
                assert np.allclose(g["sampled"], w["sampled"], rtol=0, atol=2e-4), (name, float(np.abs(np.array(g["sampled"]) - w["sampled"]).max()))
            else:
                assert g == w, (name, k)
