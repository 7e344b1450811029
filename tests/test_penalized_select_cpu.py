"""Greedy decoding under a repetition penalty, without a GPU: the reference of tests/penalized_util.py against [3P] HF's own processor bit for bit,
the argument checks of the two entry points (they answer before any GPU work), generate()'s penalised branch on the simulated device of
tests/test_generate_host_cpu.py, and the kernels' scratch segment (the kernels themselves: tests/test_penalized_select_gpu.py)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import penalized_util as PU
import ultravox_amd.model as M
from test_generate_host_cpu import D, V, FakeLib, left_padded
from ultravox_amd import _lib
from ultravox_amd.model import KVState, UltravoxModel


@pytest.mark.parametrize("bf16", [False, True])
def test_reference_equals_hf_repetition_penalty_processor(bf16):
    """4 x 4099 rows of 4 * randn (as f32, and rounded to bf16 first), ids with duplicates: penalized_util.penalized == RepetitionPenaltyLogitsProcessor
    in every bit, for penalties 1.1, 1.3, 50 and 0.5."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    Vv, B = 4099, 4
    g = torch.Generator().manual_seed(11)
    rows = 4 * torch.randn(B, Vv, generator=g)
    if bf16:
        rows = rows.bfloat16().float()
    ids = torch.randint(0, Vv, (B, 600), generator=g)
    ids[:, 300:400] = ids[:, :100]                   # duplicates
    ids[:, 0], ids[:, 1] = 0, Vv - 1
    for p in (1.1, 1.3, 50.0, 0.5):
        want = RepetitionPenaltyLogitsProcessor(p)(ids, rows.clone()).numpy()
        for b in range(B):
            got = PU.penalized(rows[b].numpy(), ids[b].numpy(), p)
            assert PU.same_bits(got, want[b]), (p, b)
            assert PU.argmax(got) == int(want[b].argmax())
    assert not PU.same_bits(PU.penalized(rows[0].numpy(), ids[0].numpy(), 1.3), rows[0].numpy())


def test_reference_helpers():
    bm = PU.bitmap([[0, 31, 32, 5, 5, -1, 70, 1 << 40], []], 70, words=4)
    assert bm.dtype == np.uint32 and bm.tolist() == [[(1 << 31) | (1 << 5) | 1, 1, 0, 0], [0, 0, 0, 0]]
    assert PU.ids_of(bm[0]).tolist() == [0, 5, 31, 32]
    s = PU.penalized(np.array([2.0, -2.0, np.nan, -0.0, np.inf, -np.inf], dtype=np.float32), [0, 1, 2, 3, 4, 5, 5, 9], 2.0)
    assert s[:2].tolist() == [1.0, -4.0] and np.isnan(s[2]) and np.signbit(s[3]) and s[3] == 0 and s[4] == np.inf and s[5] == -np.inf
    assert PU.argmax(np.array([np.nan, 1.0, 1.0], dtype=np.float32)) == 1 and PU.argmax(np.full(3, -np.inf, dtype=np.float32)) == 0
    assert PU.greedy_loop(np.array([3.0, 2.0, 1.0], dtype=np.float32), 50.0, 4) == [0, 1, 2, 0]


def _buf(n=64):
    return C.cast((C.c_uint8 * n)(), C.c_void_p)


def test_argument_errors_without_a_gpu():
    """Null buffers, penalty <= 0 (or not finite), too few bitmap words and col >= stride are argument / shape errors with uvx_last_error set - in
    that order of checks - and B == 0 is a no-op; nothing is launched."""
    lib = _lib.lib()
    a = _buf()        # one address that is never dereferenced: every call below returns before a launch
    mark = lambda ids, B, n, Vv, seen, words: lib.uvx_seen_mark(None, ids, 8, B, n, Vv, seen, words)
    assert mark(a, 2, 3, 100, None, 4) == -1 and b"seen_mark: null" in lib.uvx_last_error()
    assert mark(None, 2, 3, 100, a, 4) == -1 and b"seen_mark: null" in lib.uvx_last_error()
    assert mark(a, 2, 3, 100, a, 3) == -2 and b"words=3" in lib.uvx_last_error()            # ceil(100 / 32) = 4
    assert mark(a, 2, 3, 0, a, 4) == -2 and mark(a, 2, 3, 1 << 23, a, 1 << 18) == -2 and mark(a, -1, 3, 100, a, 4) == -2
    assert mark(a, 0, 3, 100, a, 4) == 0 and mark(a, 2, 0, 100, a, 4) == 0 and mark(None, 2, 0, 100, a, 4) == 0

    def sel(logits=a, B=2, Vv=100, penalty=1.3, seen=a, words=4, eos=None, n_eos=0, live=a, nxt=a, seq=a, stride=8, col=3, pos0=None, pos=None, step=0,
            counter=a, code=_lib.F32):
        return lib.uvx_greedy_select_penalized(None, code, logits, B, Vv, penalty, seen, words, None, eos, n_eos, 0, live, nxt, seq, stride, col, pos0, pos,
                                               step, counter)
    for kw in (dict(logits=None), dict(seen=None), dict(live=None), dict(nxt=None), dict(seq=None), dict(counter=None), dict(n_eos=1), dict(pos=a)):
        assert sel(**kw) == -1 and b"greedy_select_penalized: null" in lib.uvx_last_error(), kw
    assert sel(logits=None, penalty=-1.0, words=0) == -1 and b"null" in lib.uvx_last_error()        # the null check answers first
    assert sel(code=7) == -1 and b"logits_dtype=7" in lib.uvx_last_error()
    for kw in (dict(words=3), dict(col=8), dict(col=9), dict(col=-1), dict(Vv=0), dict(Vv=1 << 23, words=1 << 18), dict(B=-1), dict(step=-1), dict(n_eos=-1, eos=a)):
        assert sel(**kw) == -2 and b"greedy_select_penalized: B=" in lib.uvx_last_error(), kw
    assert sel(words=3, penalty=0.0) == -2                                                          # shape before penalty
    for p in (0.0, -1.3, float("inf"), float("nan")):
        assert sel(penalty=p) == -1 and b"penalty" in lib.uvx_last_error(), p
    assert sel(B=0) == 0 and sel(B=0, penalty=1.0) == 0
    with pytest.raises(ValueError, match="uvx_greedy_select_penalized"):
        _lib.check(sel(penalty=0.0), "uvx_greedy_select_penalized")


class PenalizedFakeLib(FakeLib):
    """FakeLib plus torch versions of uvx_seen_mark and uvx_greedy_select_penalized (include/uvx.h) that record their calls.  Its logits reach +5,
    so that a penalty on a seen winner changes the arg-max (FakeLib's own are all <= 0: a division leaves the 0 at the top where it is)."""

    @staticmethod
    def _logits(k, v, lo, hi, out):
        FakeLib._logits(k, v, lo, hi, out)
        out += 5.0

    @staticmethod
    def _bits(seen):
        return seen.numpy().view(np.uint32)            # (shares the tensor's memory)

    def uvx_argmax(self, *a):
        self.calls.append(("argmax",))
        return super().uvx_argmax(*a)

    def uvx_seen_mark(self, st, ids, stride, B, n, Vv, seen, words):
        self.calls.append(("mark", n, tuple(ids.shape)))
        assert ids.dtype == torch.int64 and int(stride.value) == ids.stride(0) and tuple(seen.shape) == (B, words) and words == (Vv + 31) // 32
        assert not seen.any()
        self._bits(seen)[:] = PU.bitmap(ids[:, :n].numpy(), Vv, words)
        return 0

    def uvx_greedy_select_penalized(self, st, code, logits, B, Vv, penalty, seen, words, scores_out, *book):
        self.calls.append(("select", penalty, int(book[7].value)))
        assert scores_out is None
        s = logits.float().clone()
        for b in range(B):
            s[b] = torch.from_numpy(PU.penalized(s[b].numpy(), PU.ids_of(self._bits(seen)[b]), penalty))
        rc = self.uvx_greedy_select(st, code, s, B, Vv, *book)
        bits = self._bits(seen)
        for b, t in enumerate(book[4].tolist()):        # book[4]: next_tokens, the tokens written
            if 0 <= t < Vv:
                bits[b, t >> 5] |= np.uint32(1 << (t & 31))
        return rc


@pytest.fixture()
def model(monkeypatch):
    fake = PenalizedFakeLib()
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
    m.fake = fake
    return m


class Rec:
    def __init__(self):
        self.puts, self.ended = [], False

    def put(self, v):
        self.puts.append(v.clone())

    def end(self):
        self.ended = True


def both(model, *a, **kw):
    """generate() with the switch off, then on -> (host result, device result, the double's calls of the device run)."""
    assert UltravoxModel.penalized_select is False and model.penalized_select is False       # an object that never ran __init__ keeps the host loop
    host = model.generate(*a, **kw)
    assert not [c for c in model.fake.calls if c[0] in ("mark", "select")]
    model.fake.calls.clear()
    model.penalized_select = True
    try:
        dev = model.generate(*a, **kw)
    finally:
        model.penalized_select = False
    calls = list(model.fake.calls)
    model.fake.calls.clear()
    return host, dev, calls


@pytest.mark.parametrize("p", [1.3, 50.0, 0.5])
def test_generate_penalised_device_loop_equals_the_host_loop(model, p):
    ids, am = left_padded(2, 9, [0, 3])
    N = 6
    plain = model.generate(ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1)
    model.fake.calls.clear()
    host, dev, calls = both(model, ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1, repetition_penalty=p)
    assert torch.equal(host, dev) and dev.shape == (2, 9 + N)
    if p == 50.0:
        assert not torch.equal(dev, plain)
    # one mark over the full prompt width, one penalised select per token at consecutive columns, no uvx_argmax, no plain select
    assert [c for c in calls if c[0] == "mark"] == [("mark", 9, (2, 9))]
    sel = [c for c in calls if c[0] == "select"]
    assert [c[2] for c in sel] == list(range(9, 9 + N)) and all(abs(c[1] - p) < 1e-12 for c in sel)
    assert not [c for c in calls if c[0] == "argmax"] and len([c for c in calls if c[0] == "decode"]) == N - 1
    # an early EOS with pad_token_id, and a streamer
    stop = int(dev[0, 9 + 2])
    first = dev[0, 9:].tolist().index(stop)
    ra, rb = Rec(), Rec()
    kw = dict(attention_mask=am, max_new_tokens=N, eos_token_id=[stop, 96], pad_token_id=1, repetition_penalty=p)
    host_s = model.generate(ids, streamer=ra, **kw)
    model.fake.calls.clear()
    model.penalized_select = True
    dev_s = model.generate(ids, streamer=rb, **kw)
    model.penalized_select = False
    assert torch.equal(host_s, dev_s) and dev_s[0, 9:9 + first + 1].tolist() == dev[0, 9:9 + first + 1].tolist()
    assert 1 in dev_s[0, 9 + first + 1:].tolist() or dev_s.shape[1] == 9 + first + 1                    # the finished row is padded while the other runs
    assert ra.ended and rb.ended and len(ra.puts) == len(rb.puts) == dev_s.shape[1] - 9 + 1
    assert all(torch.equal(x, y) for x, y in zip(ra.puts, rb.puts)) and torch.equal(rb.puts[0], ids)
    assert len([c for c in model.fake.calls if c[0] == "select"]) == dev_s.shape[1] - 9


def test_generate_penalised_second_turn_over_past_key_values(model):
    """return_dict_in_generate, then a second turn that reuses the cache: the chunk prefill sees only the new tokens, the bitmap is marked from the
    WHOLE input_ids (HF penalises every id of the row)."""
    p = 50.0
    ids1, am1 = left_padded(2, 9, [0, 3])
    h1, d1, _ = both(model, ids1, attention_mask=am1, max_new_tokens=5, eos_token_id=-1, repetition_penalty=p, return_dict_in_generate=True)
    assert torch.equal(h1.sequences, d1.sequences)
    sh, sd = h1.past_key_values, d1.past_key_values
    assert isinstance(sd, KVState) and (sd.cur_len, sd.Tmax) == (sh.cur_len, sh.Tmax) == (13, 14)
    assert torch.equal(sd.pos_next, sh.pos_next) and torch.equal(sd.kv_start, sh.kv_start) and torch.equal(sd.tokens, sh.tokens)
    ids2 = torch.cat([d1.sequences, torch.randint(3, V, (2, 6), generator=torch.Generator().manual_seed(1))], 1)
    am2 = torch.cat([am1, torch.ones(2, ids2.shape[1] - 9, dtype=torch.long)], 1)
    T2 = ids2.shape[1]
    fresh = model.generate(ids2, attention_mask=am2, max_new_tokens=4, eos_token_id=-1, repetition_penalty=p)
    model.fake.calls.clear()
    h2, d2, calls = both(model, ids2, attention_mask=am2, max_new_tokens=4, eos_token_id=-1, repetition_penalty=p, past_key_values=sd,
                         return_dict_in_generate=True)
    assert model.last_prefill_reused == 13 and calls[0] == ("chunk", 13, T2 - 13)
    assert [c for c in calls if c[0] == "mark"] == [("mark", T2, (2, T2))]
    assert torch.equal(d2.sequences, h2.sequences) and torch.equal(d2.sequences, fresh)
    assert d2.past_key_values.cur_len == h2.past_key_values.cur_len == T2 + 3
    # the penalty over the reused prefix matters here: without those ids other tokens come out
    assert not torch.equal(d2.sequences, model.generate(ids2, attention_mask=am2, max_new_tokens=4, eos_token_id=-1))


@pytest.mark.parametrize("kw", [dict(no_repeat_ngram_size=2), dict(stopping_criteria=[lambda i, s: False]), dict(do_sample=True, top_k=5),
                                dict(output_logits=True, return_dict_in_generate=True), dict(num_beams=2), dict(logits_processor=[lambda i, s: s])])
def test_other_configurations_keep_the_torch_path(model, kw):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    model.penalized_select = True
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, repetition_penalty=1.3, **kw)
    assert not [c for c in model.fake.calls if c[0] in ("mark", "select")]
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, **({} if "num_beams" in kw else kw))       # no penalty: none either
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, repetition_penalty=1.0)                   # 1.0 is no penalty: plain greedy
    assert not [c for c in model.fake.calls if c[0] in ("mark", "select")]


def test_the_environment_switch_turns_the_device_loop_off(model, monkeypatch):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    model.penalized_select = True
    want = model.generate(ids, attention_mask=am, max_new_tokens=4, eos_token_id=-1, repetition_penalty=50.0)
    assert [c[0] for c in model.fake.calls].count("select") == 4
    model.fake.calls.clear()
    monkeypatch.setenv("UVX_GREEDY_SELECT", "0")
    got = model.generate(ids, attention_mask=am, max_new_tokens=4, eos_token_id=-1, repetition_penalty=50.0)
    assert torch.equal(got, want) and not [c for c in model.fake.calls if c[0] in ("mark", "select")]


def test_score_processors_only_repetition_penalty():
    from ultravox_amd.generation import ScoreProcessors
    mk = lambda rep, **kw: ScoreProcessors(kw, 5, 8, [2], rep)
    assert mk(1.3).only_repetition_penalty and mk(1.3).active
    assert not mk(None).only_repetition_penalty and not mk(None).active
    for kw in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[4]]), dict(min_length=3), dict(min_new_tokens=2), dict(forced_eos_token_id=2),
               dict(suppress_tokens=[4]), dict(begin_suppress_tokens=[4]), dict(logits_processor=[lambda i, s: s])):
        assert not mk(1.3, **kw).only_repetition_penalty and mk(1.3, **kw).active, kw
        assert not mk(None, **kw).only_repetition_penalty
