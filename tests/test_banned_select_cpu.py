"""The token-ban score processors on the device, without a GPU: the reference of tests/ban_util.py against [3P] transformers' own processors bit for
bit, the argument checks of the two entry points (they answer before any GPU work), generate()'s banned branch and its routing on the simulated
device of tests/test_generate_host_cpu.py, and the kernels' scratch segment (the kernels themselves: tests/test_banned_select_gpu.py)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import ban_util as BU
import penalized_util as PU
import ultravox_amd.model as M
from test_generate_host_cpu import D, V, left_padded
from test_penalized_select_cpu import PenalizedFakeLib, Rec
from ultravox_amd import _lib
from ultravox_amd.generation import PhiloxGenerator, ScoreProcessors
from ultravox_amd.model import KVState, UltravoxModel

VS = [1, 7, 33, 1024, 1032, 1025, 4099, 131077]


def _hf_equals_reference(case_rows, rules, L, prompt_len, max_len, scores, penalty=None):
    lp = BU.hf_processors(rules, prompt_len, max_len, penalty)
    want = lp(torch.from_numpy(np.ascontiguousarray(case_rows)), torch.from_numpy(scores.copy())).numpy()
    for b in range(len(case_rows)):
        mask, forced = BU.banned(case_rows[b], rules, L, prompt_len, max_len)
        s = scores[b] if penalty is None else PU.penalized(scores[b], case_rows[b], penalty)
        assert PU.same_bits(BU.apply(s, mask, forced), want[b]), b


@pytest.mark.parametrize("Vv", VS)
def test_reference_equals_hf_processors_on_the_rule_edges(Vv):
    """Every edge case the kernel tests use (ban_util.edge_cases) that transformers accepts: the reference's scores equal the processor list's in
    every bit, alone and behind a repetition penalty."""
    scores = (4 * np.random.default_rng(Vv).standard_normal((3, Vv))).astype(np.float32)
    cases = BU.edge_cases(Vv)
    assert sum(c.hf for c in cases) >= 30 and sum(not c.hf for c in cases) >= 6
    for c in cases:
        if c.hf and c.L > 0:           # (HF's processors want at least one id in the row)
            _hf_equals_reference(c.rows, c.rules, c.L, c.prompt_len, c.max_len, scores)
            _hf_equals_reference(c.rows, c.rules, c.L, c.prompt_len, c.max_len, scores, penalty=1.3)


def random_rules(g, Vv, L, prompt_len):
    pick = lambda n: [int(t) for t in g.integers(0, Vv, size=n)]
    on = lambda: g.random() < 0.5
    return BU.Rules(Vv, ngram=int(g.integers(1, 4)) if on() else 0,
                    bad_words=[pick(int(g.integers(1, 4))) for _ in range(int(g.integers(1, 6)))] if on() else [],
                    eos=pick(2), min_length=int(g.integers(L - 2, L + 3)) if on() else 0, min_new=int(g.integers(0, 4)) if on() else 0,
                    forced=pick(int(g.integers(1, 3))) if on() else (), suppress=pick(int(g.integers(1, 8))) if on() else (),
                    begin=pick(int(g.integers(1, 4))) if on() else ())


def test_reference_equals_hf_processors_on_random_rule_sets():
    """Random finite rows over a small vocabulary (so that n-grams and bad-word tails do match), random rule sets, every step kind: the forced
    step, the first step, steps under the min-length rules."""
    g = np.random.default_rng(5)
    kinds = set()
    for trial in range(300):
        Vv, L = int(g.choice([5, 11, 97])), int(g.integers(1, 20))
        prompt_len = int(g.integers(max(L - 3, 0), L + 1))
        max_len = L + int(g.integers(1, 4))
        rows = g.integers(0, Vv, size=(3, L)).astype(np.int64)
        rules = random_rules(g, Vv, L, prompt_len)
        kinds.add(rules.flags(L, prompt_len, max_len))
        scores = (4 * g.standard_normal((3, Vv))).astype(np.float32)
        _hf_equals_reference(rows, rules, L, prompt_len, max_len, scores, penalty=1.2 if trial % 2 else None)
    assert kinds == set(range(8))


def test_score_processors_device_rules_and_flags_restate_call():
    """generation.ScoreProcessors: the uploaded lists and the per-step flags, interpreted by the reference, give the scores of its own __call__."""
    g = np.random.default_rng(8)
    for trial in range(60):
        Vv, L = 97, int(g.integers(1, 16))
        prompt_len = int(g.integers(max(L - 3, 0), L + 1))
        max_new = L - prompt_len + int(g.integers(1, 4))
        r = random_rules(g, Vv, L, prompt_len)
        kw = dict(no_repeat_ngram_size=r.ngram, bad_words_ids=[list(w) for w in r.bad_words], min_length=r.min_length, min_new_tokens=r.min_new,
                  forced_eos_token_id=list(r.forced), suppress_tokens=list(r.suppress), begin_suppress_tokens=list(r.begin))
        procs = ScoreProcessors(kw, prompt_len, max_new, list(r.eos), None)
        rows = torch.from_numpy(g.integers(0, Vv, size=(2, L)).astype(np.int64))
        scores = torch.from_numpy((4 * g.standard_normal((2, Vv))).astype(np.float32))
        assert procs.step_flags(L) == r.flags(L, prompt_len, prompt_len + max_new)
        if not procs.bans:
            assert not procs.on_device(Vv)
            continue
        assert procs.on_device(Vv)
        t = procs.device_rules("cpu")
        lst = lambda v: [] if v is None else v.tolist()
        offs, toks = lst(t["bad_offsets"]), lst(t["bad_tokens"])
        assert (t["n_bad"], t["n_bad_tokens"]) == (max(len(offs) - 1, 0), len(toks))
        assert [t["n_min"], t["n_forced"], t["n_suppress"], t["n_begin"]] == [len(lst(t[k])) for k in ("min_ids", "forced_ids", "suppress_ids", "begin_ids")]
        words = [toks[offs[i]:offs[i + 1]] for i in range(t["n_bad"])]
        want = procs(rows, scores.clone()).numpy()
        for b in range(2):
            mask = BU.banned_by_flags(rows[b].tolist(), Vv, t["ngram"], words, lst(t["min_ids"]), lst(t["forced_ids"]), lst(t["suppress_ids"]),
                                      lst(t["begin_ids"]), procs.step_flags(L))
            assert PU.same_bits(BU.apply(scores[b].numpy(), mask, bool(procs.step_flags(L) & 2)), want[b])
    mk = lambda **kw: ScoreProcessors(kw, 5, 8, [2], None)
    assert not mk(suppress_tokens=[4], logits_processor=[lambda i, s: s]).on_device(97)            # a caller's processor keeps the host
    assert not mk(suppress_tokens=[97]).on_device(97) and not mk(bad_words_ids=[[3, 200]]).on_device(97) and mk(bad_words_ids=[[3, 96]]).on_device(97)
    assert not ScoreProcessors({}, 5, 8, [2], 1.3).on_device(97)                                     # the penalty alone is the penalised selectors' case
    assert mk(bad_words_ids=[[2]]).device_rules("cpu")["n_bad"] == 0                               # a lone EOS entry is dropped


def _buf(n=64):
    return C.cast((C.c_uint8 * n)(), C.c_void_p)


def test_struct_mirror_matches_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uvx.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} uvx_ban_rules_t;", src, re.S).group(1), flags=re.S)
    fields = [n.strip(" *") for decl in re.findall(r"(?:const int64_t\*|const int32_t\*|int32_t)\s+([^;]+);", body) for n in decl.split(",")]
    assert fields == [f[0] for f in _lib.BanRules._fields_] and C.sizeof(_lib.BanRules) == 6 * 8 + 8 * 4
    assert (_lib.BAN_MIN, _lib.BAN_FORCED, _lib.BAN_BEGIN) == (BU.BAN_MIN, BU.BAN_FORCED, BU.BAN_BEGIN) == \
        tuple(int(re.search(rf"#define UVX_BAN_{n} (\d+)u", src).group(1)) for n in ("MIN", "FORCED", "BEGIN"))


@pytest.mark.parametrize("entry", ["greedy", "sample"])
def test_argument_errors_without_a_gpu(entry):
    """Null buffers first, then shape (too few ban or seen words, col >= stride, V >= 2^23), then values (penalty, warpers, negative counts, a null
    list with a count, unknown flag bits), each with uvx_last_error set under the entry's short name; B == 0 is a no-op; nothing is launched."""
    lib = _lib.lib()
    a = _buf()        # one address that is never dereferenced: every call below returns before a launch
    short = f"{entry}_select_banned".encode()
    ok_rules = _lib.BanRules(ngram=2, suppress_ids=a, n_suppress=3)

    def sel(logits=a, B=2, Vv=100, penalty=1.3, seen=a, words=4, rules=ok_rules, flags=0, ban=a, ban_words=4, eos=None, n_eos=0, live=a, nxt=a, seq=a,
            stride=8, col=3, pos0=None, pos=None, step=0, counter=a, code=_lib.F32, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, min_keep=1):
        r = None if rules is None else C.byref(rules)
        book = (eos, n_eos, 0, live, nxt, seq, stride, col, pos0, pos, step, counter)
        if entry == "greedy":
            return lib.uvx_greedy_select_banned(None, code, logits, B, Vv, penalty, seen, words, None, r, flags, ban, ban_words, *book)
        return lib.uvx_sample_select_banned(None, code, logits, B, Vv, penalty, seen, words, temperature, top_k, top_p, min_p, min_keep, 1, 0, None, None,
                                            r, flags, ban, ban_words, *book)
    err = lambda: lib.uvx_last_error()
    for kw in (dict(logits=None), dict(rules=None), dict(ban=None), dict(live=None), dict(nxt=None), dict(seq=None), dict(counter=None), dict(n_eos=1),
               dict(pos=a)):
        assert sel(**kw) == -1 and short + b": null" in err(), kw
    assert sel(logits=None, penalty=-1.0, ban_words=0, flags=64) == -1 and b"null" in err()          # the null check answers first
    assert sel(code=7) == -1 and b"logits_dtype=7" in err()
    assert sel(code=7, seen=None) == -1 and b"logits_dtype=7" in err()                               # ... without a penalty too
    for kw in (dict(words=3), dict(ban_words=3), dict(ban_words=3, seen=None), dict(col=8), dict(col=-1), dict(Vv=0), dict(Vv=1 << 23, words=1 << 18,
               ban_words=1 << 18), dict(Vv=1 << 23, seen=None, ban_words=1 << 18), dict(B=-1), dict(step=-1), dict(n_eos=-1, eos=a)):
        assert sel(**kw) == -2 and short + b": " in err(), kw
    assert sel(ban_words=3, penalty=0.0, flags=64) == -2                                             # shape before values
    for p in (0.0, -1.3, float("inf"), float("nan")):
        assert sel(penalty=p) == -1 and b"penalty" in err(), p
    for f in ("ngram", "n_bad", "n_bad_tokens", "n_min", "n_forced", "n_suppress", "n_begin"):
        r = _lib.BanRules(**{f: -1})
        assert sel(rules=r) == -1 and short + b": rules: ngram=" in err() and b"non-negative" in err(), f
    for kw in (dict(n_bad=1), dict(n_bad=1, bad_offsets=a, n_bad_tokens=2), dict(n_min=1), dict(n_forced=2), dict(n_suppress=1), dict(n_begin=1)):
        assert sel(rules=_lib.BanRules(**kw)) == -1 and b"null list" in err(), kw
    assert sel(flags=8) == -1 and b"flags=0x8" in err()
    if entry == "sample":
        for kw in (dict(temperature=0.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_keep=0)):
            assert sel(**kw) == -1 and b"temperature=" in err(), kw
    # B == 0 is a no-op, with and without a penalty, whatever the rules say
    assert sel(B=0) == 0 and sel(B=0, seen=None, words=0, penalty=0.0) == 0 and sel(B=0, rules=_lib.BanRules()) == 0
    with pytest.raises(ValueError, match=f"uvx_{entry}_select_banned"):
        _lib.check(sel(flags=8), f"uvx_{entry}_select_banned")


class BannedFakeLib(PenalizedFakeLib):
    """PenalizedFakeLib plus a torch / numpy version of uvx_greedy_select_banned (include/uvx.h) that records its calls: the scores behind the penalty
    (if a bitmap is given) and the bans of ban_util, then uvx_greedy_select's bookkeeping."""

    def uvx_greedy_select_banned(self, st, code, logits, B, Vv, penalty, seen, words, scores_out, rules, flags, ban, ban_words, *book):
        col, seq = int(book[7].value), book[5]
        self.calls.append(("banned", penalty if seen is not None else None, col, flags))
        assert scores_out is None and tuple(ban.shape) == (B, ban_words) and ban_words == (Vv + 31) // 32 and ban.dtype == torch.int32
        lst = lambda v: [] if v is None else v.tolist()
        offs, toks = lst(rules.bad_offsets), lst(rules.bad_tokens)
        assert (rules.n_bad, rules.n_bad_tokens) == (max(len(offs) - 1, 0), len(toks))
        bad = [toks[offs[i]:offs[i + 1]] for i in range(rules.n_bad)]
        s = logits.float().clone()
        for b in range(B):
            row = s[b].numpy() if seen is None else PU.penalized(s[b].numpy(), PU.ids_of(self._bits(seen)[b]), penalty)
            mask = BU.banned_by_flags(seq[b, :col].tolist(), Vv, rules.ngram, bad, lst(rules.min_ids), lst(rules.forced_ids), lst(rules.suppress_ids),
                                      lst(rules.begin_ids), flags)
            s[b] = torch.from_numpy(BU.apply(row, mask, bool(flags & BU.BAN_FORCED)))
            self._bits(ban)[b] = PU.bitmap([np.flatnonzero(mask)], Vv, ban_words)[0]
        rc = self.uvx_greedy_select(st, code, s, B, Vv, *book)
        if seen is not None:
            bits = self._bits(seen)
            for b, t in enumerate(book[4].tolist()):
                if 0 <= t < Vv:
                    bits[b, t >> 5] |= np.uint32(1 << (t & 31))
        return rc


@pytest.fixture()
def model(monkeypatch):
    fake = BannedFakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "BanRules", types.SimpleNamespace)          # (the double takes the lists as tensors: ptr is the identity here)
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


DEVICE_CALLS = ("mark", "select", "banned")


def both(model, *a, **kw):
    """generate() with the switch off, then on -> (host result, device result, the double's calls of the device run)."""
    assert UltravoxModel.banned_select is False and model.banned_select is False       # an object that never ran __init__ keeps the host loop
    host = model.generate(*a, **kw)
    assert not [c for c in model.fake.calls if c[0] in DEVICE_CALLS]
    model.fake.calls.clear()
    model.banned_select = True
    try:
        dev = model.generate(*a, **kw)
    finally:
        model.banned_select = False
    calls = list(model.fake.calls)
    model.fake.calls.clear()
    return host, dev, calls


def rules_kw(dev_free, N, T=9):
    """Rules that all decide something on the double's logits: the free run's own tokens are banned or suppressed."""
    free = dev_free[0, T:].tolist()
    return dict(no_repeat_ngram_size=2, bad_words_ids=[[free[0]], [free[1], free[2]], [2]], min_new_tokens=3, forced_eos_token_id=[7, 96],
                suppress_tokens=[free[1], 11], begin_suppress_tokens=[free[0], int(dev_free[1, T])], min_length=T + 2)


@pytest.mark.parametrize("p", [None, 50.0])
def test_generate_banned_device_loop_equals_the_host_loop(model, p):
    ids, am = left_padded(2, 9, [0, 3])
    N = 7
    pen = {} if p is None else dict(repetition_penalty=p)
    free = model.generate(ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1, **pen)
    model.fake.calls.clear()
    kw = dict(attention_mask=am, max_new_tokens=N, eos_token_id=[5, -1], **pen, **rules_kw(free, N))
    host, dev, calls = both(model, ids, **kw)
    assert torch.equal(host, dev) and dev.shape == (2, 9 + N) and not torch.equal(dev, free)
    assert set(dev[:, -1].tolist()) <= {7, 96, 5}                                                        # the forced step (5: the pad of a finished row)
    # exactly one banned select per token at consecutive columns, no uvx_argmax, no other select; one mark over the prompt iff there is a penalty
    ban = [c for c in calls if c[0] == "banned"]
    assert [c[2] for c in ban] == list(range(9, 9 + N)) and all(c[1] == p for c in ban)
    assert [c[3] for c in ban] == [BU.BAN_MIN | BU.BAN_BEGIN, BU.BAN_MIN, BU.BAN_MIN, 0, 0, 0, BU.BAN_FORCED]
    assert [c for c in calls if c[0] == "mark"] == ([] if p is None else [("mark", 9, (2, 9))])
    assert not [c for c in calls if c[0] in ("argmax", "select")] and len([c for c in calls if c[0] == "decode"]) == N - 1
    # an early EOS with pad_token_id, and a streamer
    stop = int(dev[0, 9 + 3])
    first = dev[0, 9:].tolist().index(stop)
    ra, rb = Rec(), Rec()
    kw2 = dict(kw, eos_token_id=[stop, 96], pad_token_id=1)
    host_s = model.generate(ids, streamer=ra, **kw2)
    model.fake.calls.clear()
    model.banned_select = True
    dev_s = model.generate(ids, streamer=rb, **kw2)
    model.banned_select = False
    assert torch.equal(host_s, dev_s)
    assert 1 in dev_s[0, 9 + first + 1:].tolist() or dev_s.shape[1] == 9 + first + 1                    # the finished row is padded while the other runs
    assert ra.ended and rb.ended and len(ra.puts) == len(rb.puts) == dev_s.shape[1] - 9 + 1
    assert all(torch.equal(x, y) for x, y in zip(ra.puts, rb.puts)) and torch.equal(rb.puts[0], ids)
    assert len([c for c in model.fake.calls if c[0] == "banned"]) == dev_s.shape[1] - 9


@pytest.mark.parametrize("p", [None, 50.0])
def test_generate_banned_second_turn_over_past_key_values(model, p):
    """A second turn that reuses the cache: the chunk prefill sees only the new tokens, the n-gram and bad-word rules read the WHOLE input_ids."""
    pen = {} if p is None else dict(repetition_penalty=p)
    ids1, am1 = left_padded(2, 9, [0, 3])
    rules = dict(no_repeat_ngram_size=1, suppress_tokens=[11])            # n = 1: every id of the row, the reused prefix included, is banned
    h1, d1, _ = both(model, ids1, attention_mask=am1, max_new_tokens=5, eos_token_id=-1, return_dict_in_generate=True, **pen, **rules)
    assert torch.equal(h1.sequences, d1.sequences)
    sh, sd = h1.past_key_values, d1.past_key_values
    assert isinstance(sd, KVState) and (sd.cur_len, sd.Tmax) == (sh.cur_len, sh.Tmax) == (13, 14)
    assert torch.equal(sd.pos_next, sh.pos_next) and torch.equal(sd.kv_start, sh.kv_start) and torch.equal(sd.tokens, sh.tokens)
    ids2 = torch.cat([d1.sequences, torch.randint(3, V, (2, 6), generator=torch.Generator().manual_seed(1))], 1)
    am2 = torch.cat([am1, torch.ones(2, ids2.shape[1] - 9, dtype=torch.long)], 1)
    T2 = ids2.shape[1]
    fresh = model.generate(ids2, attention_mask=am2, max_new_tokens=4, eos_token_id=-1, **pen, **rules)
    model.fake.calls.clear()
    h2, d2, calls = both(model, ids2, attention_mask=am2, max_new_tokens=4, eos_token_id=-1, past_key_values=sd, return_dict_in_generate=True, **pen, **rules)
    assert model.last_prefill_reused == 13 and calls[0] == ("chunk", 13, T2 - 13)
    assert [c[2] for c in calls if c[0] == "banned"] == list(range(T2, T2 + 4))
    assert torch.equal(d2.sequences, h2.sequences) and torch.equal(d2.sequences, fresh)
    assert d2.past_key_values.cur_len == h2.past_key_values.cur_len == T2 + 3
    for b in range(2):                                                    # no id of the row is produced again
        assert not set(d2.sequences[b, T2:].tolist()) & set(ids2[b].tolist()) and len(set(d2.sequences[b, T2:].tolist())) == 4


@pytest.mark.parametrize("kw", [dict(stopping_criteria=[lambda i, s: False]), dict(output_logits=True, return_dict_in_generate=True), dict(num_beams=2),
                                dict(logits_processor=[lambda i, s: s]), dict(do_sample=True, top_k=5), dict(suppress_tokens=[V])])
def test_other_configurations_keep_the_host_loop(model, kw):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    model.banned_select = True
    base = dict(attention_mask=am, max_new_tokens=3, eos_token_id=-1, no_repeat_ngram_size=2)
    if "suppress_tokens" in kw:                                           # an id outside the vocabulary: torch's indexing raises, as before
        with pytest.raises(IndexError):
            model.generate(ids, **base, **kw)
    else:
        model.generate(ids, **base, **kw)
        model.generate(ids, repetition_penalty=1.3, **base, **kw)
    assert not [c for c in model.fake.calls if c[0] in DEVICE_CALLS]


def test_the_switches_turn_the_banned_loop_off(model, monkeypatch):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    kw = dict(attention_mask=am, max_new_tokens=4, eos_token_id=-1, no_repeat_ngram_size=1, repetition_penalty=50.0)
    model.banned_select = True
    want = model.generate(ids, **kw)
    assert [c[0] for c in model.fake.calls].count("banned") == 4
    model.fake.calls.clear()
    monkeypatch.setenv("UVX_GREEDY_SELECT", "0")
    got = model.generate(ids, **kw)
    assert torch.equal(got, want) and not [c for c in model.fake.calls if c[0] in DEVICE_CALLS]
    monkeypatch.delenv("UVX_GREEDY_SELECT")
    model.banned_select = False
    model.penalized_select = True                                          # the penalised selector is not a stand-in for the banned one
    assert torch.equal(model.generate(ids, **kw), want) and not [c for c in model.fake.calls if c[0] in DEVICE_CALLS]
    model.penalized_select = False


def test_philox_generator_flags(model):
    """Without processors_on_device the ban processors are refused as before (also with penalty_on_device alone); with it, what the kernel does not
    do is refused by name."""
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    kw = dict(attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True)
    assert PhiloxGenerator(1).processors_on_device is False and PhiloxGenerator(1, penalty_on_device=True).processors_on_device is False
    g = PhiloxGenerator(1, processors_on_device=True)
    assert g.processors_on_device and g.penalty_on_device
    for gen in (PhiloxGenerator(1), PhiloxGenerator(1, penalty_on_device=True)):
        for rules in (dict(no_repeat_ngram_size=2), dict(suppress_tokens=[4], repetition_penalty=1.2), dict(min_new_tokens=2)):
            with pytest.raises(ValueError, match="PhiloxGenerator.*score processors"):
                model.generate(ids, generator=gen, **kw, **rules)
        assert gen.offset == 0
    for clash, name in ((dict(logits_processor=[lambda i, s: s]), "logits_processor"), (dict(stopping_criteria=[lambda i, s: False]), "stopping_criteria"),
                        (dict(output_logits=True, return_dict_in_generate=True), "output_logits"), (dict(num_beams=2), "num_beams > 1"),
                        (dict(suppress_tokens=[V + 1]), "outside the vocabulary")):
        with pytest.raises(ValueError, match=f"PhiloxGenerator.*{name}"):
            model.generate(ids, generator=g, no_repeat_ngram_size=2, **kw, **clash)
    assert g.offset == 0


def test_the_banned_kernels_have_no_scratch_segment():
    """hipcc's kernel-resource-usage remarks for select_banned.hip with the package's own flags: the eight instantiations of the banned select kernel
    (dtype x reader x chooser), no scratch."""
    import re
    import subprocess

    from ultravox_amd import build as B
    src = B.CSRC / "select_banned.hip"
    cmd = [B._hipcc(), *B.FLAGS, *B.EXTRA_FLAGS.get(src.name, []), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src), "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    assert len(names) == len(scratch) == 8 and len(set(names)) == 8 and all("banned_select_k" in n for n in names), names
    assert sum("SampleArgs" in n for n in names) == 4 and sum("ArgmaxArgs" in n for n in names) == 4
    assert scratch == [0] * 8, list(zip(names, scratch))
