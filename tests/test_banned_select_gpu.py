"""uvx_greedy_select_banned / uvx_sample_select_banned (include/uvx.h; csrc/select_banned.hip, csrc/ban.h) on the device - f32 and bf16 logits
throughout - then through generate().

Greedy: no tolerance.  The reference of a row is penalized_util.penalized (where a penalty is given) behind ban_util.banned / apply, which
tests/test_banned_select_cpu.py pins against transformers' own processor list bit for bit: scores_out equals it in every bit, the token is its first
maximum, the ban buffer equals its banned set on bits < V, `seen` afterwards is `seen` before OR the bit of the token written.
Sampling: that row -> sample_util.x_of -> RowRef.warp, and tests/test_sample_gpu.py's acceptance unchanged (check_probs, token_ok, its grid), with
sample_util.margins_ok asserted on the reference first - a precondition on the inputs, not a tolerance."""
import numpy as np
import pytest
import torch

import ban_util as BU
import penalized_util as PU
import sample_util as SU
from test_sample_gpu import check_probs, grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
GREEDY_VS = [1, 7, 33, 1024, 1032, 1025, 4099, 131077]      # 7: scalar walk only; 33: a second word with one live bit; 1032: last word partly used;
                                                            # 1025: rows unaligned; 131077: the clear loop wraps (4097 words for 1024 threads)
SAMPLE_VS = [1, 5, 33, 1023, 1024, 1025, 4099]


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def device_rules(r: BU.Rules):
    from ultravox_amd import ops
    return ops.ban_rules(DEV, ngram=r.ngram, bad_words=r.kept_bad_words(), min_ids=r.min_ids(), forced_ids=list(r.forced), suppress_ids=list(r.suppress),
                         begin_ids=list(r.begin))


def sequences_of(rows, B, fill):
    """int64 [B, L + 5] on the device: the rows, then five columns the kernel must not read (an id the rules would act on)."""
    L = rows.shape[1]
    seq = torch.full((B, L + 5), int(fill), dtype=torch.int64)
    seq[:, :L] = torch.from_numpy(rows[:B])
    return seq.to(DEV)


def greedy_case(dev, rows_f32, c: BU.Case, B, penalty, ban=None):
    """One launch of the greedy entry point on case c, checked in full -> the ban buffer."""
    from ultravox_amd import ops
    V, L = rows_f32.shape[1], c.L
    seq = sequences_of(c.rows, B, fill=V // 2)
    flags = c.rules.flags(L, c.prompt_len, c.max_len)
    seen = before = None
    if penalty is not None:
        seen = ops.seen_mark(seq[:, :L], V)
        before = bits(seen).copy()
        assert np.array_equal(before, PU.bitmap(c.rows[:B], V))
    out = ops.greedy_select_banned(dev[:B], device_rules(c.rules), flags, seen=seen, penalty=1.0 if penalty is None else penalty, ban=ban, want_scores=True,
                                   sequences=seq, col=L)
    scores, toks, got_ban = out["scores"].cpu().numpy(), out["tokens"].cpu().tolist(), bits(out["ban"])
    what = (c.name, B, penalty)
    for b in range(B):
        mask, forced = BU.banned(c.rows[b], c.rules, L, c.prompt_len, c.max_len)
        want = BU.apply(rows_f32[b] if penalty is None else PU.penalized(rows_f32[b], c.rows[b], penalty), mask, forced)
        assert PU.same_bits(scores[b], want), (what, b, np.flatnonzero(scores[b].view(np.uint32) != want.view(np.uint32))[:8])
        assert toks[b] == PU.argmax(want), (what, b, toks[b])
        assert np.array_equal(BU.mask_of(got_ban[b], V), mask), (what, b, np.flatnonzero(BU.mask_of(got_ban[b], V) != mask)[:8])
    assert out["sequences"][:, L].cpu().tolist() == toks and torch.equal(out["sequences"][:, :L].cpu(), torch.from_numpy(c.rows[:B]))
    if penalty is not None:
        assert np.array_equal(bits(seen), before | PU.bitmap([[t] for t in toks], V, before.shape[1])), what
    return out["ban"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", GREEDY_VS)
def test_greedy_rule_edges_exactly(V, dtype):
    """Every rule edge of ban_util.edge_cases (n-gram n = 1, 2, 3 at L = n - 2, n - 1, n, matches at j = 0 and at the last window, ids outside the
    vocabulary as the banned id and inside a matching prefix; one- and multi-token bad words, too long ones, two banning one id, a last token outside;
    the min-length and begin flags on and off; forced steps with one and two ids, a forced id that is also suppressed, all of them suppressed),
    B = 1 and 3, the sequences' stride larger than col, alone and behind a penalty."""
    g = torch.Generator().manual_seed(V)
    dev = (4 * torch.randn(3, V, generator=g)).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    cases = BU.edge_cases(V)
    for c in cases:
        for B in (1, 3):
            greedy_case(dev, rows, c, B, None)
        greedy_case(dev, rows, c, 3, 1.3)
    c = next(c for c in cases if c.name == "forced: every forced id suppressed")
    assert BU.banned(c.rows[0], c.rules, c.L, c.prompt_len, c.max_len)[0].all()      # (its token, checked above as the first maximum of all -inf, is 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [4099, 131077])
def test_greedy_long_row_and_long_lists(V, dtype):
    """The mark loops wrap: a row of 3000 ids over 40 distinct ones (hundreds of matching windows per thread stride), 2500 suppressed ids, 1500 bad
    words (one- and two-token ones), 1100 begin ids - more than the block's 1024 threads each."""
    g = np.random.default_rng(V + 1)
    L = 3000
    rows = g.integers(V - 40, V, size=(3, L)).astype(np.int64)
    last = [int(t) for t in rows[:, -1]]
    bad = [[int(t)] for t in g.integers(0, V, size=700)] + [[last[i % 3], int(t)] for i, t in enumerate(g.integers(0, V, size=800))]
    rules = BU.Rules(V, ngram=2, bad_words=bad, suppress=[int(t) for t in g.integers(0, V, size=2500)], begin=[int(t) for t in g.integers(0, V, size=1100)],
                     eos=[5 % V], min_new=3)
    dev = (4 * torch.randn(3, V, generator=torch.Generator().manual_seed(V))).to(DEV).to(dtype)
    rows_f32 = dev.float().cpu().numpy()
    for n in (2, 3):
        rules.ngram = n
        c = BU.Case(f"long n={n}", rows, rules, prompt_len=L, max_len=10 ** 6)
        assert sum(BU.banned(rows[b], rules, L, L, 10 ** 6)[0].sum() for b in range(3)) > 3 * 2000
        greedy_case(dev, rows_f32, c, 3, None)
        greedy_case(dev, rows_f32, c, 3, 1.1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_consecutive_launches_leave_no_stale_bits(dtype):
    """One ban buffer (full of ones to begin with) over a generate()-like run whose rule set shrinks: begin_suppress_tokens after the first step,
    min_new_tokens expiring after the third, the forced step at the end.  After every launch the buffer is that step's set exactly, and the
    kernel's own tokens are the ones the next step's n-gram rule reads."""
    from ultravox_amd import ops
    V, B, T, N = 1032, 3, 6, 7
    g = np.random.default_rng(2)
    rules = BU.Rules(V, ngram=1, eos=[1000, 1001], min_new=3, forced=[1001], suppress=[3, 4], begin=list(range(40, 140)))
    dev_rules = device_rules(rules)
    seq = torch.zeros(B, T + N + 2, dtype=torch.int64)
    seq[:, :T] = torch.from_numpy(g.integers(0, V, size=(B, T)))
    seq = seq.to(DEV)
    ban = torch.full((B, PU.words_of(V)), -1, dtype=torch.int32, device=DEV)
    live = torch.ones(B, dtype=torch.int32, device=DEV)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    eos = torch.tensor([1000, 1001], device=DEV)
    sizes = []
    for step in range(N):
        logits = (4 * torch.randn(B, V, generator=torch.Generator().manual_seed(step))).to(DEV).to(dtype)
        L = T + step
        before = seq.cpu().numpy()
        out = ops.greedy_select_banned(logits, dev_rules, rules.flags(L, T, T + N), ban=ban, want_scores=True, eos_ids=eos, unfinished=live, sequences=seq,
                                       col=L, step=step, counter=counter)
        assert out["ban"] is ban
        for b in range(B):
            mask, forced = BU.banned(before[b], rules, L, T, T + N)
            assert np.array_equal(BU.mask_of(bits(ban)[b], V), mask), (step, b)
            want = BU.apply(logits[b].float().cpu().numpy(), mask, forced)
            assert PU.same_bits(out["scores"][b].cpu().numpy(), want) and int(seq[b, L]) == PU.argmax(want), (step, b)
        sizes.append(int(BU.banned(before[0], rules, L, T, T + N)[0].sum()))
    assert sizes[0] > sizes[1] + 90 and sizes[2] == sizes[3] + 1 and sizes[-1] == V - 1, sizes        # begin drops out, then the EOS ids; the forced step
    assert seq[:, T + N - 1].cpu().tolist() == [1001] * B and int(counter[(N - 1) & 1]) == 0          # forced EOS: every row has finished


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1025, 4099])
def test_no_rules_is_no_change(V, dtype):
    """No rule, no flag: tokens, scores_out and probs_out bit-identical to the plain entry points without a penalty, to the _penalized ones with."""
    from ultravox_amd import ops
    from test_sample_penalized_gpu import mark, seen_ids_for
    dev = torch.from_numpy(SU.peaked_rows(V, 3, 0)).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    ids = seen_ids_for(rows, 0)
    none = ops.ban_rules(DEV)
    u_dev = torch.from_numpy(np.random.default_rng(V + 7).random(3).astype(np.float32)).to(DEV)
    seq = torch.randint(0, V, (3, 20), generator=torch.Generator().manual_seed(1)).to(DEV)
    book = lambda: dict(sequences=seq.clone(), col=15)
    got = ops.greedy_select_banned(dev, none, want_scores=True, **book())
    assert torch.equal(got["tokens"], ops.greedy_select(dev, **book())["tokens"]) and PU.same_bits(got["scores"].cpu().numpy(), rows)
    assert not BU.mask_of(bits(got["ban"])[0], V).any()
    a, b = mark(ids, V), mark(ids, V)
    got, want = ops.greedy_select_banned(dev, none, seen=a, penalty=1.3, want_scores=True, **book()), ops.greedy_select_penalized(dev, b, 1.3, want_scores=True, **book())
    assert torch.equal(got["tokens"], want["tokens"]) and PU.same_bits(got["scores"].cpu().numpy(), want["scores"].cpu().numpy()) and torch.equal(a, b)
    for t, k, p in ((0.7, 5, 0.9), (1.0, 0, 1.0)):
        kw = dict(temperature=t, top_k=k, top_p=p, uniforms=u_dev, want_probs=True)
        got, want = ops.sample_select_banned(dev, none, **kw, **book()), ops.sample_select(dev, **kw, **book())
        assert torch.equal(got["tokens"], want["tokens"]) and torch.equal(got["probs"].view(torch.int32), want["probs"].view(torch.int32))
        a, b = mark(ids, V), mark(ids, V)
        got, want = ops.sample_select_banned(dev, none, seen=a, penalty=1.3, **kw, **book()), ops.sample_select_penalized(dev, b, 1.3, **kw, **book())
        assert torch.equal(got["tokens"], want["tokens"]) and torch.equal(got["probs"].view(torch.int32), want["probs"].view(torch.int32)) and torch.equal(a, b)


# ---- sampling ----
# Inputs of the grid test: sample_util.peaked_rows(V, 3, seed) as f32 and after a bf16 round trip; row b's ban set = its head tokens ranked 3rd, 6th,
# 9th and 12th by value plus 200 random ids of default_rng(b) capped at V - 2 (so the last id is never banned by chance).  Seeds for which every
# boundary of the reference clears twice the bound over the whole grid were found on the CPU for exactly this rule (and for the penalty 1.3 over
# test_sample_penalized_gpu.seen_ids_for on top); the test asserts the margins again.
SAMPLE_SEEDS = {(V, dt, pen): 0 for V in SAMPLE_VS for dt in DTYPES for pen in (None, 1.3)}


def ban_ids_for(rows, b):
    V = rows.shape[1]
    head = np.argsort(rows[b])[::-1][:min(12, V)][2::3]
    return np.concatenate([head, np.minimum(np.random.default_rng(b).integers(0, V, size=200), V - 2)]).astype(np.int64)


def per_row_rules(ban_ids, V):
    """Rules that ban ban_ids[b] in row b only: two-token bad words whose first token is row b's last id, an id of its own outside the vocabulary
    (ids are compared by value) -> (Rules, the rows [B, 4])."""
    tails = [10 ** 9 + b for b in range(len(ban_ids))]
    rows = np.array([[0, 0, 0, t] for t in tails], dtype=np.int64)
    return BU.Rules(V, bad_words=[[tails[b], int(t)] for b, ids in enumerate(ban_ids) for t in ids]), rows


@pytest.mark.parametrize("penalty", [None, 1.3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", SAMPLE_VS)
def test_sampling_kept_set_probabilities_and_token_over_the_grid(V, dtype, penalty):
    from ultravox_amd import ops
    from test_sample_penalized_gpu import mark, seen_ids_for
    seed = SAMPLE_SEEDS[(V, dtype, penalty)]
    dev = torch.from_numpy(SU.peaked_rows(V, 3, seed)).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    ban_ids = [ban_ids_for(rows, b) for b in range(3)]
    rules, tails = per_row_rules(ban_ids, V)
    dev_rules = device_rules(rules)
    seq = sequences_of(tails, 3, fill=0)
    seen_ids = seen_ids_for(rows, seed)
    base = mark(seen_ids, V) if penalty is not None else None
    masks = [BU.banned(tails[b], rules, 4, 0, 10 ** 6)[0] for b in range(3)]
    for b in range(3):
        assert np.array_equal(np.flatnonzero(masks[b]), PU.in_range(ban_ids[b], V))

    def ref_of(b, t):
        s = BU.apply(rows[b], masks[b], False)
        if penalty is not None:
            s = PU.penalized(s, seen_ids[b], penalty)
        return SU.RowRef(SU.x_of(s, t))
    refs = {(b, t): ref_of(b, t) for b in range(3) for t in (1.0, 0.7)}
    us = np.random.default_rng(V).random(3).astype(np.float32)
    u_dev = torch.from_numpy(us).to(DEV)
    warped = {}
    for B in (1, 3):
        for t, k, p, mp, keep in grid(V):
            seen = None if base is None else base[:B].clone()
            out = ops.sample_select_banned(dev[:B], dev_rules, seen=seen, penalty=penalty or 1.0, temperature=t, top_k=k, top_p=p, min_p=mp, min_keep=keep,
                                           uniforms=u_dev, want_probs=True, sequences=seq[:B].clone(), col=4)
            probs, toks = out["probs"].cpu().numpy(), out["tokens"].cpu().tolist()
            for b in range(B):
                key = (b, t, k, p, mp, keep)
                if key not in warped:
                    warped[key] = refs[(b, t)].warp(k, p, mp, keep)
                    assert SU.margins_ok(warped[key]), ("precondition: the reference's boundary margins", key, warped[key]["margins"])
                check_probs(probs[b], warped[key], (B,) + key)
                assert SU.token_ok(toks[b], float(us[b]), warped[key]), ((B,) + key, toks[b], float(us[b]))
                assert not masks[b][toks[b]] or not warped[key]["kept"].any()
            if seen is not None:
                assert np.array_equal(bits(seen), bits(base[:B]) | PU.bitmap([[t_] for t_ in toks], V, base.shape[1]))
    for b in range(3):
        assert np.array_equal(BU.mask_of(bits(out["ban"])[b], V), masks[b])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sampling_with_top_k_1_is_the_greedy_banned_select(dtype):
    """Distinct values, top_k = 1: the sampled token is the greedy one under the same rules, for every rule edge.  (A forced step with two forced ids
    left gives two equal zeros, which top_k = 1 keeps both: those cases are left to the grid test.)"""
    from ultravox_amd import ops
    V = 256                                                               # (a permutation of 0 .. 255: distinct in bf16 too)
    dev = torch.from_numpy(np.random.default_rng(4).permutation(V).astype(np.float32)).to(DEV).to(dtype)[None].repeat(3, 1).contiguous()
    assert len(set(dev[0].float().cpu().tolist())) == V
    u = torch.full((3,), 0.5, device=DEV)
    for c in BU.edge_cases(V):
        fl = c.rules.flags(c.L, c.prompt_len, c.max_len)
        if fl & BU.BAN_FORCED and len([t for t in c.rules.forced if 0 <= t < V]) > 1:
            continue
        seq = sequences_of(c.rows, 3, fill=V // 2)
        r = device_rules(c.rules)
        a = ops.greedy_select_banned(dev, r, fl, sequences=seq.clone(), col=c.L)["tokens"]
        b = ops.sample_select_banned(dev, r, fl, top_k=1, uniforms=u, sequences=seq.clone(), col=c.L)["tokens"]
        assert torch.equal(a, b), c.name


# ---- through generate() ----
def _model(dtype=torch.float32, seed=3):
    from test_penalized_select_gpu import _small
    return _small(dtype, seed)


def host_loop(model, **kw):
    model.banned_select = False
    try:
        return model.generate(**kw)
    finally:
        model.banned_select = True


V_SMALL, EOS = 512, [510, 511]
# (model seed, input seed): as in tests/test_penalized_select_gpu.py (its note at F32_SEEDS), torch's penalty on the GPU may be an ulp off HF's rule, so
# "the host loop's tokens equal the replay" is a precondition on the inputs; these are seeds for which it held on an MI355X, asserted again below
GEN_SEEDS = (3, 16)


def gen_rules(free, T):
    """All seven rules, built from the tokens of the run under the penalty alone so that each decides something."""
    f = free[:, T:].cpu().tolist()
    return dict(no_repeat_ngram_size=2, bad_words_ids=[[f[0][0]], [f[1][1], f[1][2]], [f[0][1], f[0][2]]], min_length=T + 3, min_new_tokens=2,
                forced_eos_token_id=511, suppress_tokens=[f[0][1], f[1][3]] + list(range(100, 120)), begin_suppress_tokens=[f[1][0], 7])


def rules_of(kw, eos):
    return BU.Rules(V_SMALL, ngram=kw["no_repeat_ngram_size"], bad_words=kw["bad_words_ids"], eos=eos, min_length=kw["min_length"], min_new=kw["min_new_tokens"],
                    forced=[kw["forced_eos_token_id"]], suppress=kw["suppress_tokens"], begin=kw["begin_suppress_tokens"])


def replay(logits, seqs, T, max_len, rules, eos, pad, penalty):
    """HF's processor list (the numpy reference) on the raw logits of every step over the sequences as they grew -> the tokens [B, steps]."""
    B, n = seqs.shape[0], len(logits)
    out = np.zeros((B, n), dtype=np.int64)
    live = [True] * B
    for step in range(n):
        raw = logits[step].float().cpu().numpy()
        for b in range(B):
            mask, forced = BU.banned(seqs[b], rules, T + step, T, max_len)
            tok = PU.argmax(BU.apply(PU.penalized(raw[b], seqs[b, :T + step], penalty), mask, forced))
            out[b, step] = tok if live[b] else pad
            live[b] = live[b] and out[b, step] not in eos
    return out


def run_greedy(model, T, N, rules_kw, eos, pad, penalty, **kw):
    """Device path, host loop (reporting its raw logits) and the replay on them -> (device output, host output)."""
    rules = rules_of(rules_kw, eos)
    args = dict(max_new_tokens=N, eos_token_id=eos, pad_token_id=pad, repetition_penalty=penalty, return_dict_in_generate=True, **rules_kw, **kw)
    dev = model.generate(**args)
    host = host_loop(model, output_logits=True, **args)
    hs = host.sequences.cpu().numpy()
    n = hs.shape[1] - T
    want = replay(host.logits, hs, T, T + N, rules, eos, pad, penalty)
    assert np.array_equal(hs[:, T:], want[:, :n]), ("precondition: the host loop follows HF's rules on these inputs", hs[:, T:], want)
    assert dev.sequences.shape == host.sequences.shape and np.array_equal(dev.sequences.cpu().numpy()[:, T:], want[:, :n]), (dev.sequences[:, T:], want)
    return dev, host


def test_f32_generate_under_all_seven_rules_equals_the_replay_of_hf_rules():
    """B = 2 with left padding, every rule plus a penalty: the device path's tokens equal HF's list replayed on the raw logits of every step, and so do
    the host loop's; the KV state equals the host loop's field by field; an early EOS pads the finished row; a second turn runs over past_key_values."""
    from test_penalized_select_gpu import T_PROMPT, _padded, same_state
    model = _model(torch.float32, GEN_SEEDS[0])
    assert model.banned_select is True
    ids, am = _padded(GEN_SEEDS[1], T=T_PROMPT)
    T, N, p = ids.shape[1], 8, 1.3
    free = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1, repetition_penalty=p)
    kw = gen_rules(free, T)
    dev, host = run_greedy(model, T, N, kw, EOS, 1, p, input_ids=ids, attention_mask=am)
    assert dev.sequences.shape == (2, T + N) and dev.sequences[:, -1].tolist() == [511, 511]          # the forced step
    assert not torch.equal(dev.sequences, free) and torch.equal(dev.sequences[:, :T], ids)
    same_state(dev.past_key_values, host.past_key_values, model._c.llm_layers, 2)
    # an early EOS: the token row 0 produced at step 4 (the min-length rules have expired there) becomes a terminator
    stop = int(dev.sequences[0, T + 4])
    e_dev, e_host = run_greedy(model, T, N, kw, [stop, 511], 1, p, input_ids=ids, attention_mask=am)
    row0 = e_dev.sequences[0, T:].tolist()
    assert stop in row0 and all(v == 1 for v in row0[row0.index(stop) + 1:]) and len(row0) > row0.index(stop) + 1
    same_state(e_dev.past_key_values, e_host.past_key_values, model._c.llm_layers, 2)
    # a second turn: the first turn's sequences plus new text, over the first turn's cache
    more = torch.randint(3, 500, (2, 5), generator=torch.Generator().manual_seed(4)).to(DEV)
    ids2 = torch.cat([dev.sequences, more], 1)
    am2 = torch.cat([am, torch.ones(2, ids2.shape[1] - T, dtype=torch.long, device=DEV)], 1)
    kw2 = dict(kw, min_length=ids2.shape[1] + 3)
    t_dev, t_host = run_greedy(model, ids2.shape[1], 6, kw2, EOS, 1, p, input_ids=ids2, attention_mask=am2, past_key_values=dev.past_key_values)
    assert model.last_prefill_reused == dev.past_key_values.cur_len > 0
    same_state(t_dev.past_key_values, t_host.past_key_values, model._c.llm_layers, 2)


def test_generate_sampling_with_processors_on_device():
    """PhiloxGenerator(seed, processors_on_device=True): the call replays for equal (seed, offset) and advances the offset by the steps run; no emitted
    token violates the rule set replayed over the output; top_k = 1 is the greedy device path; without the flag the call raises."""
    from test_penalized_select_gpu import T_PROMPT, _padded
    from ultravox_amd.generation import PhiloxGenerator
    model = _model(torch.float32, GEN_SEEDS[0])
    ids, am = _padded(GEN_SEEDS[1], T=T_PROMPT)
    T, N, p = ids.shape[1], 8, 1.3
    free = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1, repetition_penalty=p)
    kw = gen_rules(free, T)
    args = dict(input_ids=ids, attention_mask=am, max_new_tokens=N, eos_token_id=EOS, pad_token_id=1, repetition_penalty=p, do_sample=True, **kw)
    gen = PhiloxGenerator(11, processors_on_device=True)
    a = model.generate(generator=gen, temperature=1.5, top_k=50, **args)
    steps = a.shape[1] - T
    assert gen.offset == steps and 1 <= steps <= N
    b = model.generate(generator=gen, temperature=1.5, top_k=50, **args)
    assert gen.offset == steps + b.shape[1] - T
    gen2 = PhiloxGenerator(11, processors_on_device=True)
    assert torch.equal(model.generate(generator=gen2, temperature=1.5, top_k=50, **args), a)
    gen2.manual_seed(11).advance(steps)
    assert torch.equal(model.generate(generator=gen2, temperature=1.5, top_k=50, **args), b)
    rules = rules_of(kw, EOS)
    for out in (a, b):
        seqs = out.cpu().numpy()
        for r in range(2):
            live = True
            for step in range(seqs.shape[1] - T):
                tok = int(seqs[r, T + step])
                if not live:
                    assert tok == 1
                    continue
                mask, _ = BU.banned(seqs[r], rules, T + step, T, T + N)
                assert not mask[tok], (r, step, tok)
                live = tok not in EOS
    assert a.shape[1] < T + N or set(a[:, -1].tolist()) <= {511, 1}                                    # the forced step (1: the pad of a finished row)
    greedy = model.generate(**dict(args, do_sample=False))
    assert torch.equal(model.generate(generator=PhiloxGenerator(5, processors_on_device=True), top_k=1, **args), greedy)
    # the rules without a penalty, and the penalty alone under the new flag (the penalised selector's case)
    no_pen = {k: v for k, v in args.items() if k != "repetition_penalty"}
    assert torch.equal(model.generate(generator=PhiloxGenerator(5, processors_on_device=True), top_k=1, **no_pen), model.generate(**dict(no_pen, do_sample=False)))
    only_pen = dict(input_ids=ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1, repetition_penalty=p, do_sample=True)
    assert torch.equal(model.generate(generator=PhiloxGenerator(5, processors_on_device=True), top_k=1, **only_pen), free)
    for g in (PhiloxGenerator(11), PhiloxGenerator(11, penalty_on_device=True)):
        with pytest.raises(ValueError, match="PhiloxGenerator.*score processors"):
            model.generate(generator=g, **args)
        assert g.offset == 0
