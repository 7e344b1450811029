"""uvx_sample_select_penalized (include/uvx.h; csrc/select.hip) on the device - f32 and bf16 logits throughout - then through generate()
and UltravoxPipeline.

The reference of a row is a composition of what the suite already trusts: penalized_util.penalized (HF's RepetitionPenaltyLogitsProcessor bit for
bit, no tolerance) -> sample_util.x_of (the temperature) -> sample_util.RowRef.warp (float64).  Acceptance is test_sample_gpu.py's, unchanged:
probs_out > 0 is EXACTLY the kept set, every probability within sample_util.bound(n_kept) relatively, sample_util.token_ok for the token drawn;
sample_util.margins_ok is asserted on the reference before the kernel is looked at - a precondition on the inputs, not a tolerance.  After every
launch the bitmap equals the one before OR the bit of the token written, exactly."""
import numpy as np
import pytest
import torch

import penalized_util as PU
import sample_util as SU
from test_sample_gpu import check_probs, grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
VS = [1, 5, 1023, 1024, 1025, 4099, 131077]
# Seeds of sample_util.peaked_rows for which every boundary of the reference clears twice the bound over the whole grid under the penalties used and the
# seen ids of seen_ids_for (found on the CPU for exactly this rule; asserted again below).  At V = 131077 the top token has to stay unpenalised: with
# it penalised the top-p 0.9 boundary falls into the flat tail, where no seed meets the margin.
SEEDS = {(V, dt): 0 for V in VS for dt in DTYPES}
SEEDS.update({(1025, torch.float32): 1, (131077, torch.float32): 2, (131077, torch.bfloat16): 2})
PHILOX_SEEDS = {torch.float32: 0, torch.bfloat16: 0}       # peaked_rows(4099, 24, .) of test_the_philox_stream, same precondition


def penalties_for(V):
    return (1.3, 0.75) if V <= 4099 else (1.3,)


def seen_ids_for(rows, seed):
    """Per row b: every second head token starting from the SECOND largest, 300 random ids, and three ids outside the vocabulary."""
    V = rows.shape[1]
    return [np.concatenate([np.argsort(rows[b])[::-1][:min(12, V)][1::2], np.random.default_rng(1000 * seed + b).choice(V, min(V, 300), replace=False),
                            [-1, V, V + 40]]).astype(np.int64) for b in range(rows.shape[0])]


def mark(ids_rows, V):
    """ops.seen_mark over the rows of ids, padded to equal length with -1 -> the device bitmap."""
    from ultravox_amd import ops
    n = max(len(r) for r in ids_rows)
    ids = np.full((len(ids_rows), n), -1, dtype=np.int64)
    for b, r in enumerate(ids_rows):
        ids[b, :len(r)] = r
    return ops.seen_mark(torch.from_numpy(ids).to(DEV), V)


def bits(seen):
    return seen.cpu().numpy().view(np.uint32)


def row_ref(row, ids, penalty, temperature):
    """RowRef of one f32 row behind the penalty and the temperature; NaN is -inf, as the kernel's canonicalisation has it."""
    x = SU.x_of(PU.penalized(row, ids, penalty), temperature)
    return SU.RowRef(np.where(np.isnan(x), np.float32(-np.inf), x).astype(np.float32))


def rows_and_ids(V, dtype, B, seed):
    dev = torch.from_numpy(SU.peaked_rows(V, B, seed)).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    return rows, dev, seen_ids_for(rows, seed)


def bitmap_after(before, toks, V):
    return before | PU.bitmap([[t] for t in toks], V, before.shape[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VS)
def test_kept_set_probabilities_token_and_bitmap_over_the_grid(V, dtype):
    from ultravox_amd import ops
    seed = SEEDS[(V, dtype)]
    rows, dev, ids = rows_and_ids(V, dtype, 3, seed)
    base = mark(ids, V)
    before = bits(base)
    assert np.array_equal(before, PU.bitmap(ids, V))
    if V == 131077:
        assert all(int(rows[b].argmax()) not in set(ids[b].tolist()) for b in range(3)), "precondition: the top token is not seen"
    us = np.random.default_rng(V).random(3).astype(np.float32)
    u_dev = torch.from_numpy(us).to(DEV)
    for pen in penalties_for(V):
        refs = {(b, t): row_ref(rows[b], ids[b], pen, t) for b in range(3) for t in (1.0, 0.7)}
        warped = {}
        for B in (1, 3):
            for t, k, p, mp, keep in grid(V):
                seen = base[:B].clone()
                out = ops.sample_select_penalized(dev[:B], seen, pen, temperature=t, top_k=k, top_p=p, min_p=mp, min_keep=keep, uniforms=u_dev,
                                                  want_probs=True)
                probs, toks = out["probs"].cpu().numpy(), out["tokens"].cpu().tolist()
                for b in range(B):
                    key = (b, t, k, p, mp, keep)
                    if key not in warped:
                        warped[key] = refs[(b, t)].warp(k, p, mp, keep)
                        assert SU.margins_ok(warped[key]), ("precondition: the reference's boundary margins", pen, key, warped[key]["margins"])
                    check_probs(probs[b], warped[key], (pen, B) + key)
                    assert SU.token_ok(toks[b], float(us[b]), warped[key]), ((pen, B) + key, toks[b], float(us[b]))
                assert np.array_equal(bits(seen), bitmap_after(before[:B], toks, V)), (pen, B, t, k, p, mp, keep)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1025, 4099])
def test_no_penalty_is_no_change(V, dtype):
    """An all-zero bitmap, and penalty 1.0 on a marked one: tokens and probs_out bit-identical to ops.sample_select on the same logits and uniforms."""
    from ultravox_amd import ops
    rows, dev, ids = rows_and_ids(V, dtype, 3, 0)
    u_dev = torch.from_numpy(np.random.default_rng(V + 7).random(3).astype(np.float32)).to(DEV)
    for t, k, p in ((0.7, 5, 0.9), (1.0, 0, 1.0)):
        kw = dict(temperature=t, top_k=k, top_p=p, uniforms=u_dev, want_probs=True)
        plain = ops.sample_select(dev, **kw)
        for what, seen, pen in (("zero bitmap", torch.zeros(3, PU.words_of(V), device=DEV, dtype=torch.int32), 1.3), ("penalty 1", mark(ids, V), 1.0)):
            got = ops.sample_select_penalized(dev, seen, pen, **kw)
            assert torch.equal(got["tokens"], plain["tokens"]), (what, t, k, p)
            assert torch.equal(got["probs"].view(torch.int32), plain["probs"].view(torch.int32)), (what, t, k, p)


@pytest.mark.parametrize("V", [1023, 4099])
def test_top_k_1_is_the_penalised_argmax(V):
    """f32 rows of distinct values at temperature 1: the token is ops.greedy_select_penalized's, and eight consecutive launches on the same logits
    with the bitmap carried over give penalized_util.greedy_loop's tokens."""
    from ultravox_amd import ops
    B, N, pen = 2, 8, 1.3
    g = np.random.default_rng(V)
    rows = (4.0 * g.standard_normal((B, V))).astype(np.float32)
    assert all(len(np.unique(r)) == V for r in rows)
    ids = [g.choice(V, 300, replace=False) for _ in range(B)]
    dev = torch.from_numpy(rows).to(DEV)
    u_dev = torch.from_numpy(g.random(B).astype(np.float32)).to(DEV)
    a = ops.sample_select_penalized(dev, mark(ids, V), pen, top_k=1, uniforms=u_dev)["tokens"]
    assert torch.equal(a, ops.greedy_select_penalized(dev, mark(ids, V), pen)["tokens"])
    seen = mark(ids, V)
    seq = torch.full((B, N), -1, device=DEV, dtype=torch.int64)
    live = torch.ones(B, device=DEV, dtype=torch.int32)
    counter = torch.zeros(2, device=DEV, dtype=torch.int32)
    for step in range(N):
        ops.sample_select_penalized(dev, seen, pen, top_k=1, seed=3, offset=step, unfinished=live, sequences=seq, col=step, step=step, counter=counter)
    want = [PU.greedy_loop(rows[b], pen, N, ids[b]) for b in range(B)]
    assert seq.cpu().tolist() == want
    assert np.array_equal(bits(seen), PU.bitmap([np.concatenate([ids[b], want[b]]) for b in range(B)], V))


SETTINGS = ((1.0, 1, 1.0, 0.0, 1), (0.7, 0, 1.0, 0.0, 1), (1.0, 5, 1.0, 0.1, 1), (0.7, 0, 0.9, 0.0, 1))


def check_rows(dev, ids, pen, what, seen=None, settings=SETTINGS):
    """Every setting on dev [B, V] with the bitmap of ids (or the given one, left as it is): kept set, probabilities, token, bitmap -> the last tokens."""
    from ultravox_amd import ops
    B, V = dev.shape
    rows = dev.float().cpu().numpy()
    base = mark(ids, V) if seen is None else seen
    before = bits(base)
    us = np.linspace(0.15, 0.85, B).astype(np.float32)
    u_dev = torch.from_numpy(us).to(DEV)
    for t, k, p, mp, keep in settings:
        seen_now = base.clone()
        out = ops.sample_select_penalized(dev, seen_now, pen, temperature=t, top_k=k, top_p=p, min_p=mp, min_keep=keep, uniforms=u_dev, want_probs=True)
        probs, toks = out["probs"].cpu().numpy(), out["tokens"].cpu().tolist()
        for b in range(B):
            ref = row_ref(rows[b], ids[b], pen, t).warp(k, p, mp, keep)
            assert SU.margins_ok(ref), ("precondition: the reference's boundary margins", what, b, t, k, p, mp, keep, ref["margins"])
            check_probs(probs[b], ref, (what, b, t, k, p, mp, keep))
            assert SU.token_ok(toks[b], float(us[b]), ref), (what, b, t, k, p, mp, keep, toks[b])
        assert np.array_equal(bits(seen_now), bitmap_after(before, toks, V)), (what, t, k, p, mp, keep)
    return toks, probs


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_rows(dtype):
    """V = 4099, penalty 2: a seen top token that falls below the second; a seen negative logit (multiplied, not divided); seen -inf and NaN entries;
    a row of nothing but -inf; the maximum in column V - 1 and seen; a bitmap of words > ceil(V / 32); rows after the first are not 16-byte aligned (V odd:
    the scalar path; test_aligned_rows_and_a_wider_bitmap is the 16-byte path next to it)."""
    from ultravox_amd import ops
    V, pen = 4099, 2.0
    rows = SU.peaked_rows(V, 5, 0)
    order = np.argsort(rows[0])[::-1]
    top, second = int(order[0]), int(order[1])
    rows[1, 7] = -3.0
    rows[2, [10, 11]] = -np.inf
    rows[2, [12, 13]] = np.nan
    rows[3] = -np.inf
    rows[4, V - 1] = 40.0
    dev = torch.from_numpy(rows).to(DEV).to(dtype)
    rows = dev.float().cpu().numpy()
    ids = [[top, -1, V], [7, V + 40], [10, 12, 5], [0, 5], [V - 1, 3]]
    assert rows[0, top] / pen < rows[0, second] < rows[0, top] and rows[4, V - 1] / pen > np.delete(rows[4], V - 1).max()
    assert dev[0].data_ptr() % 16 == 0 and all(dev[b].data_ptr() % 16 != 0 for b in (1, 2, 3))
    check_rows(dev, ids, pen, "special")
    W, guard = PU.words_of(V), np.int32(0x5A5A5A5A)          # the same under a bitmap of words > ceil(V / 32): the words past the row's own stay as they are
    wide = torch.from_numpy(PU.bitmap(ids, V, W + 3).view(np.int32).copy()).to(DEV)
    wide[:, W:] = int(guard)
    check_rows(dev, ids, pen, "special, wide bitmap", seen=wide)
    assert (bits(wide)[:, W:] == np.uint32(guard)).all()
    u_dev = torch.full((5,), 0.5, device=DEV)
    seen = mark(ids, V)
    before = bits(seen).copy()
    out = ops.sample_select_penalized(dev, seen, pen, top_k=1, uniforms=u_dev, want_probs=True)
    toks, probs = out["tokens"].cpu().tolist(), out["probs"].cpu().numpy()
    assert toks[0] == second and probs[0, second] == 1.0 and probs[0, top] == 0.0            # the winner under top_k = 1 changes
    assert ops.sample_select(dev, top_k=1, uniforms=u_dev)["tokens"][0].item() == top
    assert toks[3] == 0 and not probs[3].any() and toks[4] == V - 1
    assert np.array_equal(bits(seen), bitmap_after(before, toks, V)) and bits(seen)[3, 0] & 1       # bit 0 of the all -inf row
    # the seen negative logit is multiplied: its probability against an unseen neighbour of known value, everything kept at temperature 1
    full = ops.sample_select_penalized(dev, mark(ids, V), pen, uniforms=u_dev, want_probs=True)["probs"].cpu().numpy()
    j = int(np.argsort(rows[1])[::-1][0])
    want = np.exp(np.float64(rows[1, 7]) * pen - np.float64(rows[1, j]))
    assert abs(full[1, 7] / full[1, j] / want - 1.0) < 4 * SU.bound(V)
    assert not full[2, [10, 11, 12, 13]].any() and full[2].sum() > 0.99                       # -inf and NaN, seen or not: never kept


@pytest.mark.parametrize("dtype", DTYPES)
def test_aligned_rows_and_a_wider_bitmap(dtype):
    """V = 1024 (every row 16-byte aligned: the vector path) under a bitmap of words > ceil(V / 32): the words past the row's own stay as they are."""
    V, extra, pen = 1024, 3, 1.3
    rows, dev, ids = rows_and_ids(V, dtype, 3, 0)
    assert all(dev[b].data_ptr() % 16 == 0 for b in range(3))
    W = PU.words_of(V)
    guard = np.int32(0x5A5A5A5A)
    seen = torch.from_numpy(PU.bitmap(ids, V, W + extra).view(np.int32).copy()).to(DEV)
    seen[:, W:] = int(guard)
    check_rows(dev, ids, pen, "wide", seen=seen)
    assert (bits(seen)[:, W:] == np.uint32(guard)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_of_v_1024_at_an_8_byte_offset(dtype):
    """V % 8 == 0 with every row 8 bytes past a 16-byte boundary (a contiguous [B, V] view carved out of a flat buffer): the pointer half of the
    reader's `vec` decides, and the rows take the scalar path.  Same reference, same acceptance; and ops refuses a bitmap that is not contiguous."""
    from ultravox_amd import ops
    V, pen, B = 1024, 1.3, 3
    rows, aligned, ids = rows_and_ids(V, dtype, B, 0)
    off = 8 // aligned.element_size()
    flat = torch.zeros(B * V + 16, device=DEV, dtype=dtype)
    dev = flat[off:off + B * V].view(B, V)
    dev.copy_(aligned)
    assert dev.is_contiguous() and all(dev[b].data_ptr() % 16 == 8 for b in range(B))
    check_rows(dev, ids, pen, "offset")
    wide = torch.zeros(B, PU.words_of(V) + 2, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="contiguous"):
        ops.sample_select_penalized(dev, wide[:, :PU.words_of(V)], pen)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bookkeeping(dtype):
    """The scenario of test_sample_gpu.test_bookkeeping, V = 131077: a forced EOS, a row finished earlier (it writes the pad and sets its bit), a pad
    of -1 (no bit anywhere), sequences, positions, both counter slots; the argument errors."""
    from ultravox_amd import ops
    torch.manual_seed(5)
    B, V, stride, pad, pen = 4, 131072 + 5, 20, 7, 1.3
    W = PU.words_of(V)
    x = torch.randn(B, V, device=DEV).to(dtype)
    x[0, 11] = 50.0                                          # row 0 emits EOS 11 -> finished (seen or not: 50 / 1.3 stays the top)
    eos = torch.tensor([11, 12], device=DEV)
    unfinished = torch.tensor([1, 1, 0, 1], device=DEV, dtype=torch.int32)   # row 2 finished earlier -> pad
    seq = torch.full((B, stride), -1, device=DEV, dtype=torch.int64)
    pos0 = torch.tensor([5, 6, 7, 8], device=DEV, dtype=torch.int32)
    counter = torch.tensor([9, 0], device=DEV, dtype=torch.int32)     # slot 0: the previous step's count
    step, col = 3, 13
    rows = x.float().cpu().numpy()
    g = np.random.default_rng(5)
    ids = [np.concatenate([g.integers(13, V, size=400), np.argsort(-rows[b])[:3] if b else [11]]).astype(np.int64) for b in range(B)]
    seen = mark(ids, V)
    before = bits(seen).copy()
    out = ops.sample_select_penalized(x, seen, pen, top_k=1, seed=4, offset=2, eos_ids=eos, pad=pad, unfinished=unfinished, sequences=seq, col=col,
                                      positions0=pos0, step=step, counter=counter)
    nxt = out["tokens"].cpu().tolist()
    assert nxt[0] == 11 and nxt[2] == pad
    for b in (1, 3):                                         # top_k = 1: one of the (possibly tied, in bf16) maxima of the penalised row
        s = PU.penalized(rows[b], ids[b], pen)
        assert s[nxt[b]] == s.max() and nxt[b] != int(rows[b].argmax())        # (the raw top three are seen: the penalty decides)
    assert seq[:, col].cpu().tolist() == nxt and (seq[:, :col] == -1).all() and (seq[:, col + 1:] == -1).all()
    still = [0, int(nxt[1] not in (11, 12)), 0, int(nxt[3] not in (11, 12))]
    assert unfinished.cpu().tolist() == still
    assert out["positions"].cpu().tolist() == [5 + step, 6 + step, 7 + step, 8 + step]
    assert counter.cpu().tolist() == [0, sum(still)]           # counter[step & 1] = rows still running; the other slot cleared
    assert out["seen"] is seen and np.array_equal(bits(seen), bitmap_after(before, nxt, V)) and bits(seen)[2, 0] >> 7 & 1       # the pad's bit too
    # pad = -1 (eos_token_id = -1 callers): every row finished -> -1 written, no bit set anywhere - the words before, between and after the rows included
    big = torch.from_numpy(g.integers(-2 ** 31, 2 ** 31, size=(B + 2, W + 2), dtype=np.int64).astype(np.int32)).to(DEV)
    keep = big.clone()
    done = torch.zeros(B, device=DEV, dtype=torch.int32)
    o = ops.sample_select_penalized(x, big[1:1 + B], pen, pad=-1, unfinished=done, sequences=seq, col=0)
    assert o["tokens"].cpu().tolist() == [-1] * B and seq[:, 0].cpu().tolist() == [-1] * B
    assert torch.equal(big, keep)
    with pytest.raises(ValueError):
        ops.sample_select_penalized(x, seen, 0.0)
    with pytest.raises(ValueError):
        ops.sample_select_penalized(x, seen[:, :W - 1].contiguous(), pen)
    with pytest.raises(ValueError):
        ops.sample_select_penalized(x, seen, pen, top_p=0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_philox_stream(dtype):
    """uniforms = NULL under a penalty: the seeds and offsets of test_sample_gpu.test_the_philox_stream; the tokens are acceptable for the numpy
    Philox's uniforms, and two equal launches on equal bitmaps give equal tokens."""
    from ultravox_amd import ops
    V, B, pen = 4099, 24, 1.3
    rows, dev, ids = rows_and_ids(V, dtype, B, PHILOX_SEEDS[dtype])
    base = mark(ids, V)
    refs = [row_ref(rows[b], ids[b], pen, 0.7).warp(top_p=0.9) for b in range(B)]
    flat = [row_ref(rows[b], ids[b], pen, 1.0).warp() for b in range(B)]
    for b in range(B):
        assert SU.margins_ok(refs[b]), ("precondition: the reference's boundary margins", b, refs[b]["margins"])
    drawn = []
    for seed, offset in ((1, 0), ((7 << 32) | 5, 3), (12345, (1 << 32) + 9), (2 ** 64 - 1, 2 ** 64 - 1)):
        us = SU.philox_uniform(seed, offset, B)
        a = ops.sample_select_penalized(dev, base.clone(), pen, temperature=0.7, top_p=0.9, seed=seed, offset=offset)["tokens"].cpu().tolist()
        again = ops.sample_select_penalized(dev, base.clone(), pen, temperature=0.7, top_p=0.9, seed=seed, offset=offset)["tokens"].cpu().tolist()
        assert a == again
        f = ops.sample_select_penalized(dev, base.clone(), pen, seed=seed, offset=offset)["tokens"].cpu().tolist()
        for b in range(B):
            assert SU.token_ok(a[b], float(us[b]), refs[b]), (seed, offset, b, a[b], float(us[b]))
            assert SU.token_ok(f[b], float(us[b]), flat[b]), (seed, offset, b, f[b], float(us[b]))
        drawn.append(tuple(f))
    assert len(set(drawn)) == len(drawn)


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


def test_f32_generate_with_top_k_1_equals_the_greedy_penalised_device_path():
    """Left-padded B = 2, 160 prompt ids (a quarter of the vocabulary, so that the penalty decides tokens): top_k = 1 under a flagged generator draws
    what generate(repetition_penalty=...) selects on the device; the offset advances by the steps run."""
    from ultravox_amd.generation import PhiloxGenerator
    model = _small(torch.float32, 3)
    ids, am = _padded(16, T=160)
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=8, eos_token_id=-1)
    gen = PhiloxGenerator(5, penalty_on_device=True)
    for i, p in enumerate((1.2, 50.0)):
        greedy = model.generate(repetition_penalty=p, **kw)
        k1 = model.generate(do_sample=True, top_k=1, temperature=0.7, generator=gen, repetition_penalty=p, **kw)
        assert torch.equal(greedy, k1) and gen.offset == 8 * (i + 1)
    assert not torch.equal(greedy, model.generate(**kw))                 # the penalty decides somewhere


def test_bf16_generate_under_a_flagged_philox_generator():
    """The same seed replays the sequences, another seed gives others, the stream goes on across calls; an early stop pads the finished row; the
    KVState is the torch-sampler call's (cur_len, pos_next, kv_start); a second turn over past_key_values marks the prefix ids too; another
    processor next to the penalty raises today's message with the offset untouched."""
    from ultravox_amd.generation import PhiloxGenerator
    from ultravox_amd.model import KVState
    model = _small(torch.bfloat16, 3)
    T, N = 40, 8
    ids, am = _padded(16, T=T)
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=N, do_sample=True, top_k=5, top_p=0.95, repetition_penalty=1.2)
    gen = PhiloxGenerator(1, penalty_on_device=True)
    a = model.generate(eos_token_id=-1, generator=gen, **kw)
    assert gen.offset == N and a.shape == (2, T + N) and torch.equal(a[:, :T], ids)
    b = model.generate(eos_token_id=-1, generator=PhiloxGenerator(1, penalty_on_device=True), **kw)
    c = model.generate(eos_token_id=-1, generator=PhiloxGenerator(2, penalty_on_device=True), **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    cont = model.generate(eos_token_id=-1, generator=gen, **kw)      # the stream goes on: offsets 8.. draw other numbers
    assert gen.offset == 2 * N and not torch.equal(a, cont)
    # early stop: the token row 0 drew at step 3 becomes the terminator
    stop = int(a[0, T + 3])
    first = a[0, T:].tolist().index(stop)
    gen = PhiloxGenerator(1, penalty_on_device=True)
    out = model.generate(eos_token_id=stop, pad_token_id=1, generator=gen, return_dict_in_generate=True, **kw)
    row0 = out.sequences[0, T:].tolist()
    assert row0[:first + 1] == a[0, T:T + first + 1].tolist() and all(v == 1 for v in row0[first + 1:])
    n = out.sequences.shape[1] - T
    assert gen.offset == n
    st = out.past_key_values
    torch_kw = {**kw, "max_new_tokens": n}
    ts = model.generate(eos_token_id=-1, generator=torch.Generator(device=DEV).manual_seed(0), return_dict_in_generate=True, **torch_kw).past_key_values
    assert isinstance(st, KVState) and st.cur_len == ts.cur_len == T + n - 1
    assert torch.equal(st.pos_next, ts.pos_next) and torch.equal(st.kv_start, ts.kv_start)
    assert torch.equal(st.tokens, out.sequences[:, :st.cur_len])
    # a second turn: under a penalty of 50 and top_k = 1 no id of the whole row - the prefix that the cache covers included - is produced again
    first_turn = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=N, eos_token_id=-1, do_sample=True, top_k=1, repetition_penalty=50.0,
                                generator=gen, return_dict_in_generate=True)
    more = torch.randint(3, 500, (2, 5), generator=torch.Generator().manual_seed(4)).to(DEV)
    ids2 = torch.cat([first_turn.sequences, more], 1)
    am2 = torch.cat([am, torch.ones(2, ids2.shape[1] - T, dtype=torch.long, device=DEV)], 1)
    t2 = model.generate(input_ids=ids2, attention_mask=am2, past_key_values=first_turn.past_key_values, max_new_tokens=6, eos_token_id=-1, do_sample=True,
                        top_k=1, repetition_penalty=50.0, generator=gen)
    assert model.last_prefill_reused == first_turn.past_key_values.cur_len > 0
    for r in range(2):
        new = t2[r, ids2.shape[1]:].tolist()
        assert len(set(new)) == len(new) == 6 and not set(new) & set(ids2[r].tolist()), (r, new)
    at = gen.offset
    with pytest.raises(ValueError, match="PhiloxGenerator.*score processors"):
        model.generate(eos_token_id=-1, generator=gen, no_repeat_ngram_size=2, **kw)
    assert gen.offset == at


def test_the_pipeline_on_the_device():
    """A text-only turn list and an audio input through UltravoxPipeline, greedy, sampled by torch and sampled on the device: each returns a string;
    equal seeds give equal text, and the generator's offset grows across calls."""
    from fake_tokenizer import FakeChatTokenizer
    from oracle.reference_cpu import FeatureExtractorRef
    from ultravox_amd.pipeline import UltravoxPipeline

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
    pcm = (np.random.default_rng(0).standard_normal(16000) * 0.1 * 32768).astype(np.int16)
    text_in = lambda: {"turns": [{"role": "system", "content": "Be brief ."}, {"role": "user", "content": "Tell me a long story"}]}
    audio_in = lambda: {"audio": pcm, "turns": [], "sampling_rate": 16000}
    texts = []
    for seed in (9, 9, 10):
        pipe = UltravoxPipeline(model, SmallVocabTokenizer(), audio_processor=FeatureExtractorRef(80), sampler_seed=seed)
        assert pipe.sampler.seed == seed and pipe.sampler.penalty_on_device
        got = []
        for make in (text_in, audio_in):
            at = pipe.sampler.offset
            assert isinstance(pipe(make(), max_new_tokens=12), str) and pipe.sampler.offset == at       # no temperature: greedy, the stream is not touched
            got.append(pipe(make(), max_new_tokens=12, temperature=0.8))
            assert isinstance(got[-1], str) and at < pipe.sampler.offset <= at + 12
        texts.append(got)
    assert texts[0] == texts[1] and texts[0] != texts[2]
    plain = UltravoxPipeline(model, SmallVocabTokenizer(), audio_processor=FeatureExtractorRef(80))
    assert plain.sampler is None
    for make in (text_in, audio_in):
        assert isinstance(plain(make(), max_new_tokens=12, temperature=0.8), str) and isinstance(plain(make(), max_new_tokens=12), str)
