"""The four token selectors of csrc/select.hip - uvx_greedy_select, uvx_greedy_select_penalized, uvx_sample_select, uvx_sample_select_penalized -
held to each other and to numpy where all four must agree, and the argmax rule of uvx_argmax and the two greedy ones.  Nothing here has a
tolerance: the rows have a unique maximum (or the tie rule decides), penalty 1.0 is exact (x * 1.0, x / 1.0) and top_k = 1 keeps the maximum alone.

The shapes are the smallest that reach every branch of the shared row walk (sample.h: walk_row over PlainRow / PenalizedRow): V = 1; 7 (scalar path
only); 8 (one 16-byte load); 1031 (odd, > 1024: a second scalar trip, rows 1 and 2 start unaligned); 8200 (% 8 == 0, > 8192: a second vector trip);
1032 on a base one element off 16-byte alignment (the vector path is refused at run time)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
B = 3
# (V, base offset in elements, where the maximum is placed)
SHAPES = [(1, 0, [0]), (7, 0, [0, 6]), (8, 0, [0, 7]), (1031, 0, [0, 1030]), (8200, 0, [0, 8199, 8195]), (1032, 1, [0, 1031])]


def distinct_rows(g, n, V, dtype, top):
    """n rows, each a permutation of V distinct finite values with the largest at top[row]: -> the f32 values (numpy) for the reference.
    bf16: V consecutive bit patterns from 1.0 upwards; f32: the integers around zero, so both signs pass through the penalty."""
    rows = np.empty((n, V), np.float32)
    for b in range(n):
        perm = g.permutation(V)
        at = int(np.flatnonzero(perm == V - 1)[0])
        perm[at], perm[top[b]] = perm[top[b]], perm[at]
        if dtype == torch.bfloat16:
            rows[b] = ((perm.astype(np.uint32) + 0x3F80) << 16).view(np.float32)
        else:
            rows[b] = (perm - V // 2).astype(np.float32)
    return rows


def on_device(rows, dtype, offset=0):
    """rows (f32 numpy, exact in dtype) as a [n, V] device tensor whose first element lies `offset` elements into its allocation."""
    n, V = rows.shape
    flat = torch.zeros(n * V + offset, device=DEV, dtype=dtype)
    flat[offset:] = torch.from_numpy(rows).reshape(-1).to(DEV).to(dtype)
    x = flat[offset:].view(n, V)
    assert x.is_contiguous() and (x.data_ptr() % 16 != 0) == bool(offset)
    assert np.array_equal(x.float().cpu().numpy(), rows)
    return x


def bitmap_of(ids, V, words):
    m = np.zeros(words, np.uint32)
    for i in ids:
        if 0 <= i < V:
            m[i >> 5] |= np.uint32(1 << (i & 31))
    return m


@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("V,offset,tops", SHAPES, ids=[f"V{v}+{o}" for v, o, _ in SHAPES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_the_four_selectors_agree(dtype, V, offset, tops, step):
    """Penalty 1.0 over a non-empty bitmap and top_k = 1 at temperature 1: all four return numpy's argmax and leave byte-identical next_tokens,
    unfinished, sequences, positions and counter; the penalised two also leave seen_before | bit(token written).  B = 3, two EOS ids, row 1
    finished beforehand with pad = -1 (no bit), row 2's maximum on an EOS id; `sequences` wider than the columns used, sentinels everywhere else;
    the other counter slot holds a sentinel and has to be zero afterwards."""
    from ultravox_amd import ops
    g = np.random.default_rng(1000 * V + step)
    stride, col, pad, words = 7, 4, -1, (V + 31) // 32 + 1
    pos0 = np.array([5, 60, 700], np.int32)
    for i in range(len(tops)):
        top = [tops[i], tops[i], tops[(i + 1) % len(tops)]]
        rows = distinct_rows(g, B, V, dtype, top)
        x = on_device(rows, dtype, offset)
        ref = [int(np.argmax(r)) for r in rows]
        assert ref == top
        eos = [top[2], V + 3]
        written = [ref[0], pad, ref[2]]
        still = [int(ref[0] not in eos), 0, 0]
        want = dict(tokens=np.array(written, np.int64), unfinished=np.array(still, np.int32), positions=pos0 + np.int32(step),
                    sequences=np.full((B, stride), -7, np.int64), counter=np.zeros(2, np.int32))
        want["sequences"][:, col] = written
        want["counter"][step & 1] = sum(still)
        seen_ids = [list(g.integers(0, V, size=min(V, 40))) + [0, V - 1] for _ in range(B)]
        before = np.stack([bitmap_of(s, V, words) for s in seen_ids])
        assert before.any()
        after = before | np.stack([bitmap_of([t], V, words) for t in written])
        assert np.array_equal(after[1], before[1])

        def book():
            return dict(eos_ids=torch.tensor(eos, device=DEV), pad=pad, col=col, step=step, positions0=torch.from_numpy(pos0).to(DEV),
                        unfinished=torch.tensor([1, 0, 1], device=DEV, dtype=torch.int32),
                        sequences=torch.full((B, stride), -7, device=DEV, dtype=torch.int64),
                        counter=torch.tensor([0, 77] if step % 2 == 0 else [77, 0], device=DEV, dtype=torch.int32))
        seen = lambda: torch.from_numpy(before.view(np.int32).copy()).to(DEV)
        one = dict(temperature=1.0, top_k=1, seed=11, offset=step)
        outs = dict(greedy=ops.greedy_select(x, **book()),
                    greedy_penalized=ops.greedy_select_penalized(x, seen(), 1.0, **book()),
                    sample=ops.sample_select(x, **one, **book()),
                    sample_penalized=ops.sample_select_penalized(x, seen(), 1.0, **one, **book()))
        for name, out in outs.items():
            for k, w in want.items():
                got = out[k].cpu().numpy()
                assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), (name, k, i, got, w)
            if "seen" in out:
                assert np.array_equal(out["seen"].cpu().numpy().view(np.uint32), after), (name, i)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_the_argmax_rule(dtype, offset):
    """uvx_argmax, uvx_greedy_select and uvx_greedy_select_penalized (penalty 1.0) on V = 8200: strict > in ascending index order within a thread,
    the lower index among equal values across threads and waves, NaN never wins, index 0 for a row with nothing above -inf.  Aligned, 5 and 8199
    lie in thread 0 and 4100 in wave 8; on the offset base (the scalar path) they lie in three threads of wave 0."""
    from ultravox_amd import _lib as L
    from ultravox_amd import ops
    V, inf, nan = 8200, np.float32("inf"), np.float32("nan")
    g = np.random.default_rng(3)
    base = lambda: (g.integers(-64, 64, size=V) / 64.0).astype(np.float32)       # |x| < 1, exact in bf16
    rows, want = [], []
    rows.append(np.full(V, 1.5, np.float32)); want.append(0)                     # all equal
    r = base(); r[[5, 4100, 8199]] = 3.0
    rows.append(r); want.append(5)                                               # equal maxima: the lowest index
    r = base(); r[4101] = 3.0; r[[2, 4100, 4102, 8199]] = nan
    rows.append(r); want.append(4101)                                            # NaN above and below the maximum
    rows.append(np.full(V, -inf, np.float32)); want.append(0)
    rows.append(np.full(V, nan, np.float32)); want.append(0)
    rows = np.stack(rows)
    assert [int(np.argmax(np.where(np.isnan(r), -inf, r))) for r in rows] == want
    n = len(rows)
    flat = torch.zeros(n * V + offset, device=DEV, dtype=dtype)
    flat[offset:] = torch.from_numpy(rows).reshape(-1).to(DEV).to(dtype)
    x = flat[offset:].view(n, V)
    assert (x.data_ptr() % 16 != 0) == bool(offset)
    out = torch.empty(n, device=DEV, dtype=torch.int64)
    L.check(L.lib().uvx_argmax(L.stream_ptr(), L.dtype_code(dtype), L.ptr(x), n, V, L.ptr(out)), "uvx_argmax")
    assert out.cpu().tolist() == want
    assert ops.greedy_select(x)["tokens"].cpu().tolist() == want
    seen = ops.seen_mark(torch.tensor([[0, 5, 4100, 4101, 8199]] * n, device=DEV), V)
    assert ops.greedy_select_penalized(x, seen, 1.0)["tokens"].cpu().tolist() == want
