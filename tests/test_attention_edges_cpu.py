"""The harness of test_attention_edges_gpu.py proved on the CPU, so that a failure on the GPU means the kernel is wrong:
the analytic float64 backward is autograd's; a float64 restatement of the bf16 kernels (rounded where attention.hip rounds)
stays within every bar on every GPU case; every off-by-one of every mask boundary breaks the bars in the rows / keys it
touches; and the comparison is loud when fed such a result.

The float64 work runs at the GPU list's sizes with one seed per (case, family); the batch holds the four paddings of the GPU
test, one sequence each."""
import pytest
import torch

from attention_edge_util import (CASES, F64, MUTATIONS, OUTPUTS, Reference, assert_in_bars, bars, case_id, case_scale, case_seed,
                                 check_attention, make_inputs, padding, visible)


def _setup(c, family):
    kv_start, kv_len = padding(c["T"])
    q, k, v, do = make_inputs(family, 4, c["T"], c["Hq"], c["Hkv"], c["D"], case_seed(c, family))
    return Reference(q, k, v, do, case_scale(c)), kv_start, kv_len


def _vis(c, kv_start, kv_len, **mut):
    return visible(c["T"], c["causal"], c["block"], c["window"], kv_start, kv_len, **mut)


def test_analytic_backward_equals_autograd():
    """dq = sc dS K, dk = sc dS^T Q, dv = P^T dO with dS = P o (dP - delta), summed over the GQA group, against float64 autograd
    of the forward - with padding on both sides and rows that see no key (dO zeroed there for autograd)."""
    B, T, Hq, Hkv, D, sc = 3, 45, 4, 2, 64, 0.2
    q, k, v, do = make_inputs("R", B, T, Hq, Hkv, D, 5)
    kv_start = torch.tensor([0, 7, 3], dtype=torch.int32)
    kv_len = torch.tensor([T, T, T - 9], dtype=torch.int32)
    vis = visible(T, True, 0, 16, kv_start, kv_len)
    rows = vis.any(-1)
    assert rows.any() and not rows.all()
    val, _ = Reference(q, k, v, do, sc).full(vis)
    qr, kr, vr = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    s = qr.transpose(1, 2) @ kr.transpose(1, 2).repeat_interleave(Hq // Hkv, 1).transpose(-1, -2) * sc
    p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1).nan_to_num(0.0)
    o = (p @ vr.transpose(1, 2).repeat_interleave(Hq // Hkv, 1)).transpose(1, 2).reshape(B, T, Hq * D)
    assert (o.detach() - val["o"]).abs().max().item() < 1e-12
    lse = torch.logsumexp(s.masked_fill(~vis[:, None], float("-inf")), -1).detach()
    assert (lse - val["lse"])[rows[:, None].expand_as(lse)].abs().max().item() < 1e-12
    o.backward(do.to(F64) * rows[..., None])
    for name, g in (("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad)):
        assert (g - val[name]).abs().max().item() < 1e-12, name


def restatement_in_bars(c, family):
    """-> check_attention's result for the restatement of the kernels on one case and family."""
    ref, kv_start, kv_len = _setup(c, family)
    vis = _vis(c, kv_start, kv_len)
    val, sca = ref.full(vis)
    return check_attention(ref.restatement(vis), val, sca, vis.any(-1), bars(c["D"], c["T"], c["Hq"], c["Hkv"]))


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_restatement_of_the_kernels_stays_within_every_bar(c):
    """float64 arithmetic rounded to bf16 at the documented points (P, o, dS, the GQA partials, the outputs) is within every bar.
    Largest value seen over all cases and families, in bar units: o 0.78, lse 0.00, dq 0.33, dk 0.56, dv 0.75 (all in family V) -
    the bars are worst-case sums, so a kernel that rounds where the derivation says has this much room."""
    for family in ("R", "V", "Q"):
        assert_in_bars(restatement_in_bars(c, family), c["D"], f"{case_id(c)} family {family}")


def mutation_shares(c, family):
    """For every mutation that changes a visible pair -> (mutation, smallest lse move in units of its bar over the affected rows
    that still see a key, share of the affected keys whose dv moves by more than 2 bars (family V) or of the affected rows whose
    dq does (family Q); None where there is nothing to count)."""
    ref, kv_start, kv_len = _setup(c, family)
    vis = _vis(c, kv_start, kv_len)
    bar = bars(c["D"], c["T"], c["Hq"], c["Hkv"])
    name = "dv" if family == "V" else "dq"
    fwd = ref.forward(vis)
    val, sca = ref.backward(fwd, want=(name,))
    lse_scale = fwd["lse"].abs() + 4 * ref.sc * c["D"] ** 0.5
    out = []
    for kind, d in MUTATIONS:
        vis_m = _vis(c, kv_start, kv_len, **{kind: d})
        changed = vis_m != vis
        if not changed.any():
            continue
        fwd_m = ref.forward(vis_m)
        rows = changed.any(-1) & vis.any(-1) & vis_m.any(-1)                      # [B, T] affected, a key before and after
        lse_move = None
        if rows.any():
            move = (fwd_m["lse"] - fwd["lse"]).abs() / (bar["lse"] * lse_scale)
            lse_move = move[rows[:, None].expand_as(move)].min().item()
        val_m, _ = ref.backward(fwd_m, want=(name,), scales=False)
        with torch.no_grad():
            diff = (val_m[name] - val[name]).abs()
            units = torch.where(diff == 0, torch.zeros_like(diff), diff / (bar[name] * sca[name])).amax((-1, -2))   # [B, T]
        where = changed.any(1) if family == "V" else rows                         # affected keys / affected rows
        share = (units[where] > 2).double().mean().item() if where.any() else None
        out.append(((kind, d), lse_move, share))
    return out


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_off_by_one_of_every_boundary_breaks_the_bars(c):
    """The float64 reference under a mask with ONE boundary moved by ONE key against the reference under the true mask: lse moves
    by more than 4 bars in every affected row that still sees a key; dv (family V) moves by more than 2 bars in at least 95 % of
    the affected keys, dq (family Q) in at least 95 % of the affected rows.  A kernel with that off-by-one cannot pass the GPU test."""
    n = 0
    for family in ("V", "Q"):
        for mut, lse_move, share in mutation_shares(c, family):
            n += 1
            assert lse_move is None or lse_move > 4, (family, mut, lse_move)
            assert share is None or share >= 0.95, (family, mut, share)
    assert n >= 2 or c["T"] == 1                  # (at T = 1 only a boundary moved across the one key changes anything)


_LLM129 = next(c for c in CASES if c["D"] == 128 and c["T"] == 129 and c["Hq"] == 4)
LOUD = {"d_diag": (_LLM129, 1), "d_window": (next(c for c in CASES if c["window"] == 64 and c["T"] == 200), -1),
        "d_block": (next(c for c in CASES if c["block"] == 64 and c["T"] == 129), 1), "d_start": (_LLM129, -1), "d_len": (_LLM129, 1)}


@pytest.mark.parametrize("kind", sorted(LOUD))
def test_comparison_is_loud_on_a_kernel_with_an_off_by_one(kind):
    """The restatement of the kernels computed under a mutated mask - what a kernel with that off-by-one would return - fed to
    check_attention against the true reference: the assertion fires, in the edge-loud families and on lse."""
    c, d = LOUD[kind]
    for family in ("V", "Q"):
        ref, kv_start, kv_len = _setup(c, family)
        vis = _vis(c, kv_start, kv_len)
        vis_m = _vis(c, kv_start, kv_len, **{kind: d})
        assert (vis_m != vis).any()
        val, sca = ref.full(vis)
        res = check_attention(ref.restatement(vis_m), val, sca, vis.any(-1) & vis_m.any(-1), bars(c["D"], c["T"], c["Hq"], c["Hkv"]))
        assert res["lse"][0] > 4 and res["dv" if family == "V" else "dq"][0] > 2, res
        with pytest.raises(AssertionError, match="lse: .* bars at batch \\d+ head \\d+ row \\d+"):
            assert_in_bars(res, c["D"], f"{case_id(c)} {kind}")
        assert set(res) == set(OUTPUTS)
