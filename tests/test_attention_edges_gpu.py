"""The bf16 attention kernels (uvx_attention_fwd / uvx_attention_bwd through ops.attention / ops.attention_bwd) at the mask and
tile edges, element by element against the float64 reference of attention_edge_util.py: padding edges on multiples of 64 / 128,
one-key windows and ranges, T on either side of every tile and of the fused backward's limit, block = tile size.

Per case three input families (R: arithmetic; V, Q: one key more or less is a large relative change of a small element of o / dv /
dq - test_attention_edges_cpu.py shows that every off-by-one of every boundary breaks these bars) and, per family: o, lse, dq, dk,
dv within their bars, exact zeros for keys nobody sees, finite outputs everywhere, bit-identical repeats, and every other kernel
form whose range logic differs bit-identical to the default (the kernel pair in place of the fused backward: within the bars).

Largest error seen on an MI355X, in bar units (the float64 restatement of the kernels reaches o 0.78, dq 0.33, dk 0.56, dv 0.75):
o 0.78 (head_dim 128, T = 321, family V), lse 0.015 (head_dim 64, T = 65, block 1, family Q), dq 0.33 (head_dim 128, T = 321, V),
dk 0.60 (head_dim 128, T = 321, V), dv 0.75 (head_dim 128, T = 320, V; the same from the fused backward and from the pair)."""
import pytest
import torch

from attention_edge_util import (CASES, FAMILIES, F64, LN2, OUTPUTS, Reference, assert_in_bars, bars, case_id, case_scale, case_seed,
                                 check_attention, describe, make_inputs, padding, visible)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(c, q, k, v, do, kv_start, kv_len, fwd=None):
    """forward + backward -> the five outputs (fwd: reuse this run's o / lse, backward only)"""
    from ultravox_amd import ops
    kw = dict(causal=c["causal"], block=c["block"], scale=case_scale(c), kv_start=kv_start, kv_len=kv_len, window=c["window"])
    o, lse = (fwd["o"], fwd["lse"]) if fwd is not None else ops.attention(q, k, v, **kw)
    dq, dk, dv = ops.attention_bwd(q, k, v, o, lse, do, **kw)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _same(a, b, what):
    for name in OUTPUTS:
        assert torch.equal(a[name], b[name]), f"{what}: {name} differs"


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_bf16_attention_at_mask_and_tile_edges(c):
    from ultravox_amd import _lib
    L = _lib.lib()
    D, T, Hq, Hkv = c["D"], c["T"], c["Hq"], c["Hkv"]
    kv_start, kv_len = padding(T, DEV)
    vis = visible(T, c["causal"], c["block"], c["window"], kv_start, kv_len)
    rows, seen = vis.any(-1), vis.any(1)                       # [B, T]: query rows that see a key; keys some query sees
    bar = bars(D, T, Hq, Hkv)
    fused = D == 128 and c["causal"] and c["block"] == 0 and T <= 320 and (c["window"] == 0 or c["window"] >= T)
    for family in FAMILIES:
        what = f"{case_id(c)} family {family}"
        q, k, v, do = make_inputs(family, 4, T, Hq, Hkv, D, case_seed(c, family), DEV)
        val, sca = Reference(q, k, v, do, case_scale(c)).full(vis)

        def held(out, form, outputs=OUTPUTS):
            got = dict(out, lse=out["lse"].to(F64) * LN2)      # log2-domain in the ABI
            res = check_attention(got, val, sca, rows, bar, outputs)
            print(f"EDGE {what} {form}: " + "  ".join(f"{n} {w:.3f} ({describe(n, i, D)})" for n, (w, i) in res.items()))
            assert_in_bars(res, D, f"{what} {form}")

        base = _run(c, q, k, v, do, kv_start, kv_len)
        held(base, "default")
        for name in ("dk", "dv"):                              # keys no query sees: exactly zero
            assert (base[name][~seen] == 0).all(), f"{what}: {name} of an unseen key is not zero"
        for name in ("o", "dq", "dk", "dv"):                   # rows that see nothing included: the product feeds them onward
            assert torch.isfinite(base[name].float()).all(), f"{what}: {name} is not finite"
        _same(_run(c, q, k, v, do, kv_start, kv_len), base, f"{what} second run")

        if fused:                                              # the dQ + dK/dV pair where the fused backward ran: another summation order
            with _lib.option(_lib.Option.ATTN_BWD_FUSED, 0):
                pair = _run(c, q, k, v, do, kv_start, kv_len, fwd=base)
            held(pair, "kernel pair", ("dq", "dk", "dv"))
            assert (pair["dk"][~seen] == 0).all() and (pair["dv"][~seen] == 0).all(), f"{what} kernel pair: unseen keys"
        if D == 64:
            for qt in (1, 2):                                  # query tiles per wave of the forward
                L.uvx_attention_force_qt(qt)
                try:
                    _same(_run(c, q, k, v, do, kv_start, kv_len), base, f"{what} force_qt({qt})")
                finally:
                    L.uvx_attention_force_qt(0)
            with _lib.option(_lib.Option.ATTN_BWD64_FORM, 1):     # one 16-row tile per wave in the backward pair
                _same(_run(c, q, k, v, do, kv_start, kv_len, fwd=base), base, f"{what} option 19 = 1")
        if D == 128 and (Hq // Hkv) % 4 == 0:
            for form in (1, 5):                                # the grouped-query block form of the forward: forced, never
                with _lib.option(_lib.Option.ATTN_FWD_GQ_FORM, form):
                    _same(_run(c, q, k, v, do, kv_start, kv_len), base, f"{what} option 25 = {form}")
