"""The harness of test_norm_edges_gpu.py, proven without a GPU (norm_edge_util.py):

1. the f32 restatement of every norm kernel, with the kernel's own summation order and rounding points, stays inside the float64 reference's bars
   on every case, family and edge vector.  Largest error in bar units per kernel and output, with the case and family (P: its edge vector):
     layernorm_fwd_wave_k  y   0.998  ln-4x512, R                layernorm_fwd_k    y   0.998  ln-5x504, P 62
     layernorm_bwd_k       dx  0.999  ln_bwd-5x8, Z              rmsnorm_fwd_wave_k y   0.999  rms-9x512, R
     rmsnorm_fwd_reg_k     y   0.998  rms-4x1544, R              rmsnorm_fwd_k      y   0.998  rms-513x4096, P 256
     rmsnorm_bwd_k         dx  0.998  rms_bwd-17x8-dx_add, R     rmsnorm_bwd_k      dw  0.995  rms_bwd-1x4096-dx_dw, P 255
     qk_norm_rope_k        qk  0.975  qk-d64-h5x1-f1-raw, Z      qk_norm_bwd_k      dqk 0.999  qk_bwd-d64-h5x1-f0, P (0, 7)
     through uvx_gemm_rmsnorm, flavor 1:  rmsnorm_fwd_wave_k 0.998 gemma-3x512-f1, Z   rmsnorm_fwd_reg_k 0.997 gemma-3x576-f1, Z   rmsnorm_fwd_k 0.994 gemma-3x8256-f1, P 512
   (a bar is the SUM of the half ulps on a path: among thousands of elements one comes within a part in a thousand of all of them at once);
2. the reference equals plain torch float64 (F.layer_norm, autograd, the rotate-half form of RoPE) to 1e-12;
3. the case list reaches every bf16 instantiation the dispatchers can launch through these entry points, on both sides of every boundary;
4. every off-by-one of the list below, applied to the restatement, breaks a bar (an element that is never stored keeps its canary, a NaN, and
   breaks every bar) on EVERY case it has a meaning on.  The case and family named with each is the first one that catches it:
     last_vec_drop      rms-1x8, P 0                  sweep_first_twice  rms-1x8, P 0              mean_padded     rms-1x8, P 0
     nv_one_short       rms-1x1024, P 0               row_guard          rms-1x512, P 0            ln_var_about_0  ln-1x512, P 0
     dx_add_ignored     rms_bwd-1x8-dx_add, P 0       coef_without_cols  rms_bwd-1x8-dx, P 0       dw_last_row     rms_bwd-1x8-dw, P 0
     butterfly_half     qk-d64-h1x1-f0, P (0, 0)      k_with_wq          qk-d64-h1x1-f0, P (0, 0)  pos_row_div_T   qk-d64-h1x1-f0, P (0, 0)
     raw_after_norm     qk-d64-h1x1-f0-raw, P (0, 0)
   and family R alone - white noise - misses a dropped or doubled vector on 8 of the (mutation, case) pairs from 504 columns on, and sees the others only
   through the one element in a thousand that sits at the edge of its bar: what the P family is for."""
import torch
import torch.nn.functional as F

import norm_edge_util as N
from norm_edge_util import CASES, F64, FAMILIES, MUTATIONS, case_id


def _runs(c, families=FAMILIES):
    for fam in families:
        for v in N.variants(c, fam):
            yield fam, v, N.make_inputs(c, fam, v)


def test_restatement_stays_within_every_bar():
    worst = {}
    for c in CASES:
        for fam, v, inp in _runs(c):
            ref, re = N.reference(c, inp), N.restatement(c, inp)
            assert set(ref) == set(re)
            for k in ref:
                u = N.bar_units(re[k], ref[k])
                assert u <= 1.0, f"{case_id(c)} family {fam} {v}: {k} at {u:.3f} bars"
                key = (N._kernel(c)[0] + (" flavor 1" if c.get("flavor") and c["entry"] == "gemma" else ""), k)
                if u > worst.get(key, (0.0,))[0]:
                    worst[key] = (u, case_id(c), fam, v)
            if c["entry"] in ("rms", "gemma"):      # the forced two-pass form is the same arithmetic in the same order
                assert torch.equal(re["y"], N.restatement(c, inp, two_pass=1)["y"])
    for (kern, out), (u, cid, fam, v) in sorted(worst.items()):
        print(f"NORM-EDGE restatement {kern:22s} {out:4s} {u:.3f}  {cid}, {fam} {'' if v is None else v}")


def _rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


def test_reference_is_plain_float64_torch():
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12, msg=lambda m: f"{what}: {m}")
    picks = [c for c in CASES if (c["rows"], c["cols"]) in ((5, 520), (5, 512), (17, 2056), (17, 8), (3, 576)) or (c["entry"] in ("qk", "qk_bwd") and c["cols"] == 64)]
    assert {c["entry"] for c in picks} == {"rms", "rms_bwd", "ln", "ln_bwd", "gemma", "qk", "qk_bwd"}
    for c in picks:
        for fam in ("R", "Z"):
            inp = {k: v.to(F64) for k, v in N.make_inputs(c, fam).items()}
            ref = {k: v[0] for k, v in N.reference(c, inp).items()}
            e, cols, what = c["entry"], c["cols"], f"{case_id(c)} {fam}"
            rms = lambda x, w, eps=N.RMS_EPS: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
            if e in ("rms", "gemma"):
                close(ref["y"], rms(inp["x"], 1.0 + inp["w"] if c.get("flavor") else inp["w"]), what)
            elif e == "ln":
                close(ref["y"], F.layer_norm(inp["x"], (cols,), inp["w"], inp["b"], N.LN_EPS), what)
            elif e in ("ln_bwd", "rms_bwd"):
                x, w = inp["x"].clone().requires_grad_(True), inp["w"].clone().requires_grad_(True)
                y = F.layer_norm(x, (cols,), w, torch.zeros_like(w), N.LN_EPS) if e == "ln_bwd" else rms(x, w)
                y.backward(inp["dy"])
                if "dx" in ref:
                    close(ref["dx"], x.grad + (inp["add"] if "add" in inp else 0.0), what)
                if "dw" in ref:
                    close(ref["dw"], w.grad, what)
            else:
                H, D, rows = c["Hq"] + c["Hkv"], cols, c["rows"]
                src = (inp["qkv"] if e == "qk" else inp["raw"])[:, :H * D].reshape(rows, H, D).clone().requires_grad_(True)
                w = torch.cat((inp["wq"].expand(c["Hq"], D), inp["wk"].expand(c["Hkv"], D)))
                n = rms(src, 1.0 + w if c["flavor"] else w)
                if e == "qk":
                    cs = inp["cs"][torch.arange(rows) % c["T"]][:, None]
                    co, si = torch.cat((cs[..., 0], cs[..., 0]), -1), torch.cat((cs[..., 1], cs[..., 1]), -1)
                    close(ref["qk"], (n * co + _rot_half(n) * si).reshape(rows, -1), what)
                    if c.get("raw"):
                        assert torch.equal(ref["raw"], inp["qkv"][:, :H * D])
                else:
                    n.backward(inp["dqkv"][:, :H * D].reshape(rows, H, D))
                    close(ref["dqk"], src.grad.reshape(rows, -1), what)


def test_zero_and_constant_rows_of_the_reference():
    """family Z: RMSNorm of the zero row is exactly 0 with a bar of 0; its backward is rsqrt(eps) dy w; LayerNorm of the constant row is the bias"""
    for c in CASES:
        if c["entry"] in ("qk", "qk_bwd"):
            continue
        inp = N.make_inputs(c, "Z")
        f = {k: v.to(F64) for k, v in inp.items()}
        ref = N.reference(c, inp)
        assert not f["x"][-1].any() and (c["rows"] == 1 or (f["x"][0] == 0.5).all())
        if c["entry"] in ("rms", "gemma"):
            assert not ref["y"][0][-1].any() and not ref["y"][1][-1].any()
        if c["entry"] == "rms_bwd" and "dx" in ref:
            want = f["dy"][-1] * f["w"] / N.RMS_EPS ** 0.5 + (f["add"][-1] if "add" in f else 0.0)
            torch.testing.assert_close(ref["dx"][0][-1], want, rtol=1e-12, atol=1e-12)
        if c["entry"] == "ln":
            assert f["b"].abs().min() >= 0.125
            torch.testing.assert_close(ref["y"][0][0 if c["rows"] > 1 else -1], f["b"], rtol=1e-12, atol=1e-12)
        for k, v in N.restatement(c, inp).items():
            assert torch.isfinite(v).all(), f"{case_id(c)}: {k}"


def test_case_list_reaches_every_instantiation_and_both_sides_of_every_boundary():
    S = N.served_by
    reached = {S(c["entry"], c["rows"], c["cols"], 0, c.get("mode")) for c in CASES}
    reached |= {S(c["entry"], c["rows"], c["cols"], 1) for c in CASES if c["entry"] == "rms"}      # every register case runs again under the two-pass option
    assert reached == N.reachable(), sorted(N.reachable() ^ reached, key=str)
    has = lambda entry, rows, cols, **kw: any(c["entry"] == entry and c["rows"] == rows and c["cols"] == cols and all(c.get(k) == v for k, v in kw.items()) for c in CASES)
    # the rows <= 512 boundary, and 513 rows at a wave width
    assert has("rms", 512, 4096) and S("rms", 512, 4096) == ("rmsnorm_fwd_reg_k", 2, 256)
    assert has("rms", 513, 4096) and S("rms", 513, 4096) == ("rmsnorm_fwd_k", 256)
    assert has("rms", 513, 1024) and S("rms", 513, 1024) == ("rmsnorm_fwd_wave_k", 2)
    # the register boundaries
    for lo, hi, klo, khi in ((2048, 2056, ("rmsnorm_fwd_wave_k", 4), ("rmsnorm_fwd_reg_k", 2, 256)), (4096, 4104, ("rmsnorm_fwd_reg_k", 2, 256), ("rmsnorm_fwd_reg_k", 4, 256)),
                             (8192, 8200, ("rmsnorm_fwd_reg_k", 4, 256), ("rmsnorm_fwd_k", 256)), (2040, 2048, ("rmsnorm_fwd_reg_k", 1, 256), ("rmsnorm_fwd_wave_k", 4)),
                             (504, 512, ("rmsnorm_fwd_reg_k", 1, 64), ("rmsnorm_fwd_wave_k", 1)), (512, 520, ("rmsnorm_fwd_wave_k", 1), ("rmsnorm_fwd_reg_k", 1, 128)),
                             (1536, 1544, ("rmsnorm_fwd_reg_k", 1, 192), ("rmsnorm_fwd_reg_k", 1, 256))):
        for rows in (1, 3, 4, 5):
            assert has("rms", rows, lo) and has("rms", rows, hi) and S("rms", rows, lo) == klo and S("rms", rows, hi) == khi
    # the backward's MV boundaries and its limit
    for mode in N.RMS_BWD_MODES:
        for rows in (1, 17):
            assert [S("rms_bwd", rows, cols, 0, mode)[3] for cols in (2048, 2056, 4096, 4104, 12288) if has("rms_bwd", rows, cols, mode=mode)] == [1, 2, 2, 6, 6]
    assert S("rms_bwd", 1, 12296, 0, "dx") == "rejected" and S("rms", 1, 12296)[0] == "rmsnorm_fwd_k"
    assert all(S(e, 1, N.REJECTED_COLS, 0, "dx") == "rejected" for e in ("ln", "ln_bwd", "rms", "rms_bwd", "gemma")) and S("qk", 15, 96) == S("qk_bwd", 15, 96) == "rejected"
    assert S("rms", 0, 8) == S("ln", 0, 8) == S("qk", 0, 64) == "noop"
    # gemma: one K for each forward form
    assert [S("gemma", 3, K)[:2] for K in N.GEMMA_K] == [("rmsnorm_fwd_wave_k", 1), ("rmsnorm_fwd_reg_k", 1), ("rmsnorm_fwd_reg_k", 2), ("rmsnorm_fwd_reg_k", 4), ("rmsnorm_fwd_k", 256)]
    # the per-head launches: strided rows with v columns and a pad, positions that wrap twice, a partial last block
    for c in CASES:
        if c["entry"] in ("qk", "qk_bwd"):
            n = c["rows"] * (c["Hq"] + c["Hkv"]) * (c["cols"] // (16 if c["entry"] == "qk" else 8))
            assert n % 256 and c["rows"] == 3 * c["T"] and c["ld"] == (c["Hq"] + 2 * c["Hkv"]) * c["cols"] + 8
    # the P family's edge vectors: both sides of every sweep boundary
    assert N.variants(dict(entry="rms", rows=1, cols=6144), "P") == (0, 255, 256, 511, 512, 767)
    assert N.variants(dict(entry="rms", rows=1, cols=1024), "P") == (0, 63, 64, 127) and N.variants(dict(entry="rms_bwd", rows=1, cols=4104, mode="dx"), "P") == (0, 255, 256, 511, 512)
    assert N.variants(dict(entry="ln", rows=1, cols=520), "P") == (0, 64) and N.variants(dict(entry="rms", rows=1, cols=1536), "P") == (0, 191)


def test_every_mutation_breaks_a_bar_on_every_case_it_touches():
    first, white_noise_misses = {}, set()
    sums = {"last_vec_drop", "sweep_first_twice"}
    for c in CASES:
        touching = {m for m in MUTATIONS if N.touches(m, c)}
        caught, caught_by_R = set(), set()
        for fam, v, inp in _runs(c, ("P", "Z", "R")):
            ms = (touching - caught) | (sums & touching if fam == "R" else set())
            if not ms:
                continue
            ref = N.reference(c, inp)
            for m in sorted(ms):
                re = N.restatement(c, inp, mut=m)
                if max(N.bar_units(re[k], ref[k]) for k in ref) > 1.0:
                    caught.add(m)
                    first.setdefault(m, f"{case_id(c)}, {fam} {'' if v is None else v}")
                    if fam == "R":
                        caught_by_R.add(m)
        assert caught == touching, f"{case_id(c)}: no family catches {sorted(touching - caught)}"
        if c["entry"] not in ("qk", "qk_bwd") and c["cols"] >= 504:
            white_noise_misses |= {(m, case_id(c)) for m in sums & touching if m not in caught_by_R}
    assert set(first) == set(MUTATIONS)
    for m in MUTATIONS:
        print(f"NORM-EDGE mutation {m:18s} first caught by {first[m]}")
    print(f"NORM-EDGE family R alone misses a dropped or doubled vector on {len(white_noise_misses)} (mutation, case) pairs")
    assert white_noise_misses, "family R alone sees a dropped vector everywhere: the P family would be for nothing"
