"""The harness of test_gemm_edges_gpu.py proved on the CPU, so that a failure on the GPU means the kernel is wrong: the float64 reference is
plain torch's (F.gelu, autograd for the two backward epilogues, operands taken with as_strided instead of the util's index arithmetic); a
restatement of the kernels' arithmetic (f32 accumulation in MFMA-step order, bf16 roundings where gemm.hip rounds) stays within every bar
on every GPU case, form and family and is bit-equal in family S wherever the GPU test asserts bit-equality; every off-by-one of
gemm_edge_util.mutations is detected on every case it touches; and the comparison is loud on one wrong element and on a written canary."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_edge_util as U
from gemm_edge_util import CASES, F64, HEAD, case_id, families, make_problem, with_form


def _strided(buf, off, shape, strides):
    return torch.as_strided(buf, shape, strides, off).to(F64)


def _plain_torch(p):
    """{out: [Z, M, W]} from plain torch float64 on as_strided views of the buffers."""
    g, b = p.g, p.buf
    M, N, K, Z = g["M"], g["N"], g["K"], g["Z"]
    A = _strided(b["A"], HEAD, (Z, M, K), (g["sA"], g["lda"], 1))
    B = _strided(b["B"], HEAD, (Z, N, K), (g["sB"], 1, g["ldb"]) if g["nn"] else (g["sB"], g["ldb"], 1))
    x = g["alpha"] * torch.einsum("zmk,znk->zmn", A, B)
    if g["has_bias"]:
        x = x + b["bias"][HEAD:HEAD + N].to(F64)
    form = g["form"]
    if form == "act2":
        return {"C": x, "C2": F.gelu(x)}
    if form == "act3":
        pre = _strided(b["C2"], HEAD, (1, M, N), (0, g["ldc2"], 1)).requires_grad_(True)
        F.gelu(pre).backward(x)                      # d pre = d out * gelu'(pre)
        return {"C": pre.grad}
    if form == "ep1":
        blk = x.view(Z, M, N // 32, 2, 16)
        return {"C": x, "C2": (F.silu(blk[:, :, :, 0]) * blk[:, :, :, 1]).reshape(Z, M, N // 2)}
    if form == "ep2":
        gu = _strided(b["C2"], HEAD, (1, M, 2 * N), (0, g["ldc2"], 1)).requires_grad_(True)
        blk = gu.view(1, M, N // 16, 2, 16)
        (F.silu(blk[:, :, :, 0]) * blk[:, :, :, 1]).reshape(1, M, N).backward(x)
        return {"C": gu.grad}
    if g["act"] == 1:
        x = F.gelu(x)
    if g["Mr"]:
        r = _strided(b["R"], HEAD, (Z, g["Mr"], N), (g["sR"], g["ldr"], 1))
        x = x + r[:, torch.arange(M) % g["Mr"]]
    if g["accumulate"]:
        x = x + _strided(b["C"], HEAD, (Z, M, N), (g["sC"], g["ldc"], 1))
    return {"C": x}


def _one_per(pred):
    seen, out = set(), []
    for c in CASES:
        for f in c["forms"]:
            key = pred(c, f)
            if key not in seen:
                seen.add(key)
                out.append((c, f))
    return out


@pytest.mark.parametrize("c,form", _one_per(lambda c, f: (f, c.get("layout"), bool(c.get("b_kn")), c["group"] == "tail")), ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_reference_equals_plain_torch_float64(c, form):
    """One case per epilogue form, batched layout and operand form: the reference's values, where its mask says they land, against plain
    torch; everything the mask leaves out is not an output."""
    c = with_form(c, form)
    fam = "G" if c["group"] == "tail" else families(c, form)[-2]
    p = make_problem(c, fam)
    want = _plain_torch(p)
    ref = U.reference(p)
    g = p.g
    for name, img in ref.items():
        w = want[name]
        ld, s = (g["ldc"], g["sC"]) if name == "C" else (g["ldc2"], 0)
        got = torch.as_strided(img.val, tuple(w.shape), (s, ld, 1), HEAD)
        scale = max(1.0, float(w.abs().max()))
        assert (got - w).abs().max().item() <= 1e-12 * scale, (name, (got - w).abs().max().item())
        assert int(img.mask.sum()) == w.numel() or g["layout"] == "group"
        assert torch.as_strided(img.mask, tuple(w.shape), (s, ld, 1), HEAD).all()


@functools.lru_cache(maxsize=None)
def _restatement(i, form, fam):
    c = with_form(CASES[i], form)
    p = make_problem(c, fam)
    ref = U.reference(p)
    rs = U.restatement(p, U.kstep(c, form))
    exact = U.kernel_images(p, U.operands(p))
    got = {}
    for name, img in rs.items():
        buf = p.buf[name].clone()
        buf[img.mask] = img.val[img.mask].to(buf.dtype)
        got[name] = buf
    res = U.compare(p, ref, got, exact if U.biteq_outputs(p) else None)
    return U.Problem(c, fam, p.g, {}), res          # (the descriptor only: the buffers are not kept)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: case_id(CASES[i]))
def test_restatement_of_the_kernels_stays_within_every_bar(i):
    """f32 accumulation in MFMA-step order with the bf16 roundings of gemm.hip is within every bar, leaves every canary alone and - family S / Sb,
    forms without a transcendental - equals the exactly accumulated chain bit for bit.  Largest value over all cases, forms and families, in bar
    units per output kind (test_largest_restatement_error_per_output_kind prints them):
      plain 0.995  bias 0.996  alpha 0.996  bias_gelu 0.933  bias_res 0.990  res_mod 0.989  f32 0.082  f32_acc 0.095  act2 0.996  act2.C2 0.933
      act3 0.954  ep1 0.996  ep1.C2 0.833  ep2 0.973
    (0.996: a value just above a power of two rounded by half an ulp - a bar of one rounding has no slack, by construction)."""
    c = CASES[i]
    for form in c["forms"]:
        for fam in families(c, form):
            p, res = _restatement(i, form, fam)
            U.assert_ok(p, res, f"{case_id(c)} {form} family {fam}")
            for name in U.biteq_outputs(p):
                assert res[name]["unequal"] == 0


def test_largest_restatement_error_per_output_kind():
    worst = {}
    for i, c in enumerate(CASES):
        for form in c["forms"]:
            for fam in families(c, form):
                p, res = _restatement(i, form, fam)
                for name, r in res.items():
                    k = U.kind(p, name)
                    if r["worst"] > worst.get(k, (-1.0,))[0]:
                        worst[k] = (r["worst"], case_id(c), fam)
    print("RESTATEMENT " + "  ".join(f"{k} {w:.3f} ({cid}, {fam})" for k, (w, cid, fam) in sorted(worst.items())))
    assert worst and all(w < 1.0 for w, _, _ in worst.values()), worst
    assert {f for c in CASES for f in c["forms"]} == {k.split(".")[0] for k in worst} == set(U.FORMS)


def test_tile_cases_cover_what_the_issue_names():
    """Per forced tile variant: every M in {1, bm - 1, bm, bm + 1, 2 bm + 1}, every K, every N, all eight epilogues, and on either side of
    N % 8 a residual and a GELU form; the second-operand epilogues on every variant; every reduce epilogue at 5 and at 37 K-tiles."""
    eight = {"plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "f32", "f32_acc"}
    for v, bm in U.BM.items():
        mine = [c for c in CASES if c["group"] == "tiles" and c["variant"] == v]
        assert {c["M"] for c in mine} >= {1, bm - 1, bm, bm + 1, 2 * bm + 1}, v
        assert {c["K"] for c in mine} >= {64, 128, 192, 320, 64 * 37}, v
        assert {c["N"] for c in mine} >= {4, 132, 252, 256, 260, 520}, v
        assert {f for c in mine for f in c["forms"]} >= eight, v
        for aligned in (True, False):
            forms = {f for c in mine if (c["N"] % 8 == 0) == aligned for f in c["forms"]}
            assert {"bias_res", "bias_gelu", "res_mod"} <= forms, (v, aligned)
        second = {f for c in CASES if c["group"] == "second" and c["variant"] == v for f in c["forms"]}
        assert second == {"act2", "act3", "ep1", "ep2"}, v
    for nk in (5, 37):
        forms = {f for c in CASES if c["group"] == "splitk" and c["K"] == 64 * nk for f in c["forms"]}
        assert forms == {"plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "ep1"}, nk
        assert {c["split"] for c in CASES if c["group"] == "splitk" and c["K"] == 64 * nk} == {2, 3, 5, 16}


def _moved_bits(a, b, dtype):
    """elementwise: the two float64 values differ once stored as `dtype` (a NaN counts as different)"""
    return U.output_bits(a.to(dtype)) != U.output_bits(b.to(dtype))


@functools.lru_cache(maxsize=None)
def _detection(i, form, fam):
    """-> {mutation name: (affected elements, share of them detected)} for every mutation with a meaning on the case."""
    c = with_form(CASES[i], form)
    p = make_problem(c, fam)
    true = U.reference(p)
    selector = fam in ("S", "Sb")
    k_true = U.kernel_images(p, U.operands(p)) if selector else None
    out = {}
    for mut in U.mutations(c):
        o = U.operands(p, mut)
        ref_m = U.images(p, U.ref_epilogue(p.g, o), o["touched"], mut)
        k_m = U.kernel_images(p, o, mut) if selector else None
        tally = {True: [0, 0, 0], False: [0, 0, 0]}                                      # exact outputs / outputs held to bars: [affected, detected]
        for name, t in true.items():
            m = ref_m[name]
            placed = t.mask != m.mask                                            # written where it must not be, or not written: the canary check
            both = t.mask & m.mask
            struct = both & ((t.src != m.src) | m.touched) & t.live
            exact = selector and name in U.biteq_outputs(p)
            n_struct = int(struct.sum())
            if exact:        # every element whose exact value the mutation changes: the kernels' chain must change too (no rounding hides it)
                struct = struct & ~(m.val == t.val)
                moved = _moved_bits(k_true[name].val, k_m[name].val, p.buf[name].dtype)
            else:
                moved = ~((m.val - t.val).abs() <= 2.0 * t.bar)                  # (a NaN read out of the padding: moved)
            if selector and not exact:       # (the selector families answer for their exact outputs; GELU / SiLU outputs are R's and G's)
                continue
            tally[exact][0] += int(placed.sum() + struct.sum())
            tally[exact][1] += int(placed.sum() + (struct & moved).sum())
            tally[exact][2] += int(placed.sum()) + n_struct
        for exact, (n_aff, n_det, n_all) in tally.items():
            if n_aff:
                out[(U.mut_name(mut), exact)] = (n_aff, n_det / n_aff, n_aff / n_all)
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: case_id(CASES[i]))
def test_every_off_by_one_is_detected(i):
    """The reference under ONE mutated piece of index arithmetic against the true reference, on every element the mutation touches (an element
    written from another logical element, or whose terms change, where the output still depends on its pre-activation): family S / Sb - wherever
    that changes the exact value (reading the same operand values elsewhere changes nothing) the kernels' chain differs bit for bit (its GELU /
    SiLU outputs are not exact and not counted: families R and G answer for those); family R - every one moves by more than 2 bars (but for the displaced reads of
    gemm_edge_util.DISPLACED, which a periodic ramp cannot all see); family G - at least 95 % do.  Elements
    written outside the true output, or left unwritten, count as detected: the canary check is bit-exact."""
    c = CASES[i]
    for form in c["forms"]:
        for fam in families(c, form):
            for (name, exact), (n, share, kept) in _detection(i, form, fam).items():
                if fam == "R" and name in U.DISPLACED:        # (see gemm_edge_util.DISPLACED: the selector families and G answer for these;
                    assert share >= 0.5, f"{case_id(c)} {form} family R: mutation {name} detected in {share:.4f} of {n}"      # a floor for the ramp)
                    continue
                if fam == "G" and name in U.K_RANGE and c["K"] >= 2048 and form not in ("plain", "bias", "alpha", "f32", "f32_acc"):
                    continue     # (one Gaussian K-tile in 37 under two roundings: 2 bars in ~93 % only; the 5-tile cases and families S, R answer)
                need = 1.0 if (exact or fam == "R") else 0.95
                assert kept >= 0.5, f"{case_id(c)} {form} family {fam}: mutation {name} changes only {kept:.3f} of the elements it touches"
                assert share >= need, f"{case_id(c)} {form} family {fam}: mutation {name} detected in {share:.4f} of {n} affected elements"


def test_every_mutation_is_covered_by_some_case():
    covered = {}
    for i, c in enumerate(CASES):
        for form in c["forms"]:
            for fam in families(c, form):
                for name, _ in _detection(i, form, fam):
                    covered.setdefault(name, set()).add(fam)
    print(f"MUTATIONS covered {len(covered)} of {len(U.ALL_MUTATIONS)}")
    assert set(covered) == set(U.ALL_MUTATIONS), set(U.ALL_MUTATIONS) ^ set(covered)
    for name, fams in covered.items():
        # (c2_ldc and a tail launch's C2 offset touch only GELU / SiLU outputs, none of which is exact: no selector family counts there)
        assert "G" in fams and (fams & {"S", "Sb"} or name in ("c2_ldc", "tail_off:C2")) and ("R" in fams or name in U.DISPLACED), (name, fams)


def _loud_setup():
    c = with_form(next(c for c in CASES if c["group"] == "ld" and c.get("pad") == dict(c=8)), "bias_res")
    p = make_problem(c, "G")
    ref = U.reference(p)
    got = {"C": p.buf["C"].clone()}
    img = ref["C"]
    got["C"][img.mask] = img.val[img.mask].to(torch.bfloat16)
    return p, ref, got


def test_comparison_fires_on_one_element_wrong_by_two_bars():
    p, ref, got = _loud_setup()
    U.assert_ok(p, U.compare(p, ref, got), "the rounded reference itself")
    img = ref["C"]
    at = int(torch.nonzero(img.mask)[1234])
    wrong = img.val[at] + 2.0 * img.bar[at]
    got["C"][at] = wrong.to(torch.bfloat16)
    assert abs(float(got["C"][at]) - float(img.val[at])) > 1.0 * float(img.bar[at])
    res = U.compare(p, ref, got)
    assert res["C"]["at"] == at and res["C"]["worst"] > 1.0
    with pytest.raises(AssertionError, match=r"bars at C\[\d+\] \(batch 0, row \d+, column \d+\)"):
        U.assert_ok(p, res, "one wrong element")


def test_comparison_fires_on_a_written_canary():
    p, ref, got = _loud_setup()
    img = ref["C"]
    for at in (HEAD - 1, HEAD + p.g["N"], int(torch.nonzero(img.mask)[-1]) + 1):      # before the output, a padding column of row 0, after the last row
        assert not img.mask[at]
        spoiled = {"C": got["C"].clone()}
        spoiled["C"][at] = 0.0
        res = U.compare(p, ref, spoiled)
        assert res["C"]["canary"] == 1 and res["C"]["first"] == at
        with pytest.raises(AssertionError, match="outside the output"):
            U.assert_ok(p, res, "a written canary")
    nan = {"C": got["C"].clone()}
    nan["C"][int(torch.nonzero(img.mask)[5])] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        U.assert_ok(p, U.compare(p, ref, nan), "a NaN output")
