"""The harness of test_gemm_skinny_edges_gpu.py proved on the CPU, so that a failure on the GPU means a kernel of gemm_skinny.hip is wrong: an f32
restatement of each kernel's summation order (row kernel: per lane, butterfly, waves; fragment kernel: per 32-column chunk in the wave's span or
interleave order, waves; staged kernel: the same over each wave's contiguous span; the fused prologues' sums of squares in their own orders) with
the quotient-form SiLU stays within every bar on every case, form and family and is bit-equal in families S / Sb; the reference's norm stage
equals plain torch float64; every off-by-one of gemm_skinny_edge_util.mutations is detected on every case it touches; the case list covers what
the dispatcher can launch; and at most 1e-3 of a fused case's activations are tippable.

Three deliberate errors in gemm_skinny.hip and the restated mutation that stands for each, with a case that catches it
(test_three_kernel_mutants_are_caught_by_named_cases):
  the `n >= p.N` store guard gone (the clamped rows' products written past N)   cols_past_n, clamp_written   frag-3x4x64 plain, family S
  `w + 1` for `w` in a span bound (a wave's chunks summed by two waves)          wave_twice                   frag-15x20x512, family Sb
  `16 * t` dropped from issue() (tile 1 streams tile 0's weight rows)            tile1_as_tile0               staged-17x16388x2048 bias_res, family S"""
import functools

import pytest
import torch

import gemm_edge_util as U
import gemm_skinny_edge_util as S
from gemm_edge_util import F64, HEAD
from gemm_skinny_edge_util import CASES, case_id, families, make_problem, with_form


def _index(cid):
    return next(i for i, c in enumerate(CASES) if case_id(c) == cid)


# ------------------------------------------------------------------ restatement
@functools.lru_cache(maxsize=None)
def _restatement(i, form, fam):
    c = with_form(CASES[i], form)
    p = make_problem(c, fam)
    ref = S.reference(p)
    rs = S.restatement(p)
    exact = S.kernel_images(p, S.operands(p)) if S.biteq_outputs(p) else None
    got = {}
    for name, img in rs.items():
        buf = p.buf[name].clone()
        buf[img.mask] = img.val[img.mask].to(buf.dtype)
        got[name] = buf
    res = U.compare(p, ref, got, exact)
    tips = p.tips[0] if S.fused(c) else None
    return U.Problem(c, fam, p.g, {}), res, tips


_SERVED = [i for i, c in enumerate(CASES) if S.kernel_of(c) is not None]


@pytest.mark.parametrize("i", _SERVED, ids=lambda i: case_id(CASES[i]))
def test_restatement_of_the_kernels_stays_within_every_bar(i):
    """Largest value over all cases, forms and families, in bar units per kernel and output kind (test_largest_restatement_error_per_kernel_and_kind
    prints them):
      rows    plain 0.990  bias 0.977  alpha 0.995  bias_gelu 0.899  bias_res 0.964  res_mod 0.964  bias_gelu_res 0.952  ep1 0.947  ep1.C2 0.532
      frag    plain 0.995  bias 0.971  alpha 0.953  bias_gelu 0.933  bias_res 0.973  res_mod 0.975  bias_gelu_res 0.773  ep1 0.960  ep1.C2 0.655
      staged  plain 0.957  bias 0.970  alpha 0.956  bias_gelu 0.775  bias_res 0.959  res_mod 0.881  bias_gelu_res 0.703  ep1 0.988  ep1.C2 0.597
    (the fused cases counted with the kernel whose prologue they run: rows' bias, ep1 and plain and staged's bias and ep1 come from them;
    the quotient-form SiLU stays inside ep1.C2's bar with a third to spare;
    0.99: one bf16 rounding of a value just above a power of two - a bar of one rounding has no slack)."""
    c = CASES[i]
    for form in c["forms"]:
        for fam in families(c, form):
            p, res, tips = _restatement(i, form, fam)
            U.assert_ok(p, res, f"{case_id(c)} {form} family {fam}")
            for name in S.biteq_outputs(p):
                assert res[name]["unequal"] == 0
            assert tips is None or tips <= S.TIP_CAP, f"{case_id(c)} family {fam}: {tips:.2e} of the activations are tippable: another seed"


def test_largest_restatement_error_per_kernel_and_kind():
    worst = {}
    for i in _SERVED:
        c = CASES[i]
        for form in c["forms"]:
            for fam in families(c, form):
                p, res, _ = _restatement(i, form, fam)
                for name, r in res.items():
                    k = (S.kernel_of(p.c)[0], S.kind(p, name))
                    if r["worst"] > worst.get(k, (-1.0,))[0]:
                        worst[k] = (r["worst"], case_id(c), fam)
    for kern in ("rows", "frag", "staged"):
        print(f"RESTATEMENT {kern}: " + "  ".join(f"{k[1]} {w:.3f} ({cid}, {fam})" for k, (w, cid, fam) in sorted(worst.items()) if k[0] == kern))
    assert all(w < 1.0 for w, _, _ in worst.values()), worst
    for kern in ("rows", "frag", "staged"):      # every form on every kernel
        assert {k[1].split(".")[0] for k in worst if k[0] == kern} == set(S.FORMS), kern


def test_tippable_activations_stay_under_the_cap():
    """At most 1e-3 of the activations of every fused case, form and family (the bars' extra term is meant for a handful per row)."""
    seen = []
    for i, c in enumerate(CASES):
        if S.fused(c):
            for fam in families(c, None):
                p = make_problem(with_form(c, c["forms"][0]), fam)
                S.operands(p)
                seen.append(p.tips[0])
                assert p.tips[0] <= S.TIP_CAP, (case_id(c), fam, p.tips[0])
    print(f"TIPPABLE {min(seen):.2e} .. {max(seen):.2e} over {len(seen)} problems")


# ------------------------------------------------------------------ the reference's norm stage
@pytest.mark.parametrize("cid", ["fused_rows-2x36x576-f0-small", "fused_rows-2x36x4096-f1-zero", "fused_rows-1x36x16384-f1", "fused_staged-15x20x4096-f1-o24-small-zero",
                                 "fused_staged-16x20x4096-f0-o24-small-zero"])
def test_norm_stage_of_the_reference_equals_plain_torch_float64(cid):
    """x rsqrt(mean(x^2) + eps) times w, or times (1 + w), with no rounding; the normalised activations of the reference lie within their own
    rounding bound of it (flavor 0: two roundings, the inner one scaled by |w|; flavor 1: one), and the product of the unrounded activations
    within that bound carried through |B|."""
    c = with_form(CASES[_index(cid)], "bias")
    for fam in ("R", "G"):
        p = make_problem(c, fam)
        g = p.g
        x = torch.as_strided(p.buf["A"], (g["M"], g["K"]), (g["lda"], 1), HEAD).to(F64)
        B = torch.as_strided(p.buf["B"], (g["N"], g["K"]), (g["ldb"], 1), HEAD).to(F64)
        w = p.buf["W"][HEAD:HEAD + g["K"]].to(F64)
        plain = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + S.NORM_EPS) * (w if c["flavor"] == 0 else 1.0 + w)
        o = S.operands(p)
        xn = p.base[0][0]
        bound = plain.abs() * ((2.0 + U.U) * U.U if c["flavor"] == 0 else U.U) * (1.0 + 1e-6)
        assert ((xn - plain).abs() <= bound).all(), (cid, fam, ((xn - plain).abs() / bound.clamp_min(1e-300)).max().item())
        assert ((o["P"][0] - plain @ B.t()).abs() <= bound @ B.abs().t() + 1e-12 * o["absP"][0]).all()
        if c.get("zero_row") is not None:
            assert (xn[c["zero_row"]] == 0).all() and (o["P"][0, c["zero_row"]] == 0).all()
        ref = S.reference(p)["C"]
        want = plain @ B.t() + p.buf["bias"][HEAD:HEAD + g["N"]].to(F64)
        got = torch.as_strided(ref.val, (g["M"], g["N"]), (g["ldc"], 1), HEAD)
        assert ((got - want).abs() <= bound @ B.abs().t() + 1e-12 * (o["absP"][0] + 1.0)).all()


# ------------------------------------------------------------------ detection
def _moved_bits(a, b, dtype):
    return U.output_bits(a.to(dtype)) != U.output_bits(b.to(dtype))


@functools.lru_cache(maxsize=None)
def _detection(i, form, fam):
    return _detect(with_form(CASES[i], form), fam)


def _detect(c, fam):
    """test_gemm_edges_cpu.py's tally with this module's reference -> {(mutation, exact): (affected, share detected, share kept)}"""
    p = make_problem(c, fam)
    true = S.reference(p)
    selector = fam in ("S", "Sb")
    k_true = S.kernel_images(p, S.operands(p)) if selector else None
    out = {}
    for mut in S.mutations(c):
        o = S.operands(p, mut)
        ref_m = S.images(p, U.ref_epilogue(p.g, o), o["touched"], mut)
        k_m = S.kernel_images(p, o, mut) if selector else None
        tally = {True: [0, 0, 0], False: [0, 0, 0]}
        for name, t in true.items():
            m = ref_m[name]
            placed = t.mask != m.mask
            both = t.mask & m.mask
            struct = both & ((t.src != m.src) | m.touched) & t.live
            exact = selector and name in S.biteq_outputs(p)
            n_struct = int(struct.sum())
            if exact:        # every element whose exact value the mutation changes: the kernels' chain must change too (no rounding hides it)
                struct = struct & ~(m.val == t.val)
                moved = _moved_bits(k_true[name].val, k_m[name].val, p.buf[name].dtype)
            else:
                moved = ~((m.val - t.val).abs() <= 2.0 * t.bar)
            if selector and not exact:       # (a saturated GELU hides a selector's step: families R and G answer for GELU / SiLU outputs)
                continue
            tally[exact][0] += int(placed.sum() + struct.sum())
            tally[exact][1] += int(placed.sum() + (struct & moved).sum())
            tally[exact][2] += int(placed.sum()) + n_struct
        for exact, (n_aff, n_det, n_all) in tally.items():
            if n_aff:
                out[(U.mut_name(mut), exact)] = (n_aff, n_det / n_aff, n_aff / n_all)
    return out


_ROUNDINGS = {"plain": 1, "bias": 1, "alpha": 1, "bias_gelu": 2, "bias_res": 2, "res_mod": 2, "ep1": 2, "bias_gelu_res": 3}
_PAD_OF = {"lda_as_k": "a", "ldb_as_k": "b", "ldc_as_n": "c", "ldr_as_n": "r"}


def _asked(c, form, fam, name):
    """Whether family `fam` answers for mutation `name` on this case.  The selector families always do, bit for bit.  Families R and G as in
    test_gemm_edges_cpu.py, with its one exception as worded there (family G, a K-range mutation at K >= 2048 under more than one rounding:
    one Gaussian K-tile in 37 moves ~93 % by 2 bars only), and these, each forced by arithmetic:
      - a K-range mutation that moves less than one part in 37 of K (the smallest share the merged cases ask of R or G: these kernels' own
        granularity is 32 columns, 1 / 192 of K = 6144, where one bf16 rounding, 1 / 256, is already more) is the selector families';
      - bias + GELU + residual is three roundings, which no merged case has: 2 bars are 6 x 2^-8 = 2.3 % of an output of up to 1.4 products, so a
        share under 1 / 16 is the selector families' there; a Gaussian output of size sqrt(K / 16 + 2 K / 64) moves by N(0, f K / 16), and the
        share that moves by less than those 2 bars, 0.8 x 2 bars / sigma = 0.034 / sqrt(f), is under 5 % with room only from f = 1 / 4 on;
      - the normalisation of the fused cases takes the ramp's row factor away (rows_swapped: family G answers), shifted norm weights move a ramp
        output by 0.3 / sqrt(K) of its size (family G answers), and a displaced read by a pad of 12 or 24 meets the ramp's period of 3 again
        (families S, Sb, G answer; at the other pads family R keeps the merged floor of one half).
    test_every_off_by_one_is_detected asserts that every mutation of every case is answered by some family."""
    base = name.split(":")[0]
    if fam in ("S", "Sb"):
        return True
    if base in S.K_RANGE:
        f = S.k_share(c, (base,), S.kernel_of(c))
        if f < 1.0 / 37.0 or (_ROUNDINGS[form] == 3 and f < (1.0 / 16.0 if fam == "R" else 1.0 / 4.0)):
            return False
        return not (fam == "G" and c["K"] >= 2048 and form not in ("plain", "bias", "alpha"))
    if fam == "R" and (base == "norm_w_shift" or (S.fused(c) and base == "rows_swapped")):
        return False
    if fam == "R" and name in _PAD_OF and c["pad"][_PAD_OF[name]] % 3 == 0:
        return False
    return True


def _enough(name, share, fam, exact):
    if fam == "R" and name in S.DISPLACED:
        return share >= 0.5
    return share >= (0.95 if fam == "G" else 1.0)


def _failures(c):
    """every (form, family, mutation) of case `c` that is not detected as _asked / _enough want, and every mutation of the case that no
    family answers on any of its forms (every case has a form without a transcendental, where the selector families answer bit for bit)"""
    bad, answered, wanted = [], set(), set()
    for form in c["forms"]:
        cf = with_form(c, form)
        wanted |= {U.mut_name(m) for m in S.mutations(cf)}
        for fam in families(c, form):
            for (name, exact), (n, share, kept) in _detect(cf, fam).items():
                if not _asked(cf, form, fam, name):
                    continue
                answered.add(name)
                if kept < 0.5:
                    bad.append(f"{case_id(c)} {form} family {fam}: mutation {name} changes only {kept:.3f} of the elements it touches")
                if not _enough(name, share, fam, exact):
                    bad.append(f"{case_id(c)} {form} family {fam}: mutation {name} detected in {share:.4f} of {n} affected elements")
    bad += [f"{case_id(c)}: no family answers for mutation {name} on any form" for name in sorted(wanted - answered)]
    return bad


_MUTATED = [i for i, c in enumerate(CASES) if S.kernel_of(c) is not None and c["group"] != "boundary"]


@pytest.mark.parametrize("i", _MUTATED, ids=lambda i: case_id(CASES[i]))
def test_every_off_by_one_is_detected(i):
    """As test_gemm_edges_cpu.py::test_every_off_by_one_is_detected: families S / Sb bit for bit wherever the exact value changes, family R every
    affected element by more than 2 bars, family G at least 95 % of them, per case (_asked: which family answers for what, and why); and every
    mutation of the case is answered by at least one family."""
    bad = _failures(CASES[i])
    assert not bad, "\n".join(bad)


def test_every_mutation_is_covered_by_some_case():
    covered, pooled = {}, {}
    for i in _MUTATED:
        c = CASES[i]
        for form in c["forms"]:
            for fam in families(c, form):
                for (name, _), (n, share, _) in _detection(i, form, fam).items():
                    if _asked(with_form(c, form), form, fam, name):
                        covered.setdefault(name, set()).add(fam)
                        if fam == "G":
                            t = pooled.setdefault(name, [0, 0])
                            t[0] += n
                            t[1] += round(n * share)
    for name, (n, det) in pooled.items():
        assert det >= 0.95 * n, f"family G: mutation {name} detected on {det} of {n} affected elements of all cases"
    print(f"MUTATIONS covered {len(covered)} of {len(S.ALL_MUTATIONS)}: " + "  ".join(f"{k} {''.join(sorted(v))}" for k, v in sorted(covered.items())))
    assert set(covered) == set(S.ALL_MUTATIONS), set(S.ALL_MUTATIONS) ^ set(covered)
    for name, fams in covered.items():
        if name.split(":")[0] in S.NORM_MUTS:
            assert "G" in fams and ("R" in fams or name == "norm_w_shift:8"), (name, fams)
        else:
            assert "G" in fams and fams & {"S", "Sb"} and ("R" in fams or name in S.DISPLACED), (name, fams)


@pytest.mark.parametrize("cid,form,fam,names", [("frag-3x4x64", None, "S", ("cols_past_n", "clamp_written")), ("frag-15x20x512", None, "Sb", ("wave_twice",)),
                                                ("staged-17x16388x2048", "bias_res", "S", ("tile1_as_tile0",))])
def test_three_kernel_mutants_are_caught_by_named_cases(cid, form, fam, names):
    i = _index(cid)
    det = _detection(i, form or CASES[i]["forms"][0], fam)
    for name in names:
        assert det[(name, True)][1] == 1.0 and det[(name, True)][0] > 0, (cid, name, det.get((name, True)))


# ------------------------------------------------------------------ coverage
def test_cases_cover_what_the_dispatcher_can_launch():
    served = {}
    for c in CASES:
        for form in c["forms"]:
            s = S.kernel_of(with_form(c, form))
            if s is not None:
                served.setdefault(s, []).append((with_form(c, form), form))
    kernels = set(served)
    assert {s for s in kernels if s[0] != "rows"} == {("frag", 1), ("frag", 2)} | {("staged", t, mt) for t in (1, 2) for mt in (1, 2, 4)}
    rows = {s for s in kernels if s[0] == "rows"}
    assert {s[3] for s in rows} == {8, 16, 32} and {s[2] for s in rows if s[1] == 1} == {2, 4, 8, 16} and ("rows", 2, 4, 8) in rows and ("rows", 2, 4, 16) in rows and ("rows", 2, 4, 32) in rows
    assert {(s[2], s[3]) for s in rows if s[1] == 1} >= {(r, rb) for r in (2, 4, 8) for rb in (8, 16, 32)} | {(16, 16), (16, 32)}
    for rb in (8, 16, 32):      # a ragged last block, with and without SwiGLU's full blocks
        assert any(c["N"] % rb for s, v in served.items() if s[0] == "rows" and s[3] == rb for c, _ in v), rb
    assert S.served_by(1, 4, 64, 1, 0, False, 256) == ("rows", 1, 2, 16)         # (one block either way: no balance gain, the larger block stays)
    assert [S.rows_per_block(n, False, 256) for n in (12, 36, 100, S.RB16_N, S.RB32_N)] == [8, 8, 8, 16, 32]
    shapes = lambda kern: [S.loop_shape(s, c["K"]) for s, v in served.items() if s[0] == kern for c, _ in v]
    fr = shapes("frag")
    assert {d["span"] for d in fr} == {True, False} and any(d["idle"] == 6 for d in fr)
    for un in (8, 4):           # both unroll widths: unrolled trips with and without a remainder, and the remainder loop alone
        mine = [d for d in fr if d["un"] == un]
        waves = {w for d in mine for w in d["waves"]}
        assert any(t >= 1 and r == 0 for t, r in waves), un                  # a wave of whole unrolled trips, no remainder
        assert any(t >= 1 and r >= 1 for t, r in waves), un                  # a wave of trips and a remainder
        assert any(all(t == 0 for t, _ in d["waves"]) for d in mine), un     # a case of the remainder loop alone
    assert any(d["un"] == 4 and (2, 1) in d["waves"] for d in fr) and any(d["un"] == 8 and (1, 1) in d["waves"] for d in fr)
    assert {d["nst"] for d in shapes("staged")} == {1, 2, 3}
    rw = shapes("rows")
    assert any(d["steps"] == 1 and d["partial"] for d in rw) and any(d["steps"] == 1 and not d["partial"] for d in rw)
    assert any(d["steps"] == 2 and d["partial"] for d in rw) and any(d["q1_used"] and d["guard_hit"] for d in rw) and any(d["second_trip"] for d in rw)
    want = {"rows": ((1, 2), (64, 512, 576, 4160, 2368), (4, 12, 36, 100, 32, 96, S.RB16_N, S.RB32_N)),
            "frag": ((1, 2, 3, 15, 16), (64, 192, 512, 576, 2112, 2304, 2048), (4, 12, 16, 20, 36, 32, 96, 16388, 16404)),
            "staged": ((3, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64), (2048, 4096, 6144), (4, 20, 36, 32, 96, 16388))}
    for kern, (Ms, Ks, Ns) in want.items():
        mine = [c for s, v in served.items() if s[0] == kern for c, _ in v if not S.fused(c)]
        assert {c["M"] for c in mine} >= set(Ms) and {c["K"] for c in mine} >= set(Ks) and {c["N"] for c in mine} >= set(Ns), kern
        assert {f for s, v in served.items() if s[0] == kern for c, f in v if not S.fused(c)} == set(S.FORMS), kern
    ld = [c for c in CASES if c["group"] == "ld"]
    assert {S.kernel_of(c)[0] for c in ld} == {"rows", "frag", "staged"} and {c["pad"]["a"] for c in ld} == {8, 24} and {c["pad"]["c"] for c in ld} == {4, 12}
    assert {c["pad"]["r"] for c in ld if "r" in c["pad"]} == {4, 12} and {(S.kernel_of(c)[0], c["pad"]["c2"]) for c in ld if "c2" in c["pad"]} == {(k, n) for k in ("rows", "frag", "staged") for n in (4, 12)}
    # the boundaries: either side of M = 64 at K % 2048 == 0, of M = 16 elsewhere, and option 4 = 0
    b = {case_id(c): S.kernel_of(c) for c in CASES if c["group"] == "boundary"}
    assert b == {"boundary-64x20x2048": ("staged", 1, 4), "boundary-65x20x2048": None, "boundary-16x20x2112": ("frag", 1), "boundary-17x20x2112": None,
                 "boundary-1x36x576-o4=0": None}
    # the fused entry point: both flavors on both prologues, every K of the row prologue, the LDS limit itself, the fallback, rows in flight
    fz = [(c, S.fused_by(c["M"], c["N"], c["K"], 1, c.get("opt24", 0), c.get("opt26", 0), c["forms"] == ("ep1",), 256)) for c in CASES if S.fused(c)]
    assert {(code, c["flavor"]) for c, (code, _) in fz} >= {(201, 0), (201, 1), (202, 0), (202, 1)}
    assert {(c["M"], c["K"]) for c, (code, _) in fz if code == 201} >= {(m, k) for m in (1, 2) for k in (64, 576, 4096, 4160, 8192, 16384)}
    assert [code for c, (code, _) in fz if c["K"] == 16448] == [200]
    assert {s[2] for c, (code, s) in fz if code == 201 and c["M"] == 1} == {2, 4, 8, 16}
    assert {(c["M"], c["K"]) for c, (code, _) in fz if code == 202} == {(m, k) for m in (3, 15, 16) for k in (2048, 4096)}
    assert {c["N"] for c, (code, _) in fz if code == 202} == {20, 96, 16388} and {c["N"] for c, (code, _) in fz if code == 201} == {36, 96, S.RB16_N}
    assert any(c.get("small_row") is not None for c, _ in fz) and any(c.get("zero_row") is not None for c, _ in fz)
