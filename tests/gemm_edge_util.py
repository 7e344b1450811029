"""float64 reference, per-element bars, edge-loud inputs, off-by-one mutations and the case list for the bf16 tiled GEMM
(uvx_gemm / uvx_gemm_splitk on bf16 operands: ultravox_amd/csrc/gemm.hip).

Used by test_gemm_edges_cpu.py (which proves this harness on the CPU) and test_gemm_edges_gpu.py (which holds the kernels to it).
Everything here is plain torch and runs on whichever device the problem's buffers live on.

A Problem is a set of FLAT buffers plus the integers of a uvx_gemm_desc_t (offsets, leading dimensions, batch strides).  The
reference reads every operand through the descriptor's index arithmetic - A_z[m, k] = bufA[oA + z sA + m lda + k] and so on - and
lays its results into an IMAGE of each output buffer: value, bar and a written mask per buffer element.  Whatever the mask leaves out
(padding columns of ldc / ldc2, rows after M, the gaps between batch slabs, the space before and after the operand) holds a canary bit
pattern that the comparison wants back bit for bit.  A mutation is the same reference with ONE piece of that arithmetic off by one.

Formula (include/uvx.h): C = act(alpha A . B^T + bias) + residual[m % res_mod] (+ C for accumulate); act 2: C = alpha A . B^T + bias, C2 =
gelu(C); act 3: C = (alpha A . B^T) gelu'(C2); epilogue 1: C = gate|up = alpha A . B^T in 16-column blocks, C2 = silu(gate) up; epilogue 2:
d = alpha A . B^T [M, N], C2 = gate|up [M, 2N] (input), C [M, 2N] = d up silu'(gate) | d silu(gate).

bf16 rounding points of the kernels (gemm.hip; u = 2^-8, the bf16 unit roundoff; accumulation is f32 throughout):
  bf16 output   t = round(acc alpha + bias) (store_tile :234 staged, :498 wide, :535 fragment layout; store_tile32 :604; the split-K reduce
                :2058); act 1: t = round(gelu_fast(t)) (:235, :499, :538, :605, :2059); residual: round(t + r), the sum in f32 (:257-260, :510,
                :565, :621-624, :2068).  So plain / bias / alpha: 1 rounding, bias + GELU: 2, bias + residual: 2, all three: 3.
  f32 output    nothing is rounded to bf16 (:534-573; the staged form :334 carries no epilogue).
  act 2         C = round(acc alpha + bias) (:234 / :535), C2 = round(gelu_fast(C)) (:275 / :547).
  act 3         round(acc alpha) (:234 / :535), then round(that * gelu_fast_grad(C2)) (mul_gelu_grad2 :107 / :552, :565).
  epilogue 1    gate, up = round(acc alpha) (:300-301, :367-368, :2034-2035); C2 = round(round(silu(gate)) * up) (:301, :370-374, :2039-2041).
  epilogue 2    d = round(acc alpha) (:166, :440); d up = round(d * round(gate sigmoid(gate))) (:193, :444); d gate = round(d up' sigmoid' ..)
                (:193, :445), up' = the bf16 input.
Every bar below is carried through these steps as an absolute error bound e per element: the f32 accumulation contributes
(2 sqrt(K) + 4) 2^-24 (sum of |terms|) - the form of _gemm_bar in test_f32_kernels_gpu.py -, a rounding of a value y with incoming error e adds
u (|y| + e), GELU passes e on with its Lipschitz constant 1.13 and adds 2^-21 (|x| + e) for gelu_fast (Abramowitz-Stegun 7.1.26, |eps| <= 1.5e-7
on erfc, hardware rcp / exp2 at one ulp each), SiLU 1.1 e + |silu| (|g| + 4) 2^-23 (the f32 exp argument), a product the usual two cross terms.

`restatement` repeats the kernels' arithmetic: f32 accumulation in K order, one step per MFMA (32 columns of K; 16 for the 32 x 32 x 16 kernels
of variants 61 / 62; split-K: f32 partial sums per slab [z nk / s, (z + 1) nk / s), added in slab order), gelu_fast / gelu_fast_grad / the
sigmoid in f32, and a bf16 rounding at exactly the points above.  Its largest error over every case and family of test_gemm_edges_gpu.py, in bar
units per output kind, is measured by test_gemm_edges_cpu.py::test_restatement_of_the_kernels_stays_within_every_bar (figures in its docstring).

Input families (all bf16-representable; make_problem):
  S   selector: A rows are zero except A[m, k(m)] = s(m), k(m) = (29 m + 11 z) mod K (29 is coprime to 64 and to every K used: M >= K rows
      visit every K position), s(m) in {+-0.5, +-1, +-2}; B dense, +-{0.5 .. 2.5} with the magnitude by (k + 3 (n mod 7) + z) mod 5 and the sign by n mod 7.
      C = s(m) B[n, k(m)] exactly whatever the summation order; bias in {4, 4.5 .. 7}, residual / accumulate values +-{0.5 .. 2.5} (both x alpha):
      every value is a small multiple of 1/4 (1/16 under alpha = 0.25), so every f32 sum AND every bf16 rounding of the plain epilogues is exact and
      two different inputs never round to the same output.
      BIT-EQUAL forms (asserted on the GPU): every output without a transcendental - plain, bias, bias + residual, res_mod, alpha, f32 output,
      accumulate, C of act 2, C of epilogue 1, all of them split or unsplit, NT or NN.  GELU / SiLU outputs are held to their bars.
  Sb  the mirror: one-hot B rows, dense patterned A - the A-side indexing; the only selector family where A rows overlap (lda < K).
  R   ramp: dense positive-biased entries, uniform(0.5, 1) x a row / column factor in (1, 1.25, 1.5) x a K-tile factor in (1, 1.25) x a batch
      factor; bias, residual and accumulate values in proportion to the product (factors 0.08 / 0.16 / 0.24 by column and row, the residual x 1 / 2 / 3 by batch): neighbours differ
      by many bars and nothing cancels.
  G   Gaussian x 0.5 (the family of the existing tests); bias and residual Gaussian x max(1, sqrt(K) / 8).
"""
import math

import torch

F64 = torch.float64
U = 2.0 ** -8            # bf16 unit roundoff
EPS = 2.0 ** -24         # f32 unit roundoff
GELU_LIP, GELU_APPROX = 1.13, 2.0 ** -21
CANARY16 = 0x7FA5        # a bf16 NaN
CANARY32 = 0x7FC5A5A5    # an f32 NaN
HEAD = 64                # canary elements in front of every operand
FORMS = ("plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "f32", "f32_acc", "act2", "act3", "ep1", "ep2")
BITEQ_FORMS = ("plain", "bias", "bias_res", "res_mod", "alpha", "f32", "f32_acc")       # + C of act2 / ep1
BM = {0: 128, 11: 256, 15: 160, 16: 192, 17: 128, 18: 160, 19: 128, 31: 256, 32: 192, 33: 160, 34: 128, 59: 160, 60: 128, 61: 256, 62: 128}


def bf(x):
    """Round float64 to bf16 (through f32, as f2bf sees an f32 value) and back."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def f32r(x):
    return x.to(torch.float32).to(F64)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _erfc_poly32(x):
    """poly(t) exp(-x^2 / 2) of gelu_fast / gelu_fast_grad (common.h) in f32 -> (poly * e, e)"""
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = torch.exp2(-z * z * 1.4426950408889634)
    return poly * e, e


def gelu_fast(x):
    x32 = x.to(torch.float32)
    pe, _ = _erfc_poly32(x32)
    return (0.5 * x32 * torch.where(x32 < 0, pe, 2.0 - pe)).to(F64)


def gelu_fast_grad(x):
    x32 = x.to(torch.float32)
    pe, e = _erfc_poly32(x32)
    hp = 0.5 * pe
    return (torch.where(x32 < 0, hp, 1.0 - hp) + x32 * (0.3989422804014327 * e)).to(F64)


# ------------------------------------------------------------------ geometry
def geometry(c):
    """The integers of the descriptor and the buffer sizes of a case (elements).  Layouts:
    plain   separate slabs per batch with a canary gap; `shared_b` / `shared_r`: stride_b / stride_r = 0
    conv    the conv stems: rows of A overlap (lda < K), shared B
    group   the grouped positional conv: rows of A overlap (lda = K / taps), own B per batch, stride_c = N columns inside one ldc, f32 output
    ksplit  the LM-head weight gradient: stride_a = stride_b = K along the rows of [.., batch K], f32 output into separate slabs"""
    M, N, K, Z = c["M"], c["N"], c["K"], c.get("batch", 1)
    form, layout, pad = c["form"], c.get("layout", "plain"), c.get("pad", {})
    nn = bool(c.get("b_kn"))
    g = dict(M=M, N=N, K=K, Z=Z, nn=nn, form=form, layout=layout)
    g["Nc"] = 2 * N if form == "ep2" else N
    g["W2"] = {"act2": N, "act3": N, "ep1": N // 2, "ep2": 2 * N}.get(form, 0)
    g["res_mod"] = c.get("res_mod", 7 if form == "res_mod" else 0)
    has_res = form in ("bias_res", "res_mod") or c.get("residual", False)
    g["Mr"] = (g["res_mod"] or M) if has_res else 0
    g["has_bias"] = form in ("bias", "bias_gelu", "bias_res", "res_mod", "alpha", "act2") or c.get("bias", False)
    g["act"] = {"bias_gelu": 1, "act2": 2, "act3": 3}.get(form, 1 if c.get("gelu") else 0)
    g["epi"] = {"ep1": 1, "ep2": 2}.get(form, 0)
    g["out_f32"] = form in ("f32", "f32_acc") or bool(c.get("out_f32"))
    g["accumulate"] = form == "f32_acc"
    # (epilogue 1 at K = 64 x 37: alpha = 1/8 keeps gate and up where silu(gate) up differs from silu(up) gate in family G too)
    g["alpha"] = 0.25 if form == "alpha" else 0.125 if (form == "ep1" and K >= 2048) else c.get("alpha", 1.0)
    if layout == "conv":
        g["lda"] = c["lda"]
    elif layout == "group":
        g["lda"] = K // c["taps"]
    elif layout == "ksplit":
        g["lda"] = Z * K + pad.get("a", 0)
    else:
        g["lda"] = K + pad.get("a", 0)
    g["ldb"] = (Z * K + pad.get("b", 0)) if layout == "ksplit" else ((N if nn else K) + pad.get("b", 0))
    g["ldc"] = (Z * N if layout == "group" else g["Nc"]) + pad.get("c", 0)
    g["ldr"] = N + pad.get("r", 0)
    g["ldc2"] = g["W2"] + pad.get("c2", 0)
    gap = 24                                             # canary elements between batch slabs (a multiple of 8)
    a_rows = (M - 1) * g["lda"] + K                      # extent of one batch's A
    if layout == "ksplit":
        g["sA"], g["sB"] = K, K
    else:
        g["sA"] = -(-(a_rows + g["lda"] + gap) // 8) * 8 if Z > 1 else 0
        g["sB"] = 0 if (c.get("shared_b") or layout == "conv" or Z == 1) else (K if nn else N) * g["ldb"] + gap
    g["sC"] = N if layout == "group" else (M * g["ldc"] + gap if Z > 1 else 0)
    g["sR"] = 0 if (c.get("shared_r") or Z == 1 or not has_res) else g["Mr"] * g["ldr"] + gap
    ext = lambda s, ld, rows, cols: HEAD + s * (Z - 1) + ld * (rows - 1) + cols
    tail = lambda ld: 2 * ld + 72                        # canary rows after the operand
    g["nA"] = ext(g["sA"], g["lda"], M, K) + tail(g["lda"])
    g["nB"] = ext(g["sB"], g["ldb"], K if nn else N, N if nn else K) + tail(g["ldb"])
    g["nC"] = ext(g["sC"], g["ldc"], M, g["Nc"]) + tail(g["ldc"])
    g["nR"] = ext(g["sR"], g["ldr"], g["Mr"], N) + tail(g["ldr"]) if has_res else 0
    g["nC2"] = ext(0, g["ldc2"], M, g["W2"]) + tail(g["ldc2"]) if g["W2"] else 0
    g["nbias"] = HEAD + N + 72 if g["has_bias"] else 0
    return g


def _ar(n, dev):
    return torch.arange(n, device=dev)


def _idx(o, s, ld, Z, rows, cols, dev):
    """flat index [Z, rows, cols] of element (z, r, c)"""
    return o + s * _ar(Z, dev)[:, None, None] + ld * _ar(rows, dev)[None, :, None] + _ar(cols, dev)[None, None, :]


# ------------------------------------------------------------------ inputs
def _pattern(Z, R, Cn, shift=0):
    """dense values of family S / Sb: +-{0.5 .. 2.5}, the magnitude by (c + 3 r' + z) mod 5, the sign by r' = r mod 7 - with the selector's sign,
    which alternates too, neighbouring rows and columns of C have opposite signs.  Steps of 0.5: every sum of the epilogue is exact."""
    z, r, c = _ar(Z, "cpu")[:, None, None], _ar(R, "cpu")[None, :, None], _ar(Cn, "cpu")[None, None, :]
    r = r % 7               # (period 7: a tail launch 16384 rows further on reads another class)
    return (1.0 - 2.0 * (r % 2).to(F64)) * (0.5 + 0.5 * ((c + 3 * r + z + shift) % 5).to(F64))


def _onehot(Z, R, Cn):
    z, r = _ar(Z, "cpu")[:, None], _ar(R, "cpu")[None, :]
    k = (29 * r + 11 * z) % Cn
    s = torch.tensor([1.0, -0.5, 2.0, -1.0, 0.5, -2.0], dtype=F64)[(r + z) % 6]
    out = torch.zeros(Z, R, Cn, dtype=F64)
    out.scatter_(2, k[..., None], s[..., None])
    return out


def _ramp(Z, R, Cn, gen, tiles):
    z, r, c = _ar(Z, "cpu")[:, None, None], _ar(R, "cpu")[None, :, None], _ar(Cn, "cpu")[None, None, :]
    v = torch.rand(Z, R, Cn, generator=gen, dtype=F64) * 0.5 + 0.5
    v = v * (1.0 + 0.25 * (r % 3).to(F64)) * (1.0 + 0.25 * (z % 3).to(F64))
    return v * (1.0 + 0.25 * ((c // 64) % 2).to(F64)) if (tiles and Cn < 2048) else v      # (37 K-tiles: equal shares, so that one of them still shows)


def _cyc(i, half=False):
    return torch.tensor([0.08, 0.16, 0.24], dtype=F64)[i % 3] * (0.5 if half else 1.0)


def make_problem(c, family, device="cpu"):
    """-> Problem: canary-filled buffers with the operands of one input family laid in through the descriptor (drawn on the CPU from a
    fixed seed: the same values on every device)."""
    g = geometry(c)
    M, N, K, Z, nn, form = g["M"], g["N"], g["K"], g["Z"], g["nn"], g["form"]
    gen = torch.Generator().manual_seed(c["seed"] + 1000003 * ("S", "Sb", "R", "G").index(family))
    overlap = g["lda"] < K
    assert not (overlap and family == "S"), "family S needs rows of A that do not overlap"
    a_shape = (Z, 1, (M - 1) * g["lda"] + K) if overlap else (Z, M, K)       # overlapping rows: one flat run per batch
    p0 = K * 0.75 ** 2 * 1.25 * 1.25 * (1.125 if K < 2048 else 1.0) * abs(g["alpha"])              # family R: the product's size
    if overlap:
        p0 = K * 0.75 ** 2 * 1.25 * (7.0 / 3.0) * 1.25 * abs(g["alpha"])    # (overlapping rows: chunk factors 1 / 4 / 2 in place of the row and K-tile factors)
    sb = max(1.0, math.sqrt(K) / 8.0)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    mi, ni = _ar(max(M, g["Mr"], 1), "cpu")[:, None], _ar(N, "cpu")[None, :]
    if family == "S":
        A, B = _onehot(*a_shape), _pattern(Z, N, K)
    elif family == "Sb":
        A, B = _pattern(*a_shape, shift=5), _onehot(Z, N, K)
    elif family == "R":
        A, B = _ramp(*a_shape, gen, True), _ramp(Z, N, K, gen, False)
        if overlap:  # overlapping rows: the factor goes by the lda-sized chunk, so that neighbouring windows still differ by several per cent
            chunk = (_ar(a_shape[2], "cpu") // g["lda"]) % 3
            A = (0.5 + 0.5 * torch.rand(*a_shape, generator=gen, dtype=F64)) * torch.tensor([1.0, 4.0, 2.0], dtype=F64)[chunk] * (1.0 + 0.25 * (_ar(Z, "cpu") % 3).to(F64))[:, None, None]
        if form == "ep1":  # gate ~ 0.25 and up ~ 1, where silu(gate) up is far from silu(up) gate (for large values both are gate up)
            A = A * 2.0 ** -round(math.log2(p0))
            B = B * (0.25 + 0.75 * ((_ar(N, "cpu") // 16) % 2).to(F64))[None, :, None]
    else:
        A, B = 0.5 * rn(*a_shape), 0.5 * rn(Z, N, K)
    if family in ("S", "Sb"):
        bias = (4.0 + 0.5 * ((3 * ni[0]) % 7).to(F64)) * abs(g["alpha"])
        small = (0.5 + 0.5 * ((3 * mi + ni) % 5).to(F64)) * (1.0 - 2.0 * ((mi + ni) % 2).to(F64)) * abs(g["alpha"])      # steps of 0.5: no rounding hides one
        res, c0 = small[: max(g["Mr"], 1)], small[:M].flip(1)
        w2 = _ar(max(g["W2"], 1), "cpu")[None, :]
        if form == "ep2":  # gate in {0.5 .. 2}, up in {2.5 .. 4}: swapped or shifted reads change every result by several per cent
            x2 = 0.5 + 0.5 * ((mi[:M] + w2) % 4).to(F64) + 2.0 * ((w2 // 16) % 2).to(F64)
        else:                   # six pre-activations whose GELU derivatives lie >= 0.045 apart
            x2 = torch.tensor([-1.5, 0.25, -1.0, 0.75, -0.5, 1.5], dtype=F64)[(3 * mi[:M] + w2) % 6]
    elif family == "R":
        bias = p0 * _cyc(ni[0], K >= 2048) * (1.0 + 0.05 * torch.rand(N, generator=gen, dtype=F64))
        res = p0 * (_cyc(ni, K >= 2048) * (1.0 + 0.5 * (mi % 3).to(F64)))[: max(g["Mr"], 1)] * (1.0 + 0.05 * torch.rand(max(g["Mr"], 1), N, generator=gen, dtype=F64))
        c0 = p0 * _cyc(mi + 2 * ni)[:M]
        w2 = _ar(max(g["W2"], 1), "cpu")[None, :]
        x2 = 0.6 + 0.05 * torch.rand(M, max(g["W2"], 1), generator=gen, dtype=F64) + (2.0 * ((w2 // 16) % 2).to(F64) + 0.5 * (4 - (w2 // 32) % 5).to(F64) if form == "ep2" else 0.5 * (mi[:M] % 2).to(F64))
    else:
        sb = sb * abs(g["alpha"])
        bias, res, c0, x2 = sb * rn(N), sb * rn(max(g["Mr"], 1), N), 3.0 * rn(M, N), rn(M, max(g["W2"], 1))
    buf = {}

    def lay(name, n, dtype, parts):
        if not n:
            return
        flat = torch.full((n,), CANARY32 if dtype == torch.float32 else CANARY16, dtype=torch.int32 if dtype == torch.float32 else torch.int16).view(dtype)
        for idx, val in parts:
            flat[idx.reshape(-1)] = val.reshape(-1).to(dtype)
        buf[name] = flat.to(device)

    if overlap:
        a_idx = HEAD + g["sA"] * _ar(Z, "cpu")[:, None] + _ar(a_shape[2], "cpu")[None, :]
    else:
        a_idx = _idx(HEAD, g["sA"], g["lda"], Z, M, K, "cpu")
    lay("A", g["nA"], torch.bfloat16, [(a_idx, A)])
    b_idx = _idx(HEAD, g["sB"], g["ldb"], Z, K, N, "cpu").transpose(1, 2) if nn else _idx(HEAD, g["sB"], g["ldb"], Z, N, K, "cpu")
    zb = 1 if g["sB"] == 0 else Z                    # a shared operand is laid once (one writer per element: the same buffers on every run)
    lay("B", g["nB"], torch.bfloat16, [(b_idx[:zb], B[:zb])])
    lay("bias", g["nbias"], torch.bfloat16, [(HEAD + _ar(N, "cpu"), bias)])
    if g["Mr"]:
        res_z = sb * rn(Z, g["Mr"], N) if family == "G" else res[None] * (1.0 + _ar(Z, "cpu")[:, None, None])      # (x 1, 2, 3 by batch: exact)
        lay("R", g["nR"], torch.bfloat16, [(_idx(HEAD, g["sR"], g["ldr"], Z, g["Mr"], N, "cpu"), res_z)])
    out_dt = torch.float32 if g["out_f32"] else torch.bfloat16
    lay("C", g["nC"], out_dt, [(_idx(HEAD, g["sC"], g["ldc"], Z, M, N, "cpu"), c0[None].expand(Z, -1, -1).to(torch.bfloat16).to(F64))] if g["accumulate"] else [])
    if g["W2"]:
        lay("C2", g["nC2"], torch.bfloat16, [(_idx(HEAD, 0, g["ldc2"], 1, M, g["W2"], "cpu"), x2[None])] if form in ("act3", "ep2") else [])
    return Problem(c, family, g, buf)


class Problem:
    def __init__(self, c, family, g, buf):
        self.c, self.family, self.g, self.buf = c, family, g, buf
        self.base = None
        self.dev = buf["A"].device if buf else None

    def to(self, device):
        return Problem(self.c, self.family, self.g, {k: v.to(device) for k, v in self.buf.items()})

    def outputs(self):
        return ("C", "C2") if self.g["form"] in ("act2", "ep1") else ("C",)

    def read(self, name, idx):
        """the buffer's values at `idx`; NaN where a (mutated) index leaves the buffer"""
        b = self.buf[name]
        inside = (idx >= 0) & (idx < b.numel())
        return torch.where(inside, b[idx.clamp(0, b.numel() - 1)].to(F64), torch.full((), float("nan"), dtype=F64, device=b.device))


# ------------------------------------------------------------------ mutations
def mutations(c):
    """Every off-by-one that has a meaning on this case (the affected set may still be empty: the CPU test counts coverage)."""
    g = geometry(c)
    M, N, K, Z = g["M"], g["N"], g["K"], g["Z"]
    out = [("k_first_drop",), ("k_first_twice",), ("k_last_drop",), ("k_last_twice",), ("last_row_skip",), ("last_cols_skip",), ("row_past_m",), ("cols_past_n",)]
    s = c.get("split", 0)
    if s > 1 and K // 64 >= s:
        out += [("slab_omit",), ("slab_twice",)]
        if (K // 64) % s:
            out += [("split_short",), ("split_long",)]
    out += [("seam_row", bm) for bm in (128, 160, 192, 256) if M > bm] + [("seam_col", n) for n in (128, 256) if N > n]
    if g["has_bias"]:
        out.append(("bias_shift",))
    if c.get("n_main"):
        out += [("tail_off", x) for x in ("B", "C") + (("bias",) if g["has_bias"] else ()) + (("R",) if g["Mr"] else ()) + (("C2",) if g["W2"] else ())]
    if g["res_mod"]:
        out.append(("res_row_m",))
    if g["Mr"] and g["ldr"] != N:
        out.append(("ldr_as_n",))
    if g["lda"] != K:
        out.append(("lda_as_k",))
    if g["ldb"] != (N if g["nn"] else K):
        out.append(("ldb_as_k",))
    if g["ldc"] != g["Nc"]:
        out.append(("ldc_as_n",))
    if Z > 1:
        out += [("batch0", x) for x in ("a", "b", "c") + (("r",) if g["Mr"] else ()) if g["s" + x.upper()] != 0]
    if g["alpha"] != 1.0 and g["has_bias"]:
        out.append(("alpha_after_bias",))
    if g["accumulate"]:
        out.append(("acc_dropped",))
    if g["epi"]:
        out.append(("gu_swapped",))
    if g["form"] in ("act3", "ep2") and g["ldc2"] != g["ldc"]:
        out.append(("c2_ldc",))
    if g["nn"]:
        out.append(("nn_as_nk",))
    return out


# Mutations that read or write at an arbitrary displacement (a leading dimension taken as the width, the NN operand read as NT, a tail launch
# without its column offset).  The ramp
# of family R has period 3 in rows and columns, so one displaced read in three meets its own class: these belong to the selector families
# (every changed element) and to family G (95 %); family R answers for the neighbour mutations - seams, K-tiles, slabs, batches, shifts by one.
DISPLACED = ("lda_as_k", "ldb_as_k", "ldc_as_n", "ldr_as_n", "c2_ldc", "nn_as_nk", "tail_off:B", "tail_off:C", "tail_off:bias", "tail_off:R", "tail_off:C2")
K_RANGE = ("k_first_drop", "k_first_twice", "k_last_drop", "k_last_twice", "slab_omit", "slab_twice", "split_short", "split_long")
ALL_MUTATIONS = ("k_first_drop", "k_first_twice", "k_last_drop", "k_last_twice", "last_row_skip", "last_cols_skip", "row_past_m", "cols_past_n",
                 "slab_omit", "slab_twice", "split_short", "split_long", "seam_row:128", "seam_row:160", "seam_row:192", "seam_row:256",
                 "seam_col:128", "seam_col:256", "bias_shift", "tail_off:B", "tail_off:C", "tail_off:bias", "tail_off:R", "tail_off:C2", "res_row_m",
                 "ldr_as_n", "lda_as_k", "ldb_as_k", "ldc_as_n", "batch0:a", "batch0:b", "batch0:c", "batch0:r", "alpha_after_bias", "acc_dropped",
                 "gu_swapped", "c2_ldc", "nn_as_nk")


def mut_name(mut):
    return ":".join(str(x) for x in mut)


def _ktile_weights(p, mut):
    """how often each K-tile enters the sum under `mut` (None: every tile once)"""
    nk, s = p.g["K"] // 64, p.c.get("split", 0)
    w = torch.ones(nk, dtype=F64, device=p.dev)
    name = mut[0] if mut else None
    if name == "k_first_drop":
        w[0] = 0
    elif name == "k_first_twice":
        w[0] = 2
    elif name == "k_last_drop":
        w[-1] = 0
    elif name == "k_last_twice":
        w[-1] = 2
    elif name in ("slab_omit", "slab_twice", "split_short", "split_long"):
        w.zero_()
        for z in range(s):
            kb, ke = z * nk // s, (z + 1) * nk // s
            if name == "split_short":
                ke = kb + nk // s
            if name == "split_long":
                ke = min(nk, kb + -(-nk // s))
            times = 0 if (name == "slab_omit" and z == s - 1) else 2 if (name == "slab_twice" and z == 0) else 1
            w[kb:ke] += times
    else:
        return None
    return w


def _perm_gu(n, dev):
    """column permutation that swaps each 16-column gate block with its up block"""
    i = _ar(n, dev)
    return i + 16 - 32 * ((i // 16) % 2)


# ------------------------------------------------------------------ operands as the (possibly mutated) descriptor reads them
def operands(p, mut=None):
    """-> dict: P, absP [Z, M, N] (float64 A . B^T and |A| . |B|^T), A, B, bias [Z, M, N]-broadcastable, res, c0, x2, and `touched`
    [Z, M, N] bool: the elements whose terms `mut` changes."""
    g, dev = p.g, p.dev
    M, N, K, Z, nn = g["M"], g["N"], g["K"], g["Z"], g["nn"]
    name, arg = (mut[0], mut[1] if len(mut) > 1 else None) if mut else (None, None)
    n_main = p.c.get("n_main", 0)
    touched = torch.zeros(Z, M, N, dtype=torch.bool, device=dev)
    lda = K if name == "lda_as_k" else g["lda"]
    sA = 0 if mut == ("batch0", "a") else g["sA"]
    sB = 0 if mut == ("batch0", "b") else g["sB"]
    ldb = (N if nn else K) if name == "ldb_as_k" else g["ldb"]
    reads_differ = name in ("lda_as_k", "ldb_as_k", "nn_as_nk") or mut in (("batch0", "a"), ("batch0", "b"), ("tail_off", "B"))
    if reads_differ or p.base is None:
        A = p.read("A", _idx(HEAD, sA, lda, Z, M, K, dev))
        if nn and name != "nn_as_nk":
            b_idx = _idx(HEAD, sB, ldb, Z, K, N, dev).transpose(1, 2)
        else:
            b_idx = _idx(HEAD, sB, ldb, Z, N, K, dev)
        if mut == ("tail_off", "B"):  # the tail launch reads B from its first row / column again
            b_idx = torch.where((_ar(N, dev) >= n_main)[None, :, None], b_idx - n_main * (1 if nn else ldb), b_idx)
        B = p.read("B", b_idx)
        P, absP = A @ B.transpose(1, 2), A.abs() @ B.abs().transpose(1, 2)
        if not reads_differ:
            p.base = (A, B, P, absP)                          # (the unmutated reads: shared by every mutation that leaves them alone)
    else:
        A, B, P, absP = p.base
    if name in ("lda_as_k",):
        touched[:, 1:, :] = True
    if name == "ldb_as_k": touched[:, :, (0 if nn else 1):] = True
    if name == "nn_as_nk":
        touched[:] = True
    if mut in (("batch0", "a"), ("batch0", "b")):
        touched[1:] = True
    if mut == ("tail_off", "B"):
        touched[:, :, n_main:] = True
    w = _ktile_weights(p, mut)
    if w is not None:
        d = (w - 1.0).repeat_interleave(64)
        sel = d != 0
        Ad, Bd = A[:, :, sel], B[:, :, sel]
        P = P + (Ad * d[sel]) @ Bd.transpose(1, 2)
        touched |= (Ad.abs() @ Bd.abs().transpose(1, 2)) > 0
    if name == "seam_row":
        rows = _ar(M, dev)[(_ar(M, dev) % arg == 0) & (_ar(M, dev) > 0)]
        P = P.clone(); P[:, rows] = P[:, rows - 1]; touched[:, rows] = True
    if name == "seam_col":
        P = P.clone(); P[:, :, arg] = P[:, :, arg - 1]; touched[:, :, arg] = True
    if name == "gu_swapped" and g["epi"] == 1:
        P, absP = P[:, :, _perm_gu(N, dev)], absP[:, :, _perm_gu(N, dev)]; touched[:] = True
    ops = dict(P=P, absP=absP, K=K, alpha=g["alpha"], bias=None, res=None, c0=None, x2=None)
    if g["has_bias"]:
        n_i = _ar(N, dev) + (1 if name == "bias_shift" else 0)
        if mut == ("tail_off", "bias"):
            n_i = torch.where(n_i >= n_main, n_i - n_main, n_i)
            touched[:, :, n_main:] = True
        ops["bias"] = p.read("bias", HEAD + n_i)[None, None, :] * (g["alpha"] if name == "alpha_after_bias" else 1.0)
        if name in ("bias_shift", "alpha_after_bias"):
            touched[:] = True
    if g["Mr"]:
        rm = _ar(M, dev) if (name == "res_row_m" or not g["res_mod"]) else _ar(M, dev) % g["res_mod"]
        ldr = N if name == "ldr_as_n" else g["ldr"]
        r_idx = HEAD + (0 if mut == ("batch0", "r") else g["sR"]) * _ar(Z, dev)[:, None, None] + ldr * rm[None, :, None] + _ar(N, dev)[None, None, :]
        if mut == ("tail_off", "R"):
            r_idx = torch.where((_ar(N, dev) >= n_main)[None, None, :], r_idx - n_main, r_idx)
            touched[:, :, n_main:] = True
        ops["res"] = p.read("R", r_idx)
        if name == "res_row_m":  # rows past the residual's own are not residual data, whatever lies there
            ops["res"] = torch.where((rm >= g["Mr"])[None, :, None], torch.full((), float("nan"), dtype=F64, device=dev), ops["res"])
        if name == "res_row_m":
            touched[:, g["res_mod"]:] = True
        if name == "ldr_as_n":
            touched[:, rm >= 1] = True
        if mut == ("batch0", "r"):
            touched[1:] = True
    if g["accumulate"] and name != "acc_dropped":
        ops["c0"] = p.read("C", _idx(HEAD, g["sC"], g["ldc"], Z, M, N, dev))
    if name == "acc_dropped":
        touched[:] = True
    if g["form"] in ("act3", "ep2"):
        ld2 = g["ldc"] if name == "c2_ldc" else g["ldc2"]
        x_idx = _idx(HEAD, 0, ld2, 1, M, g["W2"], dev)
        if mut == ("tail_off", "C2"):
            shift = n_main * (2 if g["epi"] == 2 else 1)
            x_idx = torch.where((_ar(g["W2"], dev) >= shift)[None, None, :], x_idx - shift, x_idx); touched[:, :, n_main:] = True
        x2 = p.read("C2", x_idx)
        if name == "gu_swapped":
            x2 = x2[:, :, _perm_gu(g["W2"], dev)]
            touched[:] = True
        if name == "c2_ldc":
            touched[:, 1:] = True
        ops["x2"] = x2
    ops["touched"] = touched
    return ops


# ------------------------------------------------------------------ the two epilogues
def _rnd(y, e):
    return e + U * (y.abs() + e)


def _split_gu(x):
    """[.., 32 b + j] -> gate [.., 16 b + j], up [.., 16 b + j]"""
    blk = x.reshape(*x.shape[:-1], -1, 2, 16)
    return blk[..., 0, :].reshape(*x.shape[:-1], -1), blk[..., 1, :].reshape(*x.shape[:-1], -1)


def _join_gu(gate, up):
    sh = gate.shape[:-1]
    return torch.stack((gate.reshape(*sh, -1, 16), up.reshape(*sh, -1, 16)), -2).reshape(*sh, -1)


def ref_epilogue(g, o):
    """float64 epilogue, no rounding anywhere -> {out: (value, bar, live)}; bar = the absolute error bound of the module docstring;
    live = the output really depends on its pre-activation (|GELU'| / |SiLU'| >= 0.25: a changed pre-activation must show there).
    o["e_extra"], where given: error that the operands bring along (gemm_skinny_edge_util's norm stage), carried like the accumulation's."""
    al, P = o["alpha"], o["P"]
    acc = (2.0 * math.sqrt(o["K"]) + 4.0) * EPS
    x = al * P
    s0 = abs(al) * o["absP"]
    if o["bias"] is not None:
        x, s0 = x + o["bias"], s0 + o["bias"].abs()
    e = acc * s0 + o.get("e_extra", 0.0)
    yes = torch.ones_like(x, dtype=torch.bool)
    form = g["form"]
    if g["epi"] == 1:
        ec = _rnd(x, e)
        (gv, uv), (eg, eu) = _split_gu(x), _split_gu(ec)
        sg = torch.sigmoid(gv)
        sl = gv * sg
        es = _rnd(sl, 1.1 * eg + sl.abs() * (gv.abs() + 4.0) * 2.0 ** -23)
        a = sl * uv
        ea = es * (uv.abs() + eu) + sl.abs() * eu + EPS * a.abs()
        return {"C": (x, ec, yes), "C2": (a, _rnd(a, ea), (sg * (1.0 + gv * (1.0 - sg))).abs() >= 0.25)}
    if g["epi"] == 2:
        ed = _rnd(x, e)
        gv, uv = _split_gu(o["x2"])
        sg = torch.sigmoid(gv)
        sl = gv * sg
        esl = _rnd(sl, sl.abs() * (gv.abs() + 4.0) * 2.0 ** -23)
        du = x * sl
        edu = _rnd(du, ed * (sl.abs() + esl) + x.abs() * esl + EPS * du.abs())
        f = sg * (1.0 + gv * (1.0 - sg))
        ef = (gv.abs() + 8.0) * 2.0 ** -23 * sg * (1.0 + gv.abs() * (1.0 - sg))
        dg = x * uv * f
        edg = _rnd(dg, ed * (uv * f).abs() + (x.abs() + ed) * uv.abs() * ef + 3.0 * EPS * dg.abs())
        return {"C": (_join_gu(dg, du), _join_gu(edg, edu), _join_gu(yes, yes))}
    if form == "act2":
        ec = _rnd(x, e)
        y = gelu64(x)
        return {"C": (x, ec, yes), "C2": (y, _rnd(y, GELU_LIP * ec + GELU_APPROX * (x.abs() + ec)), gelu_grad64(x).abs() >= 0.25)}
    if form == "act3":
        ed = _rnd(x, e)
        gp = gelu_grad64(o["x2"])
        y = x * gp
        return {"C": (y, _rnd(y, ed * gp.abs() + (x.abs() + ed) * GELU_APPROX * (1.0 + o["x2"].abs()) + EPS * y.abs()), yes)}
    live = yes
    rnd = (lambda y, e_: e_ + EPS * y.abs()) if g["out_f32"] else _rnd
    y = x
    if not g["out_f32"]:
        e = rnd(y, e)
    if g["act"] == 1:
        live = gelu_grad64(x).abs() >= 0.25
        y, e = gelu64(x), GELU_LIP * e + GELU_APPROX * (x.abs() + e)
        e = rnd(y, e)
    if o["res"] is not None:
        y = y + o["res"]
        e = rnd(y, e + EPS * y.abs())
    if o["c0"] is not None:
        y = y + o["c0"]
        e = e + EPS * y.abs()
    return {"C": (y, e, live)}


def kernel_epilogue(g, o):
    """The kernels' epilogue arithmetic: f32 operations, bf16 roundings at the points of the module docstring -> {out: value}"""
    al, P = o["alpha"], o["P"]
    x = f32r(al * P + (o["bias"] if o["bias"] is not None else 0.0))
    form = g["form"]
    sig = lambda v: f32r(1.0 / f32r(1.0 + torch.exp(-v.to(torch.float32)).to(F64)))
    if g["epi"] == 1:
        c = bf(x)
        gv, uv = _split_gu(c)
        return {"C": c, "C2": bf(f32r(bf(f32r(gv * sig(gv))) * uv))}
    if g["epi"] == 2:
        d = bf(x)
        gv, uv = _split_gu(o["x2"])
        sg = sig(gv)
        du = bf(f32r(d * bf(f32r(gv * sg))))
        f = f32r(sg * f32r(1.0 + f32r(gv * f32r(1.0 - sg))))
        return {"C": _join_gu(bf(f32r(f32r(d * uv) * f)), du)}
    if form == "act2":
        return {"C": bf(x), "C2": bf(gelu_fast(bf(x)))}
    if form == "act3":
        return {"C": bf(f32r(bf(x) * gelu_fast_grad(o["x2"])))}
    if g["out_f32"]:
        t = gelu_fast(x) if g["act"] == 1 else x
        if o["res"] is not None:
            t = f32r(t + o["res"])
        if o["c0"] is not None:
            t = f32r(t + o["c0"])
        return {"C": t}
    t = bf(x)
    if g["act"] == 1:
        t = bf(gelu_fast(t))
    if o["res"] is not None:
        t = bf(f32r(t + o["res"]))
    return {"C": t}


def mfma_order_product(p, kstep=32):
    """A . B^T accumulated as the kernels do: one f32 partial per `kstep` columns of K (the MFMA's own sum taken as exact), added to an f32
    accumulator in K order; split-K: one accumulator per slab, the slabs added in slab order in f32."""
    o = dict(operands(p))
    g = p.g
    A, B = p.base[0], p.base[1]
    nk, s = g["K"] // 64, p.c.get("split", 0)
    slabs = [(z * nk // s * 64, (z + 1) * nk // s * 64) for z in range(s)] if (s > 1 and nk >= s) else [(0, g["K"])]
    total = None
    for lo, hi in slabs:
        acc = torch.zeros_like(o["P"])
        for k0 in range(lo, hi, kstep):
            acc = f32r(acc + f32r(A[:, :, k0:k0 + kstep] @ B[:, :, k0:k0 + kstep].transpose(1, 2)))
        total = acc if total is None else f32r(total + acc)
    o["P"] = total
    return o


# ------------------------------------------------------------------ images of the output buffers
class Image:
    """What one output buffer must hold: val / bar / live / src per buffer element, `mask` = written by the kernel (elsewhere: the canary;
    src = the logical element that lands there, -1 = none), `touched` = written from a logical element whose terms a mutation changes."""

    def __init__(self, n, dev):
        self.val = torch.zeros(n, dtype=F64, device=dev)
        self.bar = torch.zeros(n, dtype=F64, device=dev)
        self.mask = torch.zeros(n, dtype=torch.bool, device=dev)
        self.live = torch.zeros(n, dtype=torch.bool, device=dev)
        self.touched = torch.zeros(n, dtype=torch.bool, device=dev)
        self.src = torch.full((n,), -1, dtype=torch.long, device=dev)

    def put(self, idx, val, bar, live, touched, src, keep=None):
        flat = [t.reshape(-1) for t in (idx, val, bar, live, touched, src)]
        if keep is not None:
            flat = [t[keep.reshape(-1)] for t in flat]
        idx = flat[0] % self.val.numel()
        self.val[idx], self.bar[idx], self.live[idx], self.touched[idx], self.src[idx] = flat[1:]
        self.mask[idx] = True


def _widen(t, out, g):
    """[Z, M, N] per-product-element flags -> the logical shape of output `out`"""
    if out == "C" and g["epi"] == 2:
        return _join_gu(t, t)
    if out == "C2" and g["epi"] == 1:
        a, b = _split_gu(t)
        return a | b
    return t


def images(p, results, touched, mut=None):
    """Scatter {out: (value, bar, live)} into images of the output buffers through the (possibly mutated) descriptor."""
    g, dev = p.g, p.dev
    M, Z = g["M"], g["Z"]
    name = mut[0] if mut else None
    n_main = p.c.get("n_main", 0)
    out = {}
    for o_name, (val, bar, live) in results.items():
        is_c = o_name == "C"
        W = val.shape[-1]
        ld = g["ldc"] if is_c else g["ldc2"]
        if is_c and name == "ldc_as_n":
            ld = g["Nc"]
        s = (0 if mut == ("batch0", "c") else g["sC"]) if is_c else 0
        idx = _idx(HEAD, s, ld, val.shape[0], M, W, dev)
        per = W // g["N"] if W >= g["N"] else 1          # buffer columns per product column (2 for the [M, 2N] operands)
        if mut == ("tail_off", "C" if is_c else "C2") and not (o_name == "C2" and g["form"] in ("act3", "ep2")):
            shift = n_main * per if W >= g["N"] else n_main // 2
            idx = torch.where((_ar(W, dev) >= shift)[None, None, :], idx - shift, idx)
        t = _widen(touched, o_name, g)
        if name == "ldc_as_n" and is_c:
            t = t.clone()
            t[:, 1:] = True
        if mut == ("batch0", "c") and is_c:
            t = t.clone()
            t[1:] = True
        if mut == ("tail_off", "C" if is_c else "C2"): t = t.clone(); t[:, :, (n_main * per if W >= g["N"] else n_main // 2):] = True
        img = Image(p.buf[o_name].numel(), dev)
        src = _ar(val.numel(), dev).reshape(val.shape)
        keep = None
        if name == "last_row_skip":
            keep = torch.ones_like(live); keep[:, M - 1] = False
        if name == "last_cols_skip":
            keep = torch.ones_like(live); keep[:, :, W - 4:] = False
        if name == "row_past_m":  # row M written with row M - 1's values (first, so that real rows win)
            img.put(idx[:, M - 1:] + ld, val[:, M - 1:], bar[:, M - 1:], live[:, M - 1:], t[:, M - 1:], src[:, M - 1:])
        if name == "cols_past_n":
            img.put(idx[:, :, W - 4:] + 4, val[:, :, W - 4:], bar[:, :, W - 4:], live[:, :, W - 4:], t[:, :, W - 4:], src[:, :, W - 4:])
        cuts = (slice(0, W),)
        if mut == ("tail_off", "C" if is_c else "C2") and not (o_name == "C2" and g["form"] in ("act3", "ep2")):
            cuts = (slice(0, shift), slice(shift, W))        # the tail launch runs second: where both write, it wins
        for z in range(val.shape[0]):                    # in batch order: with a mutated stride the last writer wins
            for cut in cuts:
                img.put(idx[z][:, cut], val[z][:, cut], bar[z][:, cut], live[z][:, cut], t[z][:, cut], src[z][:, cut], None if keep is None else keep[z][:, cut])
        out[o_name] = img
    return out


def reference(p, mut=None):
    """-> {out: Image}: the float64 reference of the problem, or of the problem under one mutation."""
    o = operands(p, mut)
    return images(p, ref_epilogue(p.g, o), o["touched"], mut)


def kernel_images(p, o, mut=None):
    """The kernels' arithmetic on the operands `o` (operands(p, mut): exact products; mfma_order_product(p): the restatement) -> {out: Image}"""
    res = kernel_epilogue(p.g, o)
    full = {k: (v, torch.zeros_like(v), torch.ones_like(v, dtype=torch.bool)) for k, v in res.items()}
    return images(p, full, o["touched"], mut)


def restatement(p, kstep=32):
    return kernel_images(p, mfma_order_product(p, kstep))


def biteq_outputs(p):
    """The outputs of a family-S / Sb problem that must equal kernel_images(p, operands(p)) bit for bit (module docstring)."""
    if p.family not in ("S", "Sb"):
        return ()
    form = p.g["form"]
    if p.c.get("gelu"):
        return ()
    return ("C",) if (form in BITEQ_FORMS or form in ("act2", "ep1")) else ()


# ------------------------------------------------------------------ comparison
def output_bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def compare(p, ref, got, exact=None):
    """got: {out: the buffer after the call}; ref: reference(p); exact: {out: Image} whose values the written elements must equal bit for
    bit (family S).  -> {out: dict(worst = largest error in bar units, at = buffer index, canary = count of unwritten elements that
    changed, first = index of the first, nonfinite = count, unequal = count of elements that differ from `exact`)}"""
    res = {}
    for name, img in ref.items():
        buf = got[name]
        bits = output_bits(buf)
        canary = CANARY32 if buf.dtype == torch.float32 else CANARY16
        broken = (~img.mask) & (bits != canary)
        v = buf.to(F64)
        err = (v - img.val).abs()
        ratio = (err / img.bar).nan_to_num(nan=float("inf"), posinf=float("inf"))
        ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
        ratio = torch.where(img.mask, ratio, torch.zeros_like(ratio))
        at = int(ratio.argmax())
        r = dict(worst=ratio[at].item(), at=at, canary=int(broken.sum()), first=int(broken.to(torch.int8).argmax()) if broken.any() else -1,
                 nonfinite=int((img.mask & ~torch.isfinite(v)).sum()), unequal=0)
        if exact is not None and name in exact:
            want = exact[name].val.to(buf.dtype)
            r["unequal"] = int((img.mask & (output_bits(want) != bits)).sum())
        res[name] = r
    return res


def where(p, name, at):
    """A buffer index of output `name` in words."""
    g = p.g
    ld, s = (g["ldc"], g["sC"]) if name == "C" else (g["ldc2"], 0)
    rel = at - HEAD
    z = min(rel // s, g["Z"] - 1) if s > ld else 0
    rel -= z * s
    return f"{name}[{at}] (batch {z}, row {rel // ld}, column {rel % ld})"


def assert_ok(p, res, what):
    bad = []
    for name, r in res.items():
        if r["canary"]:
            bad.append(f"{r['canary']} elements outside the output were written, first {where(p, name, r['first'])}")
        if r["nonfinite"]:
            bad.append(f"{name}: {r['nonfinite']} outputs are not finite")
        if not r["worst"] <= 1.0:
            bad.append(f"{r['worst']:.3g} bars at {where(p, name, r['at'])}")
        if r["unequal"]:
            bad.append(f"{name}: {r['unequal']} elements differ from the exact result")
    assert not bad, f"{what}: " + "; ".join(bad)


def kind(p, name):
    return p.g["form"] + ("" if name == "C" else ".C2")


# ------------------------------------------------------------------ the cases of test_gemm_edges_gpu.py
def case_id(c):
    v = "auto" if c["variant"] is None else f"v{c['variant']}"
    extra = "".join(f"-{k}{c[k]}" for k in ("batch", "split") if c.get(k)) + (f"-{c['layout']}" if c.get("layout") else "") + ("-nn" if c.get("b_kn") else "")
    pad = "".join(f"-ld{k}+{n}" for k, n in c.get("pad", {}).items())
    return f"{c['group']}-{v}-{c['M']}x{c['N']}x{c['K']}{extra}{pad}"


SEED_BUMP = {"tiles-v11-257x4x2368": 1, "tiles-v60-1x4x192": 1}          # case id -> another draw (family G's 95 % share over a few hundred elements depends on the draw)
GROUPS = ("tiles", "second", "nn", "ld", "batched", "splitk", "tail")


def _case(group, **kw):
    c = dict(kw, group=group)
    c.setdefault("forms", ("plain",))
    v = 99 if c["variant"] is None else c["variant"]
    pads = sum((i + 2) * n for i, n in enumerate(c.get("pad", {}).values()))
    c["seed"] = (17 * c["M"] + 3 * c["N"] + c["K"] + 1009 * v + 13 * c.get("batch", 0) + 7 * c.get("split", 0) + 5 * pads + 29 * len(c.get("layout", ""))
                 + 100003 * GROUPS.index(group) + 31 * SEED_BUMP.get(case_id(c), 0))
    return c


def _cases():
    out = []
    plain8 = ("plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "f32", "f32_acc")
    Ns, Ks = (4, 132, 252, 256, 260, 520), (64, 128, 192, 320, 64 * 37)
    # 1. every product tile variant: every M, every K, all six N and all eight epilogues per variant; a residual and a GELU form on either
    #    side of N % 8 (the 16-byte staged store path and the fragment-layout one) - test_gemm_edges_cpu.py asserts this coverage
    for vi, v in enumerate((0, 11, 15, 16, 17, 18, 19, 31, 32, 33, 34, 59, 60, 61, 62)):
        bm = BM[v]
        for i, M in enumerate((1, bm - 1, bm, bm + 1)):
            forms = (plain8[(2 * i + vi) % 8], plain8[(2 * i + vi + 1) % 8])
            out.append(_case("tiles", variant=v, M=M, N=(4, 132, 252, 520)[(i + vi) % 4], K=Ks[(i + vi) % 5], forms=forms))
        out.append(_case("tiles", variant=v, M=2 * bm + 1, N=256, K=Ks[(4 + vi) % 5], forms=("bias_res", "bias_gelu", "res_mod")))
        out.append(_case("tiles", variant=v, M=bm + 1, N=260, K=192, forms=("bias_res", "bias_gelu", "res_mod")))
        if v in (61, 62):  # served by the 32 x 32 x 16 kernel itself (aligned, bf16) and handed to the twin (N % 8 != 0)
            out.append(_case("tiles", variant=v, M=bm + 1, N=264, K=192, forms=("bias_res", "bias_gelu", "res_mod"), m32=True))
            out.append(_case("tiles", variant=v, M=bm + 1, N=140, K=192, forms=("bias_res", "bias_gelu")))
    # 2. epilogues with a second operand: builds of 0 and 32..34 and launch_variant's reroutes
    #    (59 / 60 run the SwiGLU epilogues themselves; 61 / 62 hand every one of these to their twins)
    for v in (0, 32, 33, 34, 31, 11, 15, 16, 17, 18, 19, 59, 60, 61, 62):
        bm = BM[v]
        out.append(_case("second", variant=v, M=bm, N=256, K=128, forms=("act2", "act3", "ep1", "ep2"), opt2=(1, 2)))
        out.append(_case("second", variant=v, M=bm + 1, N=260 if v % 2 else 132, K=192, forms=("act2", "act3")))
        out.append(_case("second", variant=v, M=bm + 1, N=288, K=192, forms=("ep1", "ep2"), opt2=(1, 2)))      # (gemm_nt wants N % 32 == 0 for both)
    # 3. the NN form
    for v in (31, 32, 33, 34, None):
        bm = BM[v] if v is not None else 192
        out.append(_case("nn", variant=v, M=bm + 1, N=264, K=320, b_kn=True, pad=dict(b=8), forms=("plain", "bias_res")))
        out.append(_case("nn", variant=v, M=2 * bm + 1, N=136, K=128, b_kn=True, pad=dict(b=24), forms=("bias_res",)))
    # 4. padded leading dimensions, one at a time at both alignments gemm_nt admits, then all together; the conv2 strided-rows view
    for pad in (dict(a=8), dict(b=8), dict(c=4), dict(c=8), dict(r=4), dict(r=8), dict(a=24, b=16, c=12, r=20)):
        out.append(_case("ld", variant=None, M=130, N=132, K=192, pad=pad, forms=("bias_res", "res_mod", "f32_acc")))
    for pad in (dict(c2=4), dict(c2=8), dict(c=8, c2=16)):
        out.append(_case("ld", variant=None, M=130, N=132, K=192, pad=pad, forms=("act2", "act3")))
        out.append(_case("ld", variant=None, M=130, N=160, K=128, pad=pad, forms=("ep1", "ep2")))
    out.append(_case("ld", variant=None, M=72, N=132, K=192, layout="conv", lda=128, forms=("bias_gelu", "plain")))
    # 5. the batched form, as the project calls it
    for v, Z in ((0, 2), (31, 3), (34, 2), (None, 3)):
        out.append(_case("batched", variant=v, M=130, N=132, K=192, batch=Z, layout="conv", lda=128, forms=("bias_gelu",)))
        out.append(_case("batched", variant=v, M=70 if v is None else 50, N=64 + 4, K=128, batch=Z, layout="group", taps=4, pad=dict(c=4), forms=("f32",)))
        out.append(_case("batched", variant=v, M=129, N=260, K=128, batch=Z, layout="ksplit", pad=dict(a=8, b=8), forms=("f32",)))
        out.append(_case("batched", variant=v, M=129, N=132, K=64, batch=Z, forms=("bias_res", "res_mod")))
        out.append(_case("batched", variant=v, M=129, N=136, K=64, batch=Z, shared_r=True, shared_b=True, forms=("bias_res", "res_mod")))
    # 6. split-K (uvx_gemm_splitk, force_split): every tile the dispatcher serves split, K / 64 in {5, 37}, every epilogue of the reduce kernel
    sk_forms = ("plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "ep1")
    for vi, v in enumerate((0, 31, 32, 33, 34, 59, 60, 11, 15, 16, 17, 18, 19)):
        for si, s in enumerate((2, 3, 5, 16)):
            nk = (5, 37)[(si + vi) % 2]
            forms = (sk_forms[(2 * si + vi) % 7], sk_forms[(2 * si + vi + 1) % 7])
            out.append(_case("splitk", variant=v, M=BM[v] + 1, N=288, K=64 * nk, split=s, pad=dict(c=8), forms=forms))
    # 7. the tail split: 2 x 130 tiles of 128 x 128, the last 160 columns by a second launch (option 10 moves the threshold)
    out.append(_case("tail", variant=None, M=130, N=16544, K=128, n_main=16384, forms=("bias_res", "res_mod", "act2", "ep1", "ep2")))
    return out


CASES = _cases()


def families(c, form):
    """The input families of a case: S needs rows of A that do not overlap (Sb there); Sb also wherever the A side has its own stride."""
    if c.get("layout") in ("conv", "group"):
        return ("Sb", "R", "G")
    if c["group"] in ("nn", "ld", "batched"):
        return ("S", "Sb", "R", "G")
    return ("S", "R", "G")


def with_form(c, form):
    return dict(c, form=form)


def kstep(c, form):
    """K columns per MFMA of the kernel that serves the case: 16 where the 32 x 32 x 16 kernel itself runs (launch_variant's `plain`)"""
    return 16 if (c.get("m32") and form in ("plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha")) else 32
