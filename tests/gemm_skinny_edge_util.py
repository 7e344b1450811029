"""The few-row bf16 GEMM kernels (ultravox_amd/csrc/gemm_skinny.hip) under the harness of gemm_edge_util.py: the dispatcher restated as a pure
function, the three kernels' summation orders restated in f32, their own off-by-one mutations, a norm stage in front of the product for
uvx_gemm_rmsnorm, and the case list of test_gemm_skinny_edges_{cpu,gpu}.py.  Problem, geometry, the float64 reference, the bars, the input
families and the canaries are gemm_edge_util's; its case list is not touched.

Kernels (gemm_skinny_bf16; `served_by` below restates the choice):
  rows    gemv_rows_bf16_k<MB, R, RB>: M <= 2.  A block owns RB weight rows (32 under SwiGLU, else gemv_rows_per_block's pick by CU balance), walks
          them R at a time; wave w takes the 512-element K steps w, w + 8, ..; lane l the 8 elements [512 j + 8 l, + 8) of a step.  Sum order:
          per lane over its steps, halving butterfly over the lanes (a balanced tree: l with l ^ 32, then ^ 16, ..), waves 0..7 in order, * alpha.
  frag    gemm_skinny_bf16_k<TILES, false>: M <= 16.  A block owns 16 TILES columns; one MFMA per 32-column chunk of K; wave w takes the chunks
          [w n / 8, (w + 1) n / 8) when n = K / 32 is a multiple of 8 (span), else w, w + 8, .. (interleave); UN = 8 (TILES 1) or 4 (TILES 2)
          chunks per unrolled trip, the rest one by one.  Sum order: per wave in its chunk order, waves in order, * alpha.
  staged  gemm_skinny_bf16_k<TILES, true, MT>: M <= 64, K % 2048 == 0.  Wave w owns the span [w K / 8, (w + 1) K / 8) in nst = K / 2048 steps of 256
          columns (eight MFMAs each, in K order); MT = 1, 2, 4 activation row tiles; wave mt finishes row tile mt.
Epilogue: t = round(acc alpha + bias); GELU: round(gelu_fast(t)); residual: round(t + r) - gemm_edge_util's points.  SwiGLU: gate, up =
round(acc alpha), C2 = round(round(g / (1 + __expf(-g))) * up): the quotient form, not the tiled kernels' g * sigmoid(g); both are SiLU to
within the f32 exp, which is what the ep1.C2 bar allows (skinny_kernel_epilogue restates the quotient form; the CPU test holds it to that bar).

uvx_gemm_rmsnorm (families R and G only: a selector row does not survive a normalisation).  The reference takes the NORMALISED activations
in float64 with the kernels' rounding points (flavor 0: round(w * round(x rstd)); flavor 1: round((x rstd) (1 + w)); rstd = (mean(x^2) +
eps)^-1/2 exactly) and runs the product and epilogue above on them with the same bars.  An activation is TIPPABLE when the pre-rounding value
that depends on rstd (x rstd; (x rstd)(1 + w)) lies within a relative 2^-20 of a bf16 rounding boundary - 2^-20 covers the f32 sum of
squares in any order, rsqrtf and two f32 products; w * a of two bf16 values is exact in f32, so flavor 0's outer rounding is decided.  Each
element's bar gets sum over tippable k of ulp_bf16(xn[m, k]) |B[n, k]| |alpha| more (entered as incoming error, so every later step of the
epilogue carries it); at most 1e-3 of a case's activations may be tippable (asserted in both tests).

Mutations of these kernels' own arithmetic (the K-range ones at the kernels' granularity; `mutations`):
  chunk_last_drop (the last 32 columns), lane_tail_drop (the partial 512-step of the row kernel), wave_omit / wave_twice (every K position of
  the wave that sums the last one, under the case's mapping), step_last_drop (the last 256 columns of every staged span), seam_row:16 (row tile
  mt + 1 gets tile mt's products), seam_col:8|16|32 (a block's first weight row read from the previous block), rows_swapped (M = 2: the
  butterfly's m index), clamp_written (the clamped weight row N - 1 stored at column N), tile1_as_tile0 (TILES = 2, staged: the second
  16-column tile of a block streams the first one's weight rows - issue() without its 16 t), and for the fused cases norm_w_shift:8,
  norm_row0 (every row with row 0's rstd), norm_flavor_swapped, eps_dropped (counted on the row whose mean square is 3 eps).
A K-range mutation that moves a share f of K moves a ramp output (family R: positive terms, nothing cancels) by about f of its size, and one
bf16 rounding is 2^-8 of it: below one part in 37 of K the selector families answer, bit for bit (test_gemm_skinny_edges_cpu.py, _asked).  For
that their one-hot rows sit where these kernels' K loops end (selector_positions: the last chunk, step and wave, the first K-tile, and
gemm_edge_util's 29 i mod K) - with M <= 2 or N = 4 rows the merged positions alone reach none of them.  The fused cases have no selector
family: the K-range mutations under that share are listed on the plain cases only, whose K loops the fused kernels share."""
import math

import torch

import gemm_edge_util as U
from gemm_edge_util import F64, HEAD, bf, f32r

NORM_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
TIP, TIP_CAP = 2.0 ** -20, 1e-3
FORMS = ("plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "ep1", "bias_gelu_res")
CUS = 256                # the CU count the case list is laid out for (an MI355X; the GPU test re-derives the RB cases if the device differs)


# ------------------------------------------------------------------ the dispatcher, restated
def rows_per_block(N, swiglu, cus):
    """gemv_rows_per_block: 32 under SwiGLU; else the largest of 32 / 16 / 8 that no smaller one beats by more than 5 % in CU balance"""
    if swiglu:
        return 32
    best, best_cost = 32, 1e30
    for rb in (32, 16, 8):
        if rb == 32 and N < 16384:
            continue
        per_cu = -(-N // rb) / cus
        cost = math.ceil(per_cu) / per_cu
        if cost < 0.95 * best_cost:
            best_cost, best = cost, rb
    return best


def served_by(M, N, K, option4, option26, swiglu, cus):
    """gemm_nt's few-row branch, gemm_skinny_applicable and gemm_skinny_bf16 for a bf16, unbatched NT problem whose leading dimensions pass
    gemm_nt's checks -> ("rows", MB, R, RB) | ("staged", TILES, MT) | ("frag", TILES) | "tiled" """
    rows_ok = M <= 16 or (M <= 64 and K % 2048 == 0 and option4 != 2)
    if not (option4 and M > 0 and rows_ok and K % 64 == 0 and N % 4 == 0 and (not swiglu or N % 32 == 0)):
        return "tiled"
    if M <= 2 and option4 != 2:
        rb = rows_per_block(N, swiglu, cus)
        if M == 2:
            return ("rows", 2, 4, rb)
        return ("rows", 1, {0: 2, 8: 8, 16: 16 if rb >= 16 else 8}.get(option26, 4), rb)
    tiles = 2 if (swiglu or N >= 16384) else 1
    if K % 2048 == 0 and option4 != 2:
        return ("staged", tiles, 1 if M <= 16 else 2 if M <= 32 else 4)
    return ("frag", tiles)


def fused_by(M, N, K, option4, option24, option26, swiglu, cus):
    """gemm_skinny_rmsnorm_bf16 (lda = K) -> (201, ("rows", ..)) | (202, ("staged", TILES, 1)) | (200 or a tile, the two launches' GEMM)"""
    if option4 == 1 and M <= 2 and K % 8 == 0 and K <= 16384 and M * K * 2 <= 64 * 1024 and (not swiglu or N % 32 == 0):
        return 201, served_by(M, N, K, 1, option26, swiglu, cus)
    if option4 == 1 and option24 == 1 and 3 <= M <= 16 and K % 2048 == 0 and N % 4 == 0:
        return 202, ("staged", 2 if (swiglu or N >= 16384) else 1, 1)
    s = served_by(M, N, K, option4, option26, swiglu, cus)
    return (200 if s != "tiled" else 0), s


def block_cols(s):
    return s[3] if s[0] == "rows" else 16 * s[1]


def wave_positions(s, K):
    """[8, K] bool: the K positions wave w sums under the served kernel's mapping"""
    k = torch.arange(K)
    if s[0] == "rows":
        wave = (k // 512) % 8
    elif s[0] == "staged" or (K // 32) % 8 == 0:
        wave = k // (K // 8)
    else:
        wave = (k // 32) % 8
    return wave[None, :] == torch.arange(8)[:, None]


def loop_shape(s, K):
    """what the K loops of the served kernel do -> dict (the CPU test's coverage)"""
    if s[0] == "rows":
        ns = -(-K // 512)
        return dict(steps=ns, partial=K % 512 != 0, q1_used=ns > 8, second_trip=ns > 16, guard_hit=any(j + 8 >= ns for w in range(8) for j in range(w, ns, 16)))
    if s[0] == "staged":
        return dict(nst=K // 2048)
    n, un = K // 32, 8 if s[1] == 1 else 4
    span = n % 8 == 0
    per_wave = [n // 8] * 8 if span else [len(range(w, n, 8)) for w in range(8)]
    return dict(span=span, un=un, waves={(c // un, c % un) for c in per_wave if c}, idle=per_wave.count(0))      # waves: (unrolled trips, remainder) of the busy ones


# ------------------------------------------------------------------ problems
def fused(c):
    return c.get("flavor") is not None


def with_form(c, form):
    c = dict(c, form=form, kind=form)
    if form == "bias_gelu_res":
        c.update(form="bias_gelu", residual=True)
    if form == "res_mod":  # smaller than M wherever M allows, never a divisor of 16
        c["res_mod"] = 7 if c["M"] > 7 else 3 if c["M"] > 3 else max(c["M"] - 1, 1)
    return c


def kind(p, name):
    return p.c["kind"] + ("" if name == "C" else ".C2")


def norm_weights(c, family, device="cpu"):
    """drawn, so without a period in k: a read shifted by a fragment, a step or a wave span meets other weights.  Family R: 1 + 0.2 randn (positive:
    nothing cancels); family G: +-(0.75 .. 1.25) with a drawn sign, so that a shifted read moves a Gaussian output by about its own size"""
    gen = torch.Generator().manual_seed(c["seed"] + 77)
    w = 1.0 + 0.2 * torch.randn(c["K"], generator=gen, dtype=F64)
    if family == "G":
        w = (0.75 + 0.5 * torch.rand(c["K"], generator=gen, dtype=F64)) * (1.0 - 2.0 * torch.randint(0, 2, (c["K"],), generator=gen).to(F64))
    return w.to(torch.bfloat16).to(device)


def selector_positions(n, K):
    """K position of selector row i: rows 0, 3, 6, .. walk back from K - 1 (the last 32-column chunk, the last 256-column step, the partial 512-step,
    the last wave), rows 1, 4, .. forward from 0 (the first K-tile), rows 2, 5, .. gemm_edge_util's 29 i mod K - with few rows (M <= 2, N = 4) its
    positions alone would leave every edge of the K loops to the other families"""
    i = torch.arange(n)
    return torch.where(i % 3 == 0, K - 1 - (i // 3) % 32, torch.where(i % 3 == 1, (i // 3) % 64, (29 * i) % K))


def _place_selectors(p):
    """family S: the one-hot rows of A, family Sb: those of B, moved to selector_positions (the values stay gemm_edge_util's)"""
    g = p.g
    name, rows, ld = ("A", g["M"], g["lda"]) if p.family == "S" else ("B", g["N"], g["ldb"])
    K, buf = g["K"], p.buf[name]
    s = torch.tensor([1.0, -0.5, 2.0, -1.0, 0.5, -2.0], dtype=F64)[torch.arange(rows) % 6]
    block = torch.zeros(rows, K, dtype=F64)
    block[torch.arange(rows), selector_positions(rows, K)] = s
    idx = (HEAD + ld * torch.arange(rows)[:, None] + torch.arange(K)[None, :]).to(buf.device)
    buf[idx.reshape(-1)] = block.reshape(-1).to(torch.bfloat16).to(buf.device)


def make_problem(c, family, device="cpu"):
    """gemm_edge_util.make_problem; a fused case gets the norm weights (buffer W, canaries around them) and its special rows: `small_row` scaled
    down to a mean square of 3e-5 (eps = 1e-5 is a third of it), `zero_row` all zeros."""
    p = U.make_problem(c, family, device)
    if family in ("S", "Sb"):
        _place_selectors(p)
    if fused(c):
        K = c["K"]
        if p.g["epi"] == 1:  # the normalised activations are of size 1: alpha makes gate and up of size 1 again (the ramp's product is 0.9 K, the Gaussian's 0.5 sqrt(K)),
            p.g = dict(p.g, alpha=2.0 ** -round(math.log2(0.9 * K if family == "R" else 0.5 * math.sqrt(K))))      # where silu(gate) up is far from silu(up) gate
        w = torch.full((HEAD + K + 72,), U.CANARY16, dtype=torch.int16).view(torch.bfloat16)
        w[HEAD:HEAD + K] = norm_weights(c, family)
        p.buf["W"] = w.to(device)
        a = p.buf["A"]
        if c.get("small_row") is not None:
            lo = HEAD + c["small_row"] * K
            row = a[lo:lo + K].to(F64)
            a[lo:lo + K] = (row * math.sqrt(3e-5 / float((row * row).mean()))).to(torch.bfloat16)
        if c.get("zero_row") is not None:
            lo = HEAD + c["zero_row"] * K
            a[lo:lo + K] = 0.0
    p.tips = None
    return p


# ------------------------------------------------------------------ the norm stage
def normed(x, w, flavor, eps=NORM_EPS, row0=False):
    """float64 RMSNorm of the rows of x [.., M, K] with the kernels' two bf16 rounding points -> (xn, pre): pre = the value before the rounding
    that depends on rstd"""
    ms = (x * x).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(ms + eps)
    if row0:
        rstd = rstd[..., :1, :].expand_as(rstd)
    v = x * rstd
    if flavor == 0:
        return bf(w * bf(v)), v
    v = v * (1.0 + w)
    return bf(v), v


def tippable(pre):
    return bf(pre * (1.0 + TIP)) != bf(pre * (1.0 - TIP))


def ulp_bf16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.where(x == 0, torch.zeros_like(x), torch.exp2(e - 7.0))


def _raw(p):
    g = p.g
    A = p.read("A", U._idx(HEAD, 0, g["lda"], 1, g["M"], g["K"], p.dev))
    B = p.read("B", U._idx(HEAD, 0, g["ldb"], 1, g["N"], g["K"], p.dev))
    return A, B


def _norm_base(p, mut=None):
    """-> (xn, B, P, absP) of a fused problem, possibly under a mutation of the norm stage; the unmutated one also fills p.tips = (share of
    tippable activations, the bars' extra term [1, M, N])"""
    name = mut[0] if mut else None
    x, B = _raw(p)
    w = p.buf["W"][HEAD:HEAD + p.g["K"]].to(F64)
    flavor = p.c["flavor"]
    if name == "norm_w_shift":
        w = torch.roll(w, -mut[1])
    if name == "norm_flavor_swapped":
        flavor = 1 - flavor
    xn, pre = normed(x, w, flavor, 0.0 if name == "eps_dropped" else NORM_EPS, row0=name == "norm_row0")
    base = (xn, B, xn @ B.transpose(1, 2), xn.abs() @ B.abs().transpose(1, 2))
    if mut is None and p.tips is None:
        tip = tippable(pre)
        p.tips = (tip.to(F64).mean().item(), abs(p.g["alpha"]) * ((tip.to(F64) * ulp_bf16(xn)) @ B.abs().transpose(1, 2)))
    return base


# ------------------------------------------------------------------ mutations
OWN = ("chunk_last_drop", "lane_tail_drop", "wave_omit", "wave_twice", "step_last_drop", "seam_row", "seam_col", "rows_swapped", "clamp_written", "tile1_as_tile0",
       "norm_w_shift", "norm_row0", "norm_flavor_swapped", "eps_dropped")
NORM_MUTS = ("norm_w_shift", "norm_row0", "norm_flavor_swapped", "eps_dropped")
K_RANGE = U.K_RANGE + ("chunk_last_drop", "lane_tail_drop", "wave_omit", "wave_twice", "step_last_drop")
ALL_MUTATIONS = ("k_first_drop", "k_first_twice", "k_last_drop", "k_last_twice", "last_row_skip", "last_cols_skip", "row_past_m", "cols_past_n", "bias_shift",
                 "res_row_m", "ldr_as_n", "lda_as_k", "ldb_as_k", "ldc_as_n", "alpha_after_bias", "gu_swapped", "chunk_last_drop", "lane_tail_drop", "wave_omit",
                 "wave_twice", "step_last_drop", "seam_row:16", "seam_col:8", "seam_col:16", "seam_col:32", "rows_swapped", "clamp_written", "tile1_as_tile0", "norm_w_shift:8",
                 "norm_row0", "norm_flavor_swapped", "eps_dropped")
DISPLACED = U.DISPLACED


def kernel_of(c, cus=CUS):
    """the kernel whose arithmetic a case's result comes from (a fused case: its GEMM's) - None where the tiled kernels serve it"""
    sw = c.get("form") == "ep1" or c.get("forms") == ("ep1",)
    if fused(c):
        s = fused_by(c["M"], c["N"], c["K"], 1, c.get("opt24", 0), c.get("opt26", 0), sw, cus)[1]
    else:
        s = served_by(c["M"], c["N"], c["K"], c.get("opt4", 1), c.get("opt26", 0), sw, cus)
    return None if s == "tiled" else s


def k_weights(c, mut, s):
    """how often each K position enters the sum under one of this module's K-range mutations -> [K] float64, or None where it has no meaning"""
    K, name = c["K"], mut[0]
    w = torch.ones(K, dtype=F64)
    pos = wave_positions(s, K)
    if name == "chunk_last_drop" and s[0] != "rows":
        w[K - 32:] = 0
    elif name == "lane_tail_drop" and s[0] == "rows" and K % 512:
        w[K // 512 * 512:] = 0
    elif name in ("wave_omit", "wave_twice") and int(pos.any(1).sum()) > 1:
        w[pos[int(torch.nonzero(pos[:, K - 1]))]] = 0 if name == "wave_omit" else 2
    elif name == "step_last_drop" and s[0] == "staged":
        w[(torch.arange(K) % (K // 8)) >= K // 8 - 256] = 0
    else:
        return None
    return w


def k_share(c, mut, s):
    """the share of K a K-range mutation moves"""
    if mut[0] in U.K_RANGE:
        return 64.0 / c["K"]
    w = k_weights(c, mut, s)
    return float((w != 1).sum()) / c["K"]


def mutations(c):
    """every off-by-one with a meaning on the case: gemm_edge_util's that apply to one unbatched NT launch, and this module's"""
    s = kernel_of(c)
    g = U.geometry(c)
    out = [m for m in U.mutations(c) if m[0] not in ("seam_row", "seam_col") and not (m[0] == "res_row_m" and c["M"] <= g["res_mod"]) and not (m[0] == "ldr_as_n" and g["Mr"] == 1)]
    if s is None:
        return out
    g = U.geometry(c)
    for name in ("chunk_last_drop", "lane_tail_drop", "wave_omit", "wave_twice", "step_last_drop"):
        if k_weights(c, (name,), s) is not None:
            out.append((name,))
    if fused(c):  # no selector family here: a K-range mutation under one part in 37 of K is left to the plain cases, whose K loops these are
        out = [m for m in out if m[0] not in K_RANGE or k_share(c, m, s) >= 1.0 / 37.0]
    if c["M"] > 16:
        out.append(("seam_row", 16))
    if c["N"] > block_cols(s):
        out.append(("seam_col", block_cols(s)))
    if s[0] == "rows" and c["M"] == 2:
        out.append(("rows_swapped",))
    if s[0] == "staged" and s[1] == 2:
        out.append(("tile1_as_tile0",))
    if not g["epi"] and c["N"] % block_cols(s):
        out.append(("clamp_written",))
    if fused(c):
        out += [("norm_w_shift", 8), ("norm_flavor_swapped",)] + ([("norm_row0",)] if c.get("small_row") is not None else []) + ([("eps_dropped",)] if c.get("small_row") is not None else [])
    return out


def operands(p, mut=None):
    """gemm_edge_util.operands with the norm stage in front (fused cases) and this module's mutations"""
    name = mut[0] if mut else None
    own = name in OWN
    if p.base is None:
        if fused(p.c):
            p.base = _norm_base(p)
        else:
            U.operands(p)
    keep = p.base
    if name in NORM_MUTS:
        p.base = _norm_base(p, mut)
    try:
        o = dict(U.operands(p, None if own else mut))
        A, B = p.base[0], p.base[1]
    finally:
        p.base = keep
    if fused(p.c):
        o["e_extra"] = p.tips[1]
    if not own:
        return o
    touched, P = o["touched"].clone(), o["P"]
    M, N = p.g["M"], p.g["N"]
    s = kernel_of(p.c)
    if name in NORM_MUTS:       # (a zero row stays zero under every one of them)
        touched[:] = True
        if name == "norm_row0":  # the rows whose own rstd is more than 1 / 16 away from row 0's: many bars
            x = _raw(p)[0][0]
            r = 1.0 / torch.sqrt((x * x).mean(-1) + NORM_EPS)
            touched[:] = False
            touched[:, (r / r[0] - 1.0).abs() > 1.0 / 16.0] = True
        if name == "eps_dropped":
            touched[:] = False
            touched[:, p.c["small_row"]] = True
        if p.c.get("zero_row") is not None:
            touched[:, p.c["zero_row"]] = False
    elif name == "seam_row":
        P = P.clone(); P[:, 16:] = o["P"][:, :M - 16]; touched[:, 16:] = True
    elif name == "seam_col":
        cols = torch.arange(mut[1], N, mut[1], device=p.dev)
        P = P.clone(); P[:, :, cols] = o["P"][:, :, cols - 1]; touched[:, :, cols] = True
    elif name == "rows_swapped":
        P = P.flip(1); touched[:] = True
    elif name == "tile1_as_tile0":
        cols = torch.arange(N, device=p.dev)
        cols = cols[cols % 32 >= 16]
        P = P.clone(); P[:, :, cols] = o["P"][:, :, cols - 16]; touched[:, :, cols] = True
    elif name != "clamp_written":
        d = (k_weights(p.c, mut, s) - 1.0).to(p.dev)
        sel = d != 0
        Ad, Bd = A[:, :, sel], B[:, :, sel]
        P = P + (Ad * d[sel]) @ Bd.transpose(1, 2)
        touched |= (Ad.abs() @ Bd.abs().transpose(1, 2)) > 0
    if name not in NORM_MUTS and p.c.get("zero_row") is not None:      # (its products are zero whichever weight row they come from)
        touched[:, p.c["zero_row"]] = False
    o["P"], o["touched"] = P, touched
    return o


def images(p, results, touched, mut=None):
    name = mut[0] if mut else None
    out = U.images(p, results, touched, None if name in OWN else mut)
    if name == "clamp_written":  # column N of every row gets column N - 1's value, where no real element lands
        g, img = p.g, out["C"]
        val, bar, live = results["C"]
        at = HEAD + g["ldc"] * torch.arange(g["M"], device=p.dev) + g["N"]
        free = ~img.mask[at]
        src = torch.arange(val.numel(), device=p.dev).reshape(val.shape)[0, :, -1]
        img.put(at, val[0, :, -1], bar[0, :, -1], live[0, :, -1], torch.ones_like(free), src, free)
    return out


def reference(p, mut=None):
    o = operands(p, mut)
    return images(p, U.ref_epilogue(p.g, o), o["touched"], mut)


def skinny_kernel_epilogue(g, o):
    """gemm_edge_util.kernel_epilogue with SiLU as these kernels compute it: g / (1 + __expf(-g))"""
    if g["epi"] != 1:
        return U.kernel_epilogue(g, o)
    c = bf(f32r(o["alpha"] * o["P"]))
    gv, uv = U._split_gu(c)
    sl = f32r(gv / f32r(1.0 + torch.exp(-gv.to(torch.float32)).to(F64)))
    return {"C": c, "C2": bf(f32r(bf(sl) * uv))}


def kernel_images(p, o, mut=None):
    res = skinny_kernel_epilogue(p.g, o)
    full = {k: (v, torch.zeros_like(v), torch.ones_like(v, dtype=torch.bool)) for k, v in res.items()}
    return images(p, full, o["touched"], mut)


# ------------------------------------------------------------------ the kernels' summation orders in f32
def _fold(x):
    """wave_sum / wave_sum_multi over the last axis (64 lanes): l with l ^ 32, then ^ 16, .."""
    h = x.shape[-1] // 2
    while h >= 1:
        x = f32r(x[..., :h] + x[..., h:2 * h])
        h //= 2
    return x[..., 0]


def _in_order(x):
    """0.f + x[.., 0] + x[.., 1] + .. in f32"""
    t = torch.zeros_like(x[..., 0])
    for i in range(x.shape[-1]):
        t = f32r(t + x[..., i])
    return t


def order_product(A, B, s):
    """A [M, K] . B [N, K]^T summed as kernel `s` sums it (module docstring) -> [M, N], f32 values in float64"""
    M, K = A.shape
    N = B.shape[0]
    if s[0] == "rows":
        acc = torch.zeros(M, N, 8, 64, dtype=F64, device=A.device)
        for j in range(-(-K // 512)):
            lo, hi = j * 512, min(K, j * 512 + 512)
            ng = (hi - lo) // 8
            part = f32r((A[:, None, lo:hi].reshape(M, 1, ng, 8) * B[None, :, lo:hi].reshape(1, N, ng, 8)).sum(-1))
            acc[:, :, j % 8, :ng] = f32r(acc[:, :, j % 8, :ng] + part)
        return _in_order(_fold(acc))
    n = K // 32
    part = f32r(torch.einsum("mck,nck->mnc", A.reshape(M, n, 32), B.reshape(N, n, 32)))
    if s[0] == "staged" or n % 8 == 0:
        per_wave = part.reshape(M, N, 8, n // 8)
    else:
        pad = -n % 8
        per_wave = torch.cat((part, torch.zeros(M, N, pad, dtype=F64, device=A.device)), -1).reshape(M, N, -1, 8).transpose(2, 3)
    return _in_order(_in_order(per_wave))


def _rstd32(x, s, K):
    """rsqrtf(sum of squares / K + eps) with the sum in each prologue's own order (x [M, K] bf16 values)"""
    M = x.shape[0]
    q = x * x
    if s[0] == "rows":      # thread t: vectors t, t + 512, ..; wave butterfly; waves in order (block_sum)
        nq = -(-K // 4096)
        pad = torch.zeros(M, 4096 * nq, dtype=F64, device=x.device)
        pad[:, :K] = q
        per_thread = _in_order(pad.reshape(M, nq, 512, 8).permute(0, 2, 1, 3).reshape(M, 512, 8 * nq))
        tot = _in_order(_fold(per_thread.reshape(M, 8, 64)))
    else:                   # lane (row, fg) of wave w: its 8 elements of every chunk of the span; fg ^ 1, fg ^ 2; waves in order
        per_lane = _in_order(q.reshape(M, 8, K // 256, 4, 8).permute(0, 1, 3, 2, 4).reshape(M, 8, 4, K // 32))
        tot = _in_order(f32r(f32r(per_lane[..., 0] + per_lane[..., 1]) + f32r(per_lane[..., 2] + per_lane[..., 3])))
    return f32r(1.0 / torch.sqrt(f32r(f32r(tot / K) + NORM_EPS)))[:, None]


def restatement(p):
    """{out: Image}: the served kernel's arithmetic in f32 - prologue (fused cases), product in the kernel's order, epilogue"""
    o = dict(operands(p))
    s = kernel_of(p.c)
    if fused(p.c):
        x = _raw(p)[0][0]
        w = p.buf["W"][HEAD:HEAD + p.g["K"]].to(F64)
        v = f32r(x * _rstd32(x, s, p.g["K"]))
        A = bf(w * bf(v)) if p.c["flavor"] == 0 else bf(f32r(v * f32r(1.0 + w)))
    else:
        A = p.base[0][0]
    B = p.base[1][0]
    o["P"] = order_product(A, B, s)[None]
    return kernel_images(p, o)


def biteq_outputs(p):
    return U.biteq_outputs(p)


# ------------------------------------------------------------------ cases
GROUPS = ("rows", "frag", "staged", "boundary", "ld", "fused_rows", "fused_staged")
# case id -> another draw.  Family G's 95 % share of a few dozen affected elements depends on the draw (as gemm_edge_util.SEED_BUMP), and a fused
# case's first draw may have more than TIP_CAP tippable activations (at K <= 576 that is a single one): the first draw that meets both.
SEED_BUMP = {"rows-2x12x64": 1, "rows-1x36x576": 1, "rows-2x12x2368": 3, "rows-1x32x576": 1,
             "rows-1x36x576-r8": 4, "rows-1x36x576-r16": 1, "frag-16x16x64": 1, "frag-16x4x576": 4,
             "frag-1x4x2048-o4=2": 1, "frag-1x20x576-o4=2": 1, "frag-16x4x576-o4=2": 1, "staged-3x4x2048": 2,
             "staged-32x4x6144": 1, "staged-63x4x2048": 1, "ld-2x36x576-lda+8-ldb+8-ldc+4-ldr+4": 7, "ld-2x36x576-lda+24-ldb+24-ldc+12-ldr+12": 7,
             "ld-2x96x576-lda+8-ldb+24-ldc+12-ldc2+4": 1, "ld-2x96x576-lda+24-ldb+8-ldc+4-ldc2+12": 2, "ld-15x36x576-lda+24-ldb+24-ldc+12-ldr+12": 6, "ld-33x36x2048-lda+24-ldb+24-ldc+12-ldr+12": 4,
             "fused_rows-1x36x64-f0": 2, "fused_rows-1x36x4160-f1": 1, "fused_rows-1x36x8192-f0": 1, "fused_rows-1x36x16384-f1": 1,
             "fused_rows-1x36x576-r0-f0": 1, "fused_rows-1x36x576-r4-f1": 12, "fused_rows-1x36x576-r8-f0": 1, "fused_rows-1x36x576-r16-f1": 12,
             "fused_staged-3x20x2048-f0-o24-small-zero": 1, "fused_staged-16x20x4096-f0-o24-small-zero": 1,}


def case_id(c):
    extra = (f"-o4={c['opt4']}" if c.get("opt4", 1) != 1 else "") + (f"-r{c['opt26']}" if "opt26" in c else "") + (f"-f{c['flavor']}" if fused(c) else "")
    extra += ("-o24" if c.get("opt24") else "") + ("-small" if c.get("small_row") is not None else "") + ("-zero" if c.get("zero_row") is not None else "")
    pad = "".join(f"-ld{k}+{n}" for k, n in c.get("pad", {}).items())
    return f"{c['group']}-{c['M']}x{c['N']}x{c['K']}{extra}{pad}"


def _case(group, **kw):
    c = dict(kw, group=group, variant=None)
    c.setdefault("forms", ("plain",))
    pads = sum((i + 2) * n for i, n in enumerate(c.get("pad", {}).values()))
    c["seed"] = (17 * c["M"] + 3 * c["N"] + c["K"] + 1009 * c.get("opt4", 1) + 7 * c.get("opt26", 0) + 5 * pads + 11 * (c.get("flavor") or 0) + 13 * c.get("opt24", 0)
                 + 100003 * (10 + GROUPS.index(group)) + 31 * SEED_BUMP.get(case_id(c), 0))
    return c


SEVEN = ("plain", "bias", "bias_gelu", "bias_res", "res_mod", "alpha", "bias_gelu_res")
RB32_N, RB16_N = 24572, 4092          # at 256 CUs: 768 blocks of 32 rows = 3 per CU, the last one 28 rows; 256 blocks of 16 rows, the last one 12


def _cases():
    out = []
    two = lambda i: (SEVEN[(2 * i) % 7], SEVEN[(2 * i + 1) % 7])
    # A. rows: M = 1, 2 at every K, RB = 8 (N = 12, 36, 100; N = 4 is ONE block of 16 rows under the 5 % rule: all sixteen clamp to row 3)
    Ks, Ns = (64, 512, 576, 4096 + 64, 64 * 37), (4, 12, 36, 100)
    for i, K in enumerate(Ks):
        out.append(_case("rows", M=1, N=Ns[i % 4], K=K, forms=two(i)))
        out.append(_case("rows", M=2, N=Ns[(i + 1) % 4], K=K, forms=two(i + 5)))
    out.append(_case("rows", M=1, N=RB16_N, K=64, forms=two(3)))
    out.append(_case("rows", M=2, N=RB16_N, K=576, forms=two(4)))
    out.append(_case("rows", M=1, N=RB32_N, K=192, forms=two(5)))
    out.append(_case("rows", M=2, N=RB32_N, K=192, forms=two(6)))
    for M, N, K in ((1, 32, 576), (2, 96, 4096 + 64), (1, 96, 64), (2, 32, 512)):
        out.append(_case("rows", M=M, N=N, K=K, forms=("ep1",)))
    for i, r in enumerate((0, 4, 8, 16)):     # rows in flight, on one ragged case per RB
        out.append(_case("rows", M=1, N=36, K=576, opt26=r, forms=(SEVEN[i],)))
        out.append(_case("rows", M=1, N=RB16_N, K=64, opt26=r, forms=(SEVEN[i + 1],)))
        out.append(_case("rows", M=1, N=RB32_N, K=192, opt26=r, forms=(SEVEN[i + 2],)))
    # frag: M = 3, 15, 16, K % 2048 != 0; TILES 1 by N < 16384
    Ks, Ns = (64, 192, 512, 576, 2112, 2304), (4, 12, 16, 20, 36)
    for i, K in enumerate(Ks):
        for j, M in enumerate((3, 15, 16)):
            out.append(_case("frag", M=M, N=Ns[(i + j) % 5], K=K, forms=two(3 * i + j)))
    for M, N, K in ((3, 32, 192), (15, 96, 2304), (16, 96, 576), (16, 32, 2112)):
        out.append(_case("frag", M=M, N=N, K=K, forms=("ep1",)))
    out.append(_case("frag", M=3, N=16388, K=64, forms=("bias_res", "plain")))
    out.append(_case("frag", M=15, N=16404, K=64, forms=("res_mod", "bias_gelu")))
    for i, (M, K) in enumerate(((1, 2048), (2, 2048), (16, 2048), (1, 576), (2, 576), (16, 576))):
        out.append(_case("frag", M=M, N=Ns[i % 5], K=K, opt4=2, forms=two(i + 2)))
    # staged: K % 2048 == 0, M = 3..64
    Ks, Ns = (2048, 4096, 6144), (4, 20, 36)
    for j, M in enumerate((3, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64)):
        out.append(_case("staged", M=M, N=Ns[(j + j // 3) % 3], K=Ks[j % 3], forms=two(j + 1)))
    for M, N, K in ((3, 32, 2048), (17, 96, 4096), (33, 96, 2048), (64, 32, 6144)):
        out.append(_case("staged", M=M, N=N, K=K, forms=("ep1",)))
    out.append(_case("staged", M=17, N=16388, K=2048, forms=("bias_res",)))
    # dispatch boundaries (the other side of each: staged 64 x 20 x 2048 and frag 16 x .. x 2112 above)
    out.append(_case("boundary", M=64, N=20, K=2048, forms=("bias_res",)))
    out.append(_case("boundary", M=65, N=20, K=2048, forms=("bias_res",)))
    out.append(_case("boundary", M=16, N=20, K=2112, forms=("bias_res",)))
    out.append(_case("boundary", M=17, N=20, K=2112, forms=("bias_res",)))
    out.append(_case("boundary", M=1, N=36, K=576, opt4=0, forms=("bias_res",)))
    # leading dimensions and alignment, one small case per kernel
    for M, K in ((2, 576), (15, 576), (33, 2048)):
        for a, cc in ((8, 4), (24, 12)):
            out.append(_case("ld", M=M, N=36, K=K, pad=dict(a=a, b=a, c=cc, r=cc), forms=("bias_res", "res_mod", "bias_gelu_res")))
        out.append(_case("ld", M=M, N=96, K=K, pad=dict(a=8, b=24, c=12, c2=4), forms=("ep1",)))
        out.append(_case("ld", M=M, N=96, K=K, pad=dict(a=24, b=8, c=4, c2=12), forms=("ep1",)))
    # B. uvx_gemm_rmsnorm, the row kernel's prologue
    for i, K in enumerate((64, 576, 4096, 4096 + 64, 8192, 16384)):
        out.append(_case("fused_rows", M=1, N=36, K=K, flavor=i % 2, forms=("bias",)))
        out.append(_case("fused_rows", M=2, N=36, K=K, flavor=(i + 1) % 2, forms=("bias", "bias_res"),
                         **(dict(small_row=1) if K in (576, 8192) else dict(zero_row=1) if K in (4096, 64) else {})))
    out.append(_case("fused_rows", M=1, N=RB16_N, K=576, flavor=0, forms=("plain",)))
    out.append(_case("fused_rows", M=2, N=RB16_N, K=64, flavor=1, forms=("bias_res",), small_row=0))
    out.append(_case("fused_rows", M=1, N=96, K=576, flavor=1, forms=("ep1",)))
    out.append(_case("fused_rows", M=2, N=96, K=4096 + 64, flavor=0, forms=("ep1",)))
    for i, r in enumerate((0, 4, 8, 16)):
        out.append(_case("fused_rows", M=1, N=36, K=576, opt26=r, flavor=i % 2, forms=("bias_res",)))
    out.append(_case("fused_rows", M=1, N=RB16_N, K=64, opt26=16, flavor=0, forms=("bias",)))
    out.append(_case("fused_rows", M=1, N=36, K=16384 + 64, flavor=1, forms=("bias",)))                  # past the prologue's 16384: the two launches
    # the staged kernel's prologue (option 24 = 1)
    out.append(_case("fused_staged", M=3, N=20, K=2048, flavor=0, opt24=1, forms=("bias",), small_row=1, zero_row=2))
    out.append(_case("fused_staged", M=15, N=20, K=4096, flavor=1, opt24=1, forms=("bias", "plain"), small_row=1, zero_row=2))
    out.append(_case("fused_staged", M=16, N=20, K=2048, flavor=1, opt24=1, forms=("bias_gelu",)))
    out.append(_case("fused_staged", M=16, N=20, K=4096, flavor=0, opt24=1, forms=("bias_res",), small_row=15, zero_row=7))
    out.append(_case("fused_staged", M=3, N=96, K=4096, flavor=0, opt24=1, forms=("ep1",)))
    out.append(_case("fused_staged", M=15, N=96, K=2048, flavor=1, opt24=1, forms=("ep1",)))
    out.append(_case("fused_staged", M=3, N=16388, K=2048, flavor=1, opt24=1, forms=("bias",)))
    return out


CASES = _cases()


def families(c, form):
    if fused(c):
        return ("R", "G")
    return ("S", "Sb", "R", "G")
