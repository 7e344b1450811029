"""The bf16 norm kernels (ultravox_amd/csrc/norms.hip, and qk_norm_rope_k / qk_norm_bwd_k of elementwise.hip) at their dispatch, row and column
edges: the dispatchers restated as a pure function (`served_by`), the case list, the input families, a float64 reference with per-element
bars, an f32 restatement of every kernel with its own summation order, and the off-by-one mutations of that restatement.
test_norm_edges_cpu.py proves the harness on the restatement; test_norm_edges_gpu.py holds the kernels to it.

Entries (`c["entry"]`): "ln" uvx_layernorm, "ln_bwd" uvx_layernorm_bwd, "rms" uvx_rmsnorm, "rms_bwd" uvx_rmsnorm_bwd (modes dx, dx_add, dw,
dx_dw), "qk" uvx_qk_norm_rope, "qk_bwd" uvx_qk_norm_bwd, "gemma" the row norm of either flavor as uvx_gemm_rmsnorm runs it at M = 3 into norm_out.

Kernels and their summation orders (all sums in f32, `s += a * b` contracted to an fma):
  block kernels (layernorm_fwd_k, layernorm_bwd_k, rmsnorm_fwd_k, rmsnorm_fwd_reg_k<NV>, rmsnorm_bwd_k<MV>): thread t of th sums the 8-element
          vectors t, t + th, .. in order, each vector's elements in order; wave_sum's xor butterfly 32, 16, .. 1 (a balanced tree); block_sum's
          ascending sum over the waves.  th = norm_threads(cols) = 64 .. 256 (the RMSNorm backward: always 256).
  wave kernels (layernorm_fwd_wave_k<NV>, rmsnorm_fwd_wave_k<NV>): lane l of a row's wave sums the vectors l, l + 64, ..; the butterfly alone.
  per-head kernels: qk_norm_rope_k - a lane holds vector j of the head's first half and vector j of its second half, D / 16 lanes share the sum
          through xor 1, 2, ..; qk_norm_bwd_k - one vector per lane, D / 8 lanes.
  the weight gradient of uvx_rmsnorm_bwd: ONE block walks the rows in order, a thread adds g * round(x r) of its columns row by row.

Families: R - randn at the scales the older tests use (the arithmetic family); P - "one vector carries the row": noise of 2^-6 and a spike of 8 in
one 8-element vector (one run per edge vector, `variants`), in dy as well for the backwards; Z - R with a constant first row (0.5: every partial
sum of it is exact) and an all-zero last row.  In every family the flavor-0 forwards get a power-of-two weight in the few columns where the inner
rounding is undecided at f32 precision (`_decide_inner_rounding` says why): the one-ulp cap against the restatement could not hold there otherwise.

Bars (`reference`): every bf16 rounding on a kernel's path adds half an ulp of the magnitude it rounds (`hu`), propagated to the output by the
factor it is multiplied with afterwards; the f32 statistics add acc(n) = 4 (sqrt(n) + 4) 2^-24 of the element's scale - the float64 sum of the
magnitudes of the terms it is made of - the form and constant of test_f32_kernels_gpu.py.  The derivations stand next to each bar."""
import math

import torch

F64 = torch.float64
RMS_EPS = float(torch.tensor(1e-6, dtype=torch.float32))
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
CANARY16 = 0x7F91        # a bf16 NaN: a canary read as data makes its output non-finite
HEAD = 64                # canary elements in front of every operand
MAX_BWD_COLS = 12288
FAMILIES = ("R", "P", "Z")


def bf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def f32r(x):
    return x.to(torch.float32).to(F64)


def ulp_bf16(m):
    """spacing of bf16 at magnitude m (0 at 0)"""
    e = torch.floor(torch.log2(m.abs().clamp_min(2.0 ** -126)))
    return torch.where(m == 0, torch.zeros_like(m), torch.exp2(e - 7.0))


def hu(m):
    """half a bf16 ulp at magnitude m, m raised by 2^-7 so that a computed value just across a binade boundary from the exact one is covered"""
    return 0.5 * ulp_bf16(m.abs() * (1.0 + 2.0 ** -7))


def acc(n, c=4.0):
    return c * (math.sqrt(n) + 4.0) * 2.0 ** -24


# ------------------------------------------------------------------ the dispatchers, restated
def norm_threads(cols):
    t = (cols // 8 + 63) // 64 * 64
    return min(max(t, 64), 256)


def served_by(entry, rows, cols, two_pass=0, mode=None):
    """layernorm_fwd, layernorm_bwd, rms_launch, rms_bwd_launch, qk_norm_rope, qk_norm_bwd for bf16 through the public entry points (cols = head_dim for
    the per-head ones) -> the kernel instantiation as a tuple, "rejected" (ValueError, nothing written) or "noop"."""
    if entry in ("qk", "qk_bwd"):
        if cols not in (64, 128, 256):
            return "rejected"
        if rows == 0:
            return "noop"
        return ("qk_norm_rope_k", cols // 16) if entry == "qk" else ("qk_norm_bwd_k", cols // 8)
    if cols % 8 or (entry == "rms_bwd" and cols > MAX_BWD_COLS):
        return "rejected"
    if rows == 0:
        return "noop"
    th = norm_threads(cols)
    if entry == "ln":
        return ("layernorm_fwd_wave_k", cols // 512) if cols in (512, 1024, 2048, 4096) else ("layernorm_fwd_k", th)
    if entry == "ln_bwd":
        return ("layernorm_bwd_k", th)
    if entry in ("rms", "gemma"):
        if cols in (512, 1024, 2048):
            return ("rmsnorm_fwd_wave_k", cols // 512)
        if cols <= th * 8 * 4 and rows <= 512 and not two_pass:
            return ("rmsnorm_fwd_reg_k", 1 if cols <= th * 8 else 2 if cols <= th * 16 else 4, th)
        return ("rmsnorm_fwd_k", th)
    if entry == "rms_bwd":
        want_dw = mode in ("dw", "dx_dw")
        return ("rmsnorm_bwd_k", mode != "dw", want_dw, 1 if cols <= 2048 else 2 if cols <= 4096 else 6, "reload" if want_dw else "cached")
    raise KeyError(entry)


def reachable():
    """every bf16 instantiation the dispatchers can launch through these entry points"""
    out = {("layernorm_fwd_wave_k", n) for n in (1, 2, 4, 8)} | {("rmsnorm_fwd_wave_k", n) for n in (1, 2, 4)}
    out |= {(k, th) for k in ("layernorm_fwd_k", "layernorm_bwd_k", "rmsnorm_fwd_k") for th in (64, 128, 192, 256)}
    out |= {("rmsnorm_fwd_reg_k", 1, th) for th in (64, 128, 192, 256)} | {("rmsnorm_fwd_reg_k", 2, 256), ("rmsnorm_fwd_reg_k", 4, 256)}
    out |= {("rmsnorm_bwd_k", dx, dw, mv, "reload" if dw else "cached") for dx, dw in ((True, False), (True, True), (False, True)) for mv in (1, 2, 6)}
    out |= {("qk_norm_rope_k", n) for n in (4, 8, 16)} | {("qk_norm_bwd_k", n) for n in (8, 16, 32)}
    return out


def step_of(c):
    """vectors per sweep of the kernel that serves the case (two-pass option off): the distance between a thread's consecutive vectors"""
    if c["entry"] == "rms_bwd":
        return 256
    k = served_by(c["entry"], c["rows"], c["cols"])
    return 64 if "wave" in k[0] else k[-1]


# ------------------------------------------------------------------ cases
RMS_COLS = (8, 504, 512, 520, 1024, 1536, 1544, 2040, 2048, 2056, 4096, 4104, 6144, 6152, 8192, 8200, 12288)
RMS_BWD_COLS = (8, 2040, 2048, 2056, 4096, 4104, 8192, 12288)
RMS_BWD_MODES = ("dx", "dx_add", "dw", "dx_dw")
LN_WAVE_COLS, LN_BLOCK_COLS = (512, 1024, 2048, 4096), (8, 384, 504, 520, 1280, 2056, 4104, 5120)
LN_BWD_COLS = (8, 384, 512, 1024, 1280, 2056, 5120)
GEMMA_K = (512, 576, 4096, 8192, 8256)
HEAD_DIMS, HEADS, QK_B, QK_T = (64, 128, 256), ((1, 1), (3, 2), (5, 1)), 3, 5


def case_id(c):
    if c["entry"] in ("qk", "qk_bwd"):
        return f"{c['entry']}-d{c['cols']}-h{c['Hq']}x{c['Hkv']}-f{c['flavor']}" + ("-raw" if c.get("raw") else "")
    tail = f"-{c['mode']}" if "mode" in c else f"-f{c['flavor']}" if c["entry"] == "gemma" else "-add" if c.get("add") else ""
    return f"{c['entry']}-{c['rows']}x{c['cols']}{tail}"


def _cases():
    out = []
    for cols in RMS_COLS:
        for rows in (1, 3, 4, 5) + ((9,) if cols in (512, 1024, 2048) else ()):
            out.append(dict(entry="rms", rows=rows, cols=cols))
    out += [dict(entry="rms", rows=512, cols=4096), dict(entry="rms", rows=513, cols=4096), dict(entry="rms", rows=513, cols=1024)]
    for cols in RMS_BWD_COLS:
        for rows in (1, 17):
            for mode in RMS_BWD_MODES:
                out.append(dict(entry="rms_bwd", rows=rows, cols=cols, mode=mode))
    for cols in LN_WAVE_COLS:
        out += [dict(entry="ln", rows=rows, cols=cols) for rows in (1, 3, 4, 5, 9)]
    for cols in LN_BLOCK_COLS:
        out += [dict(entry="ln", rows=rows, cols=cols) for rows in (1, 5)]
    for cols in LN_BWD_COLS:
        out += [dict(entry="ln_bwd", rows=rows, cols=cols, add=add) for rows in (1, 5) for add in (False, True)]
    for K in GEMMA_K:
        out += [dict(entry="gemma", rows=3, cols=K, flavor=f) for f in (0, 1)]
    for D in HEAD_DIMS:
        for Hq, Hkv in HEADS:
            geo = dict(rows=QK_B * QK_T, cols=D, Hq=Hq, Hkv=Hkv, T=QK_T, ld=(Hq + 2 * Hkv) * D + 8)
            out += [dict(geo, entry="qk", flavor=f, raw=raw) for f in (0, 1) for raw in (False, True)]
            out += [dict(geo, entry="qk_bwd", flavor=f) for f in (0, 1)]
    for i, c in enumerate(out):
        c["seed"] = 7919 * i + c["rows"] + 3 * c["cols"]
    return out


CASES = _cases()
REJECTED_COLS = 12                      # cols % 8 != 0 in each row-norm entry point; rms_bwd also MAX_BWD_COLS + 8; head_dim 96; ld % 8 != 0


def cases(entry):
    return [c for c in CASES if c["entry"] == entry]


def variants(c, family):
    """the runs of a family: (None,) for R and Z; for P one per edge vector - the first and the last vector of the row and the vectors on either side of
    every sweep boundary inside it (per head: (head, vector) for the first and last vector of the first and last q and k head)"""
    if family != "P":
        return (None,)
    if c["entry"] in ("qk", "qk_bwd"):
        heads = sorted({0, c["Hq"] - 1, c["Hq"], c["Hq"] + c["Hkv"] - 1})
        return tuple((h, v) for h in heads for v in (0, c["cols"] // 8 - 1))
    nvec, step = c["cols"] // 8, step_of(c)
    edge = {0, nvec - 1}
    for k in range(step, nvec, step):
        edge |= {k - 1, k}
    return tuple(sorted(edge))


# ------------------------------------------------------------------ inputs
def rope_table(T, D):
    """[T, D / 2, 2] f32 (cos, sin) whose values are bf16 numbers: the kernel's rounding of the table is then the identity"""
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=F64) / D)
    ang = torch.arange(T, dtype=F64)[:, None] * inv[None, :]
    return torch.stack((bf(torch.cos(ang)), bf(torch.sin(ang))), -1).to(torch.float32).contiguous()


def make_inputs(c, family, variant=None, device="cpu"):
    """{name: tensor}: bf16 operands (f32 `cs`) of one run, drawn on the CPU from the case's seed"""
    gen = torch.Generator().manual_seed(c["seed"] * 31 + FAMILIES.index(family) * 7 + (hash(variant) % 1009 if variant is not None else 0))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    entry, rows, cols = c["entry"], c["rows"], c["cols"]
    per_head = entry in ("qk", "qk_bwd")
    width = (c["Hq"] + c["Hkv"]) * cols if per_head else cols

    def body(scale, shift=0.0):
        if family == "P":
            x = 2.0 ** -6 * rn(rows, width)
            lo = (variant[0] * cols + variant[1] * 8) if per_head else variant * 8
            x[:, lo:lo + 8] = 8.0 * (0.75 + 0.5 * torch.rand(rows, 8, generator=gen, dtype=F64)) * (1.0 - 2.0 * torch.randint(0, 2, (rows, 1), generator=gen).to(F64))
            return x      # (one sign per row: neither the spike's sum nor sum(dy w x) cancels)
        x = scale * rn(rows, width) + shift
        if family == "Z":
            x[rows - 1] = 0.0
            if rows >= 2:
                x[0] = 0.5
        return x

    o = {}
    if entry in ("rms", "gemma", "rms_bwd"):
        o["x"], o["w"] = body(1.5), 0.5 + 0.2 * rn(cols)
        if entry == "gemma":
            o["B"] = rn(8, cols)
    elif entry in ("ln", "ln_bwd"):
        o["x"], o["w"] = body(1.0, 0.3), 0.5 + 0.2 * rn(cols)
        if entry == "ln":
            b = 0.3 * rn(cols)
            o["b"] = torch.where(b.abs() < 0.125, torch.where(b < 0, -0.125, 0.125).to(F64), b) if family == "Z" else b
    if entry in ("rms_bwd", "ln_bwd"):
        o["dy"] = body(1.0) if family == "P" else rn(rows, cols)
        if c.get("mode") == "dx_add" or c.get("add"):
            o["add"] = rn(rows, cols)
    if per_head:
        H, ld = c["Hq"] + c["Hkv"], c["ld"]
        o["wq"], o["wk"] = 0.5 + 0.2 * rn(cols), 0.5 + 0.2 * rn(cols)
        if entry == "qk":
            o["qkv"] = torch.cat((body(1.0), rn(rows, ld - H * cols)), 1)       # q | k, then v and the pad (the pad is made canaries by the GPU test)
        else:
            o["raw"] = body(1.0)
            g = body(1.0) if family == "P" else rn(rows, width)
            o["dqkv"] = torch.cat((g, rn(rows, ld - H * cols)), 1)
    o = {k: v.to(torch.bfloat16) for k, v in o.items()}
    if c.get("flavor", 0) == 0 and entry in ("rms", "gemma", "qk"):
        _decide_inner_rounding(c, o)
    o = {k: v.to(device) for k, v in o.items()}
    if entry == "qk":
        o["cs"] = rope_table(c["T"], cols).to(device)
    return o


TIP = 2.0 ** -20       # covers the f32 sum of squares in any order, rsqrtf and one f32 product (gemm_skinny_edge_util.TIP)


def _decide_inner_rounding(c, o):
    """Flavor 0 rounds twice, round(w * round(x rstd)).  Where x rstd lies within TIP of a bf16 rounding boundary the kernel and the restatement may
    legitimately round it apart, by one ulp of x rstd; times a weight of mantissa m that is m ulps of the output (two after the store's rounding) - over
    the one-ulp cap with nothing wrong.  The weight of every COLUMN that has such an element is therefore made the nearest power of two: the
    disagreement is then exactly one ulp of the output.  (5 rows: 2 columns in a thousand; 513 rows: one in six.)"""
    per_head = c["entry"] == "qk"
    x = (_heads(o["qkv"], c) if per_head else o["x"]).to(F64)
    v = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + RMS_EPS)
    tip = bf(v * (1.0 + TIP)) != bf(v * (1.0 - TIP))
    pow2 = lambda w: (torch.sign(w.to(F64)) * torch.exp2(torch.round(torch.log2(w.to(F64).abs())))).to(torch.bfloat16)
    if per_head:
        for name, sel in (("wq", tip[:, :c["Hq"]]), ("wk", tip[:, c["Hq"]:])):
            cols = sel.any(0).any(0)
            o[name] = torch.where(cols, pow2(o[name]), o[name])
    else:
        o["w"] = torch.where(tip.any(0), pow2(o["w"]), o["w"])


# ------------------------------------------------------------------ the float64 reference and the bars
def _stored(ref, rest):
    """bar of a stored element: `rest` (everything before the store) and the store's own half ulp, taken at the largest magnitude the computed
    value can have"""
    return rest + hu(ref.abs() + rest)


def _rms_ref(x, w, eps, flavor, n):
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    v = x * r
    weff = 1.0 + w if flavor else w
    y = v * weff
    # flavor 0: round(w * round(x r)) - the inner rounding's half ulp of x r, times |w|, and the store; flavor 1: the store alone.
    # f32: the sum of squares, rsqrtf and the products move y by acc(n) of its size
    rest = acc(n) * y.abs() + (0.0 if flavor else w.abs() * hu(v))
    return y, _stored(y, rest), acc(n) * y.abs()


def _rms_bwd_ref(x, w, dy, add, eps, flavor, n, want_dw=False, rows_sum=True):
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    gw = dy * (1.0 + w if flavor else w)
    dx = r * gw - x * r.pow(3) * (gw * x).mean(-1, keepdim=True)
    scale = r * gw.abs() + x.abs() * r.pow(3) * (gw * x).abs().mean(-1, keepdim=True)
    if add is not None:
        dx, scale = dx + add, scale + add.abs()
    # one rounding, the store; every term before it is f32
    out = {"dx": (dx, _stored(dx, acc(n) * scale), acc(n) * scale)}
    if want_dw:
        rows = x.shape[0]
        dw = (dy * x * r).sum(0)
        sw = (dy * x * r).abs().sum(0)
        # dw = sum over rows of g * round(x r): each row's rounding of x r moves its term by |g| hu(x r); the f32 row sum (sqrt(rows)) on top of
        # the statistics' sqrt(cols), as test_f32_kernels_gpu.py's barw.  dw is stored in f32: no store term
        noise = 4.0 * (math.sqrt(n) + math.sqrt(rows) + 4.0) * 2.0 ** -24 * sw
        out["dw"] = (dw, (dy.abs() * hu(x * r)).sum(0) + noise, noise)
    return out


def _ln_stats(x, eps):
    mu = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    # x_hat = (x - mean) rstd is a difference: an f32 error of the mean enters at |mean| rstd, so its scale is (|x| + |mean|) rstd
    return mu, rstd, (x - mu) * rstd, (x.abs() + mu.abs()) * rstd


def _ln_ref(x, w, b, eps, n):
    mu, rstd, xh, xs = _ln_stats(x, eps)
    y = xh * w + b
    scale = xs * w.abs() + b.abs()
    return y, _stored(y, acc(n) * scale), acc(n) * scale     # one rounding, the store


def _ln_bwd_ref(x, w, dy, add, eps, n):
    mu, rstd, xh, xs = _ln_stats(x, eps)
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    scale = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xs * (g.abs() * xs).mean(-1, keepdim=True))
    if add is not None:
        dx, scale = dx + add, scale + add.abs()
    return dx, _stored(dx, acc(n) * scale), acc(n) * scale   # one rounding, the store


def _heads(t, c):
    H = c["Hq"] + c["Hkv"]
    return t[:, :H * c["cols"]].reshape(t.shape[0], H, c["cols"])


def _head_w(inp, c, swap=False):
    wq, wk = inp["wq"].to(F64), inp["wk"].to(F64)
    return torch.cat((wq.expand(c["Hq"], -1), (wq if swap else wk).expand(c["Hkv"], -1)), 0)[None]      # [1, H, D]


def _qk_ref(c, inp):
    D, flavor = c["cols"], c["flavor"]
    x, w = _heads(inp["qkv"].to(F64), c), _head_w(inp, c)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + RMS_EPS)
    v = x * r
    n = v * (1.0 + w if flavor else w)
    # the normalised head: as the row norm (flavor 0: inner rounding times |w|; f32 statistics over D), then ITS store rounding - the kernel rounds the
    # normalised value to bf16 before it rotates it
    e = acc(D) * n.abs() + (0.0 if flavor else w.abs() * hu(v))
    e = _stored(n, e)
    pos = torch.arange(x.shape[0], device=x.device) % c["T"]
    cs = inp["cs"].to(F64)[pos][:, None]                    # [rows, 1, D / 2, 2]
    co, si = cs[..., 0], cs[..., 1]
    lo, hi, elo, ehi = n[..., :D // 2], n[..., D // 2:], e[..., :D // 2], e[..., D // 2:]
    out, bar, noise, mag = [], [], [], []
    for a, ea, b_, eb, sgn in ((lo, elo, hi, ehi, -1.0), (hi, ehi, lo, elo, 1.0)):
        y = a * co + sgn * b_ * si
        # RoPE: round(round(a cos) + round(-+ b sin)): the incoming errors times |cos|, |sin|, half an ulp of each product, and the store
        rest = ea * co.abs() + eb * si.abs() + hu(a.abs() * co.abs() + ea * co.abs()) + hu(b_.abs() * si.abs() + eb * si.abs())
        out.append(y), bar.append(_stored(y, rest)), noise.append(acc(D) * ((a * co).abs() + (b_ * si).abs())), mag.append(torch.maximum((a * co).abs(), (b_ * si).abs()))
    cat = lambda t: torch.cat(t, -1).reshape(x.shape[0], -1)
    res = {"qk": (cat(out), cat(bar), cat(noise), cat(mag))}
    if c.get("raw"):
        z = torch.zeros_like(res["qk"][0])
        res["raw"] = (x.reshape(x.shape[0], -1), z, z)      # a copy: bit for bit
    return res


def _qk_bwd_ref(c, inp):
    D = c["cols"]
    x, g, w = _heads(inp["raw"].to(F64), c), _heads(inp["dqkv"].to(F64), c), _head_w(inp, c)
    sh = x.shape
    o = _rms_bwd_ref(x.reshape(-1, D), w.expand(sh).reshape(-1, D), g.reshape(-1, D), None, RMS_EPS, c["flavor"], D)["dx"]
    return {"dqk": tuple(t.reshape(sh[0], -1) for t in o)}


def reference(c, inp):
    """{output: (float64 value, per-element bar, the f32 noise of the element: acc * scale[, the largest rounded magnitude on the element's path, where
    that is not the output's own: the two products of a RoPE output])}"""
    e = c["entry"]
    f = lambda k: inp[k].to(F64) if k in inp else None
    if e in ("rms", "gemma"):
        return {"y": _rms_ref(f("x"), f("w"), RMS_EPS, c.get("flavor", 0), c["cols"])}
    if e == "rms_bwd":
        o = _rms_bwd_ref(f("x"), f("w"), f("dy"), f("add"), RMS_EPS, 0, c["cols"], want_dw=c["mode"] in ("dw", "dx_dw"))
        if c["mode"] == "dw":
            del o["dx"]
        return o
    if e == "ln":
        return {"y": _ln_ref(f("x"), f("w"), f("b"), LN_EPS, c["cols"])}
    if e == "ln_bwd":
        return {"dx": _ln_bwd_ref(f("x"), f("w"), f("dy"), f("add"), LN_EPS, c["cols"])}
    return _qk_ref(c, inp) if e == "qk" else _qk_bwd_ref(c, inp)


# ------------------------------------------------------------------ the kernels' summation orders in f32
def _in_order(x):
    """0.f + x[.., 0] + x[.., 1] + .. in f32 (x: exact products in float64, so each step is an fma)"""
    t = torch.zeros_like(x[..., 0])
    for i in range(x.shape[-1]):
        t = f32r(t + x[..., i])
    return t


def _fold(x):
    """wave_sum over the last axis (64 lanes): l with l ^ 32, then ^ 16, .. ^ 1"""
    h = x.shape[-1] // 2
    while h >= 1:
        x = f32r(x[..., :h] + x[..., h:2 * h])
        h //= 2
    return x[..., 0]


def _pairs(x, stop=1):
    """the per-head butterfly over the last axis: l with l ^ 1, then ^ 2, ..; stop = 2: half the lanes only -> [.., stop] (every lane of a group of
    lanes that met holds that group's sum)"""
    while x.shape[-1] > stop:
        x = f32r(x[..., 0::2] + x[..., 1::2])
    return x


def _row_sum(terms, step, cnt):
    """[rows, cols] exact products -> [rows]: thread t of `step` sums its vectors t, t + step, .. in order, butterfly per wave, waves in order;
    cnt [cols / 8]: how often a vector enters (1 unless a mutation says otherwise)"""
    rows, cols = terms.shape
    terms = terms * cnt.repeat_interleave(8).to(terms.device)
    ns = -(-cols // (step * 8))
    pad = torch.zeros(rows, ns * step * 8, dtype=F64, device=terms.device)
    pad[:, :cols] = terms
    per_thread = _in_order(pad.reshape(rows, ns, step, 8).permute(0, 2, 1, 3).reshape(rows, step, ns * 8))
    return _in_order(_fold(per_thread.reshape(rows, step // 64, 64)))[:, None]


MUTATIONS = ("last_vec_drop", "sweep_first_twice", "mean_padded", "nv_one_short", "row_guard", "ln_var_about_0", "dx_add_ignored", "coef_without_cols",
             "dw_last_row", "butterfly_half", "k_with_wq", "pos_row_div_T", "raw_after_norm")
_ONE_SHORT = {2: 1, 4: 2, 8: 4, 6: 2}


def _kernel(c, two_pass=0):
    return served_by(c["entry"], c["rows"], c["cols"], two_pass, c.get("mode"))


def _nv(k):
    """NV / MV of an instantiation that has one"""
    if k[0] in ("layernorm_fwd_wave_k", "rmsnorm_fwd_wave_k", "rmsnorm_fwd_reg_k"):
        return k[1]
    return k[3] if k[0] == "rmsnorm_bwd_k" else None


def touches(mut, c):
    """whether the mutation has a meaning on the case"""
    e, k = c["entry"], _kernel(c)
    row_norm = e not in ("qk", "qk_bwd")
    return {"last_vec_drop": True, "sweep_first_twice": row_norm,
            "mean_padded": row_norm and c["cols"] % (step_of(c) * 8) != 0,
            "nv_one_short": (_nv(k) or 1) > 1, "row_guard": "wave" in k[0], "ln_var_about_0": e in ("ln", "ln_bwd"),
            "dx_add_ignored": c.get("mode") == "dx_add" or bool(c.get("add")), "coef_without_cols": (e == "rms_bwd" and c["mode"] != "dw") or e == "qk_bwd",
            "dw_last_row": c.get("mode") in ("dw", "dx_dw"), "butterfly_half": not row_norm, "k_with_wq": not row_norm, "pos_row_div_T": e == "qk",
            "raw_after_norm": e == "qk" and bool(c.get("raw"))}[mut]


def _plan(mut, cols, step, nv):
    """-> (cnt [nvec]: how often each vector enters the sums, written [cols]: the columns that get stored, the width the means divide by)"""
    nvec = cols // 8
    cnt, written, width = torch.ones(nvec, dtype=F64), torch.ones(nvec, dtype=torch.bool), cols
    if mut == "last_vec_drop":
        cnt[-1] = 0
    elif mut == "sweep_first_twice":
        cnt[(nvec - 1) // step * step] = 2
    elif mut == "mean_padded":
        width = -(-cols // (step * 8)) * step * 8
    elif mut == "nv_one_short":
        cnt[_ONE_SHORT[nv] * step:] = 0
        written[_ONE_SHORT[nv] * step:] = False
    return cnt, written.repeat_interleave(8), width


def _unwritten(y, written, c, k, mut):
    y = y.clone()
    y[:, ~written.to(y.device)] = float("nan")
    if mut == "row_guard":           # `row >= rows - 1`: the last row keeps its canary
        y[-1] = float("nan")
    return y


def _rsqrt(v):
    return f32r(1.0 / torch.sqrt(v))


def _re_rms(c, inp, k, mut):
    x, w, flavor, cols = inp["x"].to(F64), inp["w"].to(F64), c.get("flavor", 0), c["cols"]
    step = 64 if "wave" in k[0] else k[-1]
    cnt, written, width = _plan(mut, cols, step, _nv(k))
    rstd = _rsqrt(f32r(f32r(_row_sum(x * x, step, cnt) / width) + RMS_EPS))
    v = f32r(x * rstd)
    y = bf(f32r(w * bf(v))) if flavor == 0 else bf(f32r(v * f32r(1.0 + w)))
    return {"y": _unwritten(y, written, c, k, mut)}


def _re_rms_bwd(c, inp, k, mut):
    x, w, g, cols, rows = inp["x"].to(F64), inp["w"].to(F64), inp["dy"].to(F64), c["cols"], c["rows"]
    cnt, written, width = _plan(mut, cols, 256, k[3])
    gw = f32r(g * w)
    s1, s2 = _row_sum(x * x, 256, cnt), _row_sum(gw * x, 256, cnt)
    r = _rsqrt(f32r(f32r(s1 / width) + RMS_EPS))
    coef = f32r(f32r(f32r(r * r) * r) * s2)
    if mut != "coef_without_cols":
        coef = f32r(coef / width)
    out = {}
    if k[1]:
        o = f32r(f32r(f32r(r * g) * w) - x * coef)
        if "add" in inp and mut != "dx_add_ignored":
            o = f32r(inp["add"].to(F64) + o)
        out["dx"] = _unwritten(bf(o), written, c, k, mut)
    if k[2]:
        t = g * bf(f32r(x * r))                              # one block, the rows in order; a thread's dwacc += g * round(x r)
        if mut == "dw_last_row":
            t = t[:-1]
        dw = _in_order(t.t().contiguous()) if t.shape[0] else torch.zeros(cols, dtype=F64, device=x.device)
        out["dw"] = _unwritten(dw[None], written, c, k, None)[0]
    return out


def _re_ln_stats(x, step, cnt, width, mut):
    mean = f32r(_row_sum(x, step, cnt) / width)
    d = f32r(x - mean)
    dv = x if mut == "ln_var_about_0" else d
    return mean, d, _rsqrt(f32r(f32r(_row_sum(dv * dv, step, cnt) / width) + LN_EPS))


def _re_ln(c, inp, k, mut):
    x, w, b = inp["x"].to(F64), inp["w"].to(F64), inp["b"].to(F64)
    step = 64 if "wave" in k[0] else k[-1]
    cnt, written, width = _plan(mut, c["cols"], step, _nv(k))
    mean, d, rstd = _re_ln_stats(x, step, cnt, width, mut)
    return {"y": _unwritten(bf(f32r(f32r(d * rstd) * w + b)), written, c, k, mut)}


def _re_ln_bwd(c, inp, k, mut):
    x, w, g = inp["x"].to(F64), inp["w"].to(F64), inp["dy"].to(F64)
    step = k[-1]
    cnt, written, width = _plan(mut, c["cols"], step, None)
    mean, d, rstd = _re_ln_stats(x, step, cnt, width, mut)
    gw = f32r(g * w)
    a = f32r(_row_sum(gw, step, cnt) / width)
    b = f32r(_row_sum(f32r(gw * d) * rstd, step, cnt) / width)
    o = f32r(rstd * f32r(f32r(gw - a) - f32r(f32r(d * rstd) * b)))
    if "add" in inp and mut != "dx_add_ignored":
        o = f32r(inp["add"].to(F64) + o)
    return {"dx": _unwritten(bf(o), written, c, k, mut)}


def _head_sum(per_lane, mut):
    """[.., lanes] -> [.., lanes]: every lane's view of the head's sum after the butterfly"""
    lanes = per_lane.shape[-1]
    s = _pairs(per_lane, 2 if mut == "butterfly_half" else 1)
    return s.repeat_interleave(lanes // s.shape[-1], -1)


def _re_qk(c, inp, k, mut):
    D, flavor, T = c["cols"], c["flavor"], c["T"]
    x, w = _heads(inp["qkv"].to(F64), c), _head_w(inp, c, swap=mut == "k_with_wq")
    rows, H = x.shape[:2]
    lo, hi = x[..., :D // 2].reshape(rows, H, D // 16, 8), x[..., D // 2:].reshape(rows, H, D // 16, 8)
    drop = torch.ones(D // 16, 1, dtype=F64, device=x.device)
    if mut == "last_vec_drop":
        drop[-1] = 0
    ss = _head_sum(_in_order(f32r(lo * lo + hi * hi * drop)), mut)                       # ss += lo^2 + hi^2 per element, D / 16 lanes
    rstd = _rsqrt(f32r(f32r(ss / D) + RMS_EPS))[..., None]                               # [rows, H, D / 16, 1]
    wl, wh = w[..., :D // 2].reshape(1, H, D // 16, 8), w[..., D // 2:].reshape(1, H, D // 16, 8)
    norm = (lambda v, wv: bf(f32r(wv * bf(f32r(v * rstd))))) if flavor == 0 else (lambda v, wv: bf(f32r(f32r(v * rstd) * f32r(1.0 + wv))))
    nl, nh = norm(lo, wl), norm(hi, wh)
    r = torch.arange(rows, device=x.device)
    cs = inp["cs"].to(F64)[(r // T) % T if mut == "pos_row_div_T" else r % T].reshape(rows, 1, D // 16, 8, 2)
    co, si = bf(cs[..., 0]), bf(cs[..., 1])
    olo, ohi = bf(f32r(bf(f32r(nl * co)) + bf(f32r(-nh * si)))), bf(f32r(bf(f32r(nh * co)) + bf(f32r(nl * si))))
    flat = lambda a, b: torch.cat((a.reshape(rows, H, D // 2), b.reshape(rows, H, D // 2)), -1).reshape(rows, H * D)
    out = {"qk": flat(olo, ohi)}
    if c.get("raw"):
        out["raw"] = flat(nl, nh) if mut == "raw_after_norm" else x.reshape(rows, H * D)
    return out


def _re_qk_bwd(c, inp, k, mut):
    D, flavor = c["cols"], c["flavor"]
    x, g, w = _heads(inp["raw"].to(F64), c), _heads(inp["dqkv"].to(F64), c), _head_w(inp, c, swap=mut == "k_with_wq")
    rows, H = x.shape[:2]
    v8 = lambda t: t.reshape(t.shape[0], H, D // 8, 8)
    x, g, w = v8(x), v8(g), v8(f32r(1.0 + w) if flavor else w)
    drop = torch.ones(D // 8, 1, dtype=F64, device=x.device)
    if mut == "last_vec_drop":
        drop[-1] = 0
    gw = f32r(g * w)
    s1, s2 = _head_sum(_in_order(x * x * drop), mut)[..., None], _head_sum(_in_order(gw * x * drop), mut)[..., None]
    r = _rsqrt(f32r(f32r(s1 / D) + RMS_EPS))
    coef = f32r(f32r(f32r(r * r) * r) * s2)
    if mut != "coef_without_cols":
        coef = f32r(coef / D)
    return {"dqk": bf(f32r(f32r(f32r(r * g) * w) - x * coef)).reshape(rows, H * D)}


def restatement(c, inp, two_pass=0, mut=None):
    """{output: the kernel's arithmetic in f32, rounded where the kernel rounds - bf16 values (dw: f32) in float64; NaN where nothing was stored}.
    `mut`: one of MUTATIONS, applied to the served kernel"""
    k = _kernel(c, two_pass)
    f = {"rms": _re_rms, "gemma": _re_rms, "rms_bwd": _re_rms_bwd, "ln": _re_ln, "ln_bwd": _re_ln_bwd, "qk": _re_qk, "qk_bwd": _re_qk_bwd}[c["entry"]]
    return f(c, inp, k, mut)


# ------------------------------------------------------------------ comparisons
def bar_units(got, ref):
    """largest |got - value| / bar over the elements (inf where a bar of 0 is missed or the value is not finite)"""
    val, bar = ref[0], ref[1]
    err = (got.to(F64) - val).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    u = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    return u.max().item() if u.numel() else 0.0


def flips(got, want, noise, mag=None):
    """bf16 outputs against the restatement -> (share of elements whose bits differ, the largest difference in bf16 ulps).  A difference is counted
    in ulps of the largest rounded magnitude on the element's path - the larger of the two values, or `mag` (a RoPE output is the rounded sum of two
    rounded products and may be far smaller than either) - after the element's f32 noise (acc * scale, the bars' term) is taken off: an output whose
    terms cancel carries the f32 rounding of full-sized terms, which is no rounding point"""
    g, w = got.to(F64), want.to(F64)
    differ = g != w
    at = torch.maximum(g.abs(), w.abs())
    ulps = ((g - w).abs() - noise).clamp_min(0.0) / ulp_bf16(at if mag is None else torch.maximum(at, mag)).clamp_min(1e-300)
    ulps = torch.where(differ, ulps, torch.zeros_like(ulps))
    return differ.to(F64).mean().item(), ulps.max().item()


def guarded(t, tail):
    """t inside a flat buffer of canaries (bf16: CANARY16; f32: NaN): HEAD elements in front, `tail` after -> (buffer, the view of t's shape)"""
    n = HEAD + t.numel() + tail
    if t.dtype == torch.bfloat16:
        buf = torch.full((n,), CANARY16, dtype=torch.int16, device=t.device).view(torch.bfloat16)
    else:
        buf = torch.full((n,), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[HEAD:HEAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
