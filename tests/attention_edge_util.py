"""float64 reference, per-element bars, edge-loud inputs and mask mutations for the bf16 attention kernels
(uvx_attention_fwd / uvx_attention_bwd through ops.attention / ops.attention_bwd).

Used by test_attention_edges_cpu.py (which proves this harness on the CPU) and test_attention_edges_gpu.py (which holds
the kernels to it).  Everything here is plain torch and runs on whichever device its inputs live on.

Layouts (the ABI's): q [B, T, Hq, D], k / v [B, T, Hkv, D], o / dO [B, T, Hq * D], lse [B, Hq, T] (natural log here; the ABI
returns log2), dq like q, dk / dv like k.  A mask is a bool [B, T(query), T(key)] shared by the heads.

bf16 rounding points of the kernels (ultravox_amd/csrc/attention.hip), u = 2^-8 the bf16 unit roundoff.  Every bar below is
1.25 * (number of roundings on the path) * u * E with E the sum of the absolute values of the terms of that element; the
1.25 covers the f32 summation order and v_exp_f32 (about 1e-6 each, against u = 3.9e-3).

  o    attn_fwd_k.  The row sum l_run adds the f32 exp2 values (:436-442) BEFORE they are packed to bf16 for P.V (pack8, :452),
       so l - and with it lse (:500) - is f32-accurate.  Roundings: P (:452) and the output (f2bf, :497).
       bar 1.25 * 2u * E_o,  E_o = sv = P.|V|.
  lse  f32 throughout from exact inputs: the f32 bar of test_f32_attention_forward_backward,
       4 (sqrt D + sqrt T + 4) 2^-24 relative to |lse| + 4 sc sqrt D.
  dv   attn_bwd_dkdv_k: P packed to bf16 (pack8, :680), the output (:759); under GQA (Hq != Hkv) the per-query-head partial in
       dkv_part is bf16 (:744) and gqa_reduce_k sums the partials in f32 (:1265) and rounds the sum (:1286).
       attn_bwd_fused_k: P (:1127), partial (:1148), output (:1163) - the same count.
       bar 1.25 * n u * E_dv,  n = 2, or 3 under GQA;  E_dv = P^T.|dO| summed over the group.
  dq   attn_bwd_dq_k: delta = rowsum(dO * o) is taken from the bf16 o (:802-807), which carries the forward's 2u * sv, so
       delta is off by up to 2u * A with A_r = sum_c |dO_rc| sv_rc, and dS = P (dP - delta) by 2u * P A; dS is packed to bf16
       (pack8, :909: u * P (|dP| + |delta|) <= u * P (|dP| + A)); the output is rounded (:958; :964 rounds the bf16 value again,
       a no-op without the RoPE epilogue).  attn_bwd_fused_k: delta (:1069), dS (f2bf into LDS, :1122), output (:1224) - the same.
       bar 1.25 * 4u * E_dq,  E_dq = sc (P o (|dP| + A)).|K|.
  dk   attn_bwd_dkdv_k: dS packed to bf16 (:680) with delta read back from the dQ kernel's buffer (the same 2u * A), the
       output (:754; :759 a no-op), and under GQA the bf16 partial (:744) before gqa_reduce_k's rounded sum (:1271).
       attn_bwd_fused_k: dS (:1127), partial (:1148), output (:1158) - the same.
       bar 1.25 * n u * E_dk,  n = 4, or 5 under GQA;  E_dk = sc (P o (|dP| + A))^T.|Q| summed over the group.
  The fused kernel and the kernel pair round at the same points (they differ in summation order only), so one count serves both.
  In the backward P = exp2(s * sc - lse) comes from the f32 lse: no bf16 rounding before the pack.

`restatement` repeats the kernels' arithmetic in float64 with a bf16 rounding at exactly these points.  Its largest error in
units of the bars over every case and input family of test_attention_edges_gpu.py, measured on the CPU
(test_attention_edges_cpu.py::test_restatement_of_the_kernels_stays_within_every_bar):
    o 0.78   lse 0.00 (it rounds nothing there)   dq 0.33   dk 0.56   dv 0.75
(a property of the reference and the bars, not of the code under test)."""
import math

import torch

F64 = torch.float64
U = 2.0 ** -8            # bf16 unit roundoff
EPS = 2.0 ** -24         # f32 unit roundoff
LN2 = math.log(2.0)
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
FAMILIES = ("R", "V", "Q")
MUTATIONS = tuple((kind, d) for kind in ("d_diag", "d_window", "d_block", "d_start", "d_len") for d in (-1, 1))


# ------------------------------------------------------------------ mask
def visible(T, causal, block, window, kv_start, kv_len, *, d_diag=0, d_window=0, d_block=0, d_start=0, d_len=0, device=None):
    """bool [B, T, T]: query i of sequence b sees key j (the mask of _attn64 in test_f32_kernels_gpu.py; `window` counts only
    under `causal`, as in the ABI).  kv_start / kv_len: int tensors [B].  Each d_* offset moves ONE boundary by that many keys:
    all zero is the true mask, exactly one of them at +-1 the mask of a kernel with an off-by-one at that boundary."""
    device = kv_start.device if device is None else device
    i = torch.arange(T, device=device)
    qi, kj = i[:, None], i[None, :]
    ok = torch.ones(T, T, dtype=torch.bool, device=device)
    if causal:
        ok = ok & (kj <= qi + d_diag)
        if window:
            ok = ok & (kj > qi - window + d_window)
    if block:
        ok = ok & (kj < (qi // block + 1) * block + d_block)
    lo = kv_start.to(device).view(-1, 1, 1) + d_start
    hi = kv_len.to(device).view(-1, 1, 1) + d_len
    return ok[None] & (kj[None] >= lo) & (kj[None] < hi)


def padding(T, device="cpu"):
    """The four sequences of a call: no padding, kv_start = 64, kv_len = 64, kv_start = 65 with kv_len = 129, each clipped to
    0 <= kv_start < kv_len <= T; at T <= 65 a single visible key at either end instead (kv_start = T - 1; kv_len = 1)."""
    if T <= 65:
        pads = [(0, T), (T - 1, T), (0, 1), (min(65, T - 1), T)]
    else:
        pads = [(0, T), (64, T), (0, 64), (min(65, min(129, T) - 1), min(129, T))]
    assert all(0 <= s < e <= T for s, e in pads)
    kv_start = torch.tensor([s for s, _ in pads], dtype=torch.int32, device=device)
    kv_len = torch.tensor([e for _, e in pads], dtype=torch.int32, device=device)
    return kv_start, kv_len


# ------------------------------------------------------------------ inputs
def make_inputs(family, B, T, Hq, Hkv, D, seed, device="cpu"):
    """bf16 q, k, v, dO of one input family, drawn on the CPU from a fixed seed (the same values on every device).
    R  randn everywhere: the arithmetic.
    V  q = randn / 4, k = randn, v[j] = e_(j mod D), dO[r] = e_((7 r + 3) mod D): output column c carries the weight of the keys
       congruent to c, so one key more or less is a large relative change of a small element of o and dv.
    Q  q = randn / 2, k[j] = e_(j mod D), v[j] = +-1 / sqrt D (sign by the parity of j mod D), dO = 1 / sqrt D: |dP| = 1 for every
       pair and delta ~ 0, so one key more or less moves the few keys' worth of dq in column j mod D."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    t = torch.arange(T)
    if family == "R":
        q, k, v, do = rn(B, T, Hq, D), rn(B, T, Hkv, D), rn(B, T, Hkv, D), rn(B, T, Hq * D)
    elif family == "V":
        q, k = 0.25 * rn(B, T, Hq, D), rn(B, T, Hkv, D)
        v = torch.eye(D)[t % D][None, :, None, :].expand(B, T, Hkv, D)
        do = torch.eye(D)[(7 * t + 3) % D][None, :, None, :].expand(B, T, Hq, D).reshape(B, T, Hq * D)
    elif family == "Q":
        q = 0.5 * rn(B, T, Hq, D)
        k = torch.eye(D)[t % D][None, :, None, :].expand(B, T, Hkv, D)
        sign = 1.0 - 2.0 * ((t % D) % 2).to(torch.float32)
        v = (sign * D ** -0.5)[None, :, None, None].expand(B, T, Hkv, D)
        do = torch.full((B, T, Hq * D), D ** -0.5)
    else:
        raise ValueError(family)
    return tuple(x.contiguous().to(torch.bfloat16).to(device) for x in (q, k, v, do))


# ------------------------------------------------------------------ float64 reference
def bf(x):
    """Round a float64 tensor to bf16 (through f32, as the kernels' f2bf sees an f32 value) and back."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


class Reference:
    """float64 attention of bf16 inputs (converted exactly).  The products that do not depend on the mask, S = sc Q K^T and
    dP = dO V^T, are formed once; forward() and backward() then serve any number of masks."""

    def __init__(self, q, k, v, do, sc):
        B, T, Hq, D = q.shape
        Hkv = k.shape[2]
        self.B, self.T, self.Hq, self.Hkv, self.D, self.G, self.sc = B, T, Hq, Hkv, D, Hq // Hkv, sc
        self.q = q.to(F64).transpose(1, 2)                                            # [B, Hq, T, D]
        self.k = k.to(F64).transpose(1, 2).repeat_interleave(self.G, 1)
        self.v = v.to(F64).transpose(1, 2).repeat_interleave(self.G, 1)
        self.do = do.to(F64).view(B, T, Hq, D).transpose(1, 2)
        self.s = self.q @ self.k.transpose(-1, -2) * sc                               # [B, Hq, T, T]
        self.dp = self.do @ self.v.transpose(-1, -2)

    # [B, H, T, D] -> the ABI's layouts
    def rows_out(self, x):
        return x.transpose(1, 2).reshape(self.B, self.T, self.Hq * self.D)

    def q_out(self, x):
        return x.transpose(1, 2)

    def kv_out(self, x):
        """sum over the query heads of each group -> [B, T, Hkv, D]"""
        return x.view(self.B, self.Hkv, self.G, self.T, self.D).sum(2).transpose(1, 2)

    def softmax(self, vis):
        """-> unnormalised p~ = exp(s - max), row sum l, row max m (0 where a row sees nothing: p~ = 0, l = 0 there)."""
        s = self.s.masked_fill(~vis[:, None], float("-inf"))
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        pt = torch.exp(s - m)
        return pt, pt.sum(-1, keepdim=True), m

    def forward(self, vis):
        """-> dict: p [B, Hq, T, T], o, lse (natural log, +inf where a row sees nothing), sv = P.|V|"""
        pt, l, m = self.softmax(vis)
        p = pt / l.clamp_min(1e-300)
        lse = (m + torch.log(l))[..., 0]
        lse = torch.where(l[..., 0] > 0, lse, torch.full_like(lse, float("inf")))
        return {"p": p, "o": self.rows_out(p @ self.v), "lse": lse, "sv": self.rows_out(p @ self.v.abs())}

    def ds(self, p, o):
        """dS = P o (dP - delta), delta = rowsum(dO o O) from the o it is given (the exact one, or the bf16 one)"""
        delta = (self.do * o.view(self.B, self.T, self.Hq, self.D).transpose(1, 2)).sum(-1, keepdim=True)
        return p * (self.dp - delta)

    def backward(self, fwd, want=("dq", "dk", "dv"), scales=True):
        """Analytic backward from forward()'s dict (rows that see no key have P = 0: they contribute nothing, whatever dO
        holds there).  -> (values, scales) dicts in the ABI's layouts."""
        p = fwd["p"]
        val, sca = {}, {}
        ds = self.ds(p, fwd["o"]) if ("dq" in want or "dk" in want) else None
        if scales and ds is not None:
            sv = fwd["sv"].view(self.B, self.T, self.Hq, self.D).transpose(1, 2)
            a = (self.do.abs() * sv).sum(-1, keepdim=True)
            eds = p * (self.dp.abs() + a)
        if "dq" in want:
            val["dq"] = self.q_out(self.sc * (ds @ self.k))
            if scales:
                sca["dq"] = self.q_out(self.sc * (eds @ self.k.abs()))
        if "dk" in want:
            val["dk"] = self.kv_out(self.sc * (ds.transpose(-1, -2) @ self.q))
            if scales:
                sca["dk"] = self.kv_out(self.sc * (eds.transpose(-1, -2) @ self.q.abs()))
        if "dv" in want:
            val["dv"] = self.kv_out(p.transpose(-1, -2) @ self.do)
            if scales:
                sca["dv"] = self.kv_out(p.transpose(-1, -2) @ self.do.abs())
        return val, sca

    def full(self, vis):
        """-> (values, scales) for all five outputs; the lse scale is |lse| + 4 sc sqrt D (0 where lse is infinite)."""
        fwd = self.forward(vis)
        val, sca = self.backward(fwd)
        val["o"], val["lse"] = fwd["o"], fwd["lse"]
        sca["o"] = fwd["sv"]
        fin = torch.isfinite(fwd["lse"])
        sca["lse"] = torch.where(fin, fwd["lse"].abs() + 4 * self.sc * math.sqrt(self.D), torch.zeros_like(fwd["lse"]))
        return val, sca

    def restatement(self, vis):
        """The bf16 kernels' arithmetic in float64, rounded to bf16 at exactly the points the module docstring lists."""
        pt, l, m = self.softmax(vis)
        l1 = l.clamp_min(1e-300)
        o = bf(self.rows_out((bf(pt) @ self.v) / l1))                                 # P, then the output
        lse = (m + torch.log(l))[..., 0]
        lse = torch.where(l[..., 0] > 0, lse, torch.full_like(lse, float("inf")))
        p = pt / l1                                                                   # exp2(s sc - lse), f32 in the kernels
        ds = bf(self.ds(p, o))                                                        # delta from the bf16 o; dS packed to bf16
        part = bf if self.G > 1 else (lambda x: x)                                    # the per-query-head partials in dkv_part
        return {"o": o, "lse": lse,
                "dq": bf(self.q_out(self.sc * (ds @ self.k))),
                "dk": bf(self.kv_out(part(self.sc * (ds.transpose(-1, -2) @ self.q)))),
                "dv": bf(self.kv_out(part(bf(p).transpose(-1, -2) @ self.do)))}


def bars(D, T, Hq, Hkv):
    """The bar of each output as a multiple of its per-element scale (module docstring)."""
    gqa = 1 if Hq != Hkv else 0
    return {"o": 1.25 * 2 * U, "lse": 4 * (math.sqrt(D) + math.sqrt(T) + 4) * EPS, "dq": 1.25 * 4 * U,
            "dk": 1.25 * (4 + gqa) * U, "dv": 1.25 * (2 + gqa) * U}


# ------------------------------------------------------------------ comparison
def _in_bars(got, ref, scale, bar):
    """|got - ref| in units of bar * scale, elementwise; an element whose bar is zero must be exact (0 -> 0, else inf)."""
    err = (got.to(F64) - ref).abs()
    ratio = (err / (bar * scale)).nan_to_num(nan=float("inf"), posinf=float("inf"))         # (a NaN in `got` counts as infinitely wrong)
    return torch.where(err == 0, torch.zeros_like(err), ratio)


def _row_mask(name, rows_mask, shape):
    """rows_mask [B, T] -> broadcastable over the output `name` (o, lse, dq are per query row; dk, dv are compared everywhere)."""
    if name in ("dk", "dv") or rows_mask is None:
        return None
    if name == "lse":
        return rows_mask[:, None, :]
    return rows_mask.view(rows_mask.shape + (1,) * (len(shape) - 2))


def check_attention(got, ref, scales, rows_mask, bar, outputs=OUTPUTS):
    """got / ref / scales: dicts of the outputs in the ABI's layouts (lse in natural log), rows_mask: bool [B, T], the query rows
    that see a key (o, lse and dq are compared there only), bar: bars(...).
    -> {name: (largest error in units of the bar, index of that element)}."""
    res = {}
    for name in outputs:
        g, r = got[name], ref[name]
        if name == "lse":                                   # rows that see nothing: +inf on both sides, not compared
            g, r = g.to(F64).nan_to_num(posinf=0.0), r.nan_to_num(posinf=0.0)
        ratio = _in_bars(g, r, scales[name], bar[name])
        m = _row_mask(name, rows_mask, ratio.shape)
        if m is not None:
            ratio = torch.where(m, ratio, torch.zeros_like(ratio))
        flat = int(ratio.reshape(-1).argmax())
        idx = []
        for n in reversed(ratio.shape):
            idx.append(flat % n)
            flat //= n
        res[name] = (ratio.reshape(-1).max().item(), tuple(reversed(idx)))
    return res


def describe(name, idx, D):
    """A check_attention index in words."""
    if name == "o":
        return f"batch {idx[0]} head {idx[2] // D} row {idx[1]} column {idx[2] % D}"
    if name == "lse":
        return f"batch {idx[0]} head {idx[1]} row {idx[2]}"
    return f"batch {idx[0]} head {idx[2]} {'row' if name == 'dq' else 'key'} {idx[1]} column {idx[3]}"


def assert_in_bars(res, D, what):
    """Every output of a check_attention result within its bar; the message names output, batch, head, row or key, column."""
    bad = [f"{name}: {worst:.3g} bars at {describe(name, idx, D)}" for name, (worst, idx) in res.items() if not worst <= 1.0]
    assert not bad, f"{what}: " + "; ".join(bad)


# ------------------------------------------------------------------ the cases of test_attention_edges_gpu.py
def _cases():
    out = []
    # head_dim 128, causal (the LLM): the forward's 64-key tiles, the pair's 128-row blocks, FUSED_TMAX = 320 from both sides
    for T in (1, 63, 64, 65, 127, 128, 129, 319, 320, 321, 449):
        for Hq, Hkv in ((4, 1), (2, 2)):
            out.append(dict(D=128, T=T, Hq=Hq, Hkv=Hkv, causal=True, block=0, window=0, scale=None))
    # head_dim 128, sliding window; a window that covers the sequence takes the plain-causal and fused paths
    for T, windows in ((449, (1, 63, 64, 65, 128, 129, 448, 449)), (200, (64, 200))):
        for w in windows:
            out.append(dict(D=128, T=T, Hq=4, Hkv=2, causal=True, block=0, window=w, scale=None))
    # head_dim 256 (Gemma: query_pre_attn_scalar != head_dim)
    for T in (65, 129, 300):
        for w in (0, 64, 77):
            out.append(dict(D=256, T=T, Hq=2, Hkv=1, causal=True, block=0, window=w, scale=256 ** -0.5 * 1.37))
    # head_dim 64, non-causal with latency blocks (the Whisper tower); block >= T is block = 0
    for T in (1, 63, 64, 65, 129, 449):
        for blk in (0, 1, 50, 64, 128):
            if blk < T:
                out.append(dict(D=64, T=T, Hq=3, Hkv=3, causal=False, block=blk, window=0, scale=None))
    out.append(dict(D=64, T=130, Hq=4, Hkv=2, causal=True, block=0, window=0, scale=None))
    return out


CASES = _cases()


def case_id(c):
    return f"D{c['D']}-T{c['T']}-h{c['Hq']}x{c['Hkv']}-{'causal' if c['causal'] else 'full'}-w{c['window']}-b{c['block']}"


def case_scale(c):
    return c["D"] ** -0.5 if c["scale"] is None else c["scale"]


def case_seed(c, family):
    return 1000 * c["T"] + c["D"] + 7 * c["window"] + 13 * c["block"] + c["Hq"] + 100000 * FAMILIES.index(family)
