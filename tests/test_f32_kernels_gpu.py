"""Every dtype-taking single-op entry point of include/uvx.h run in UVX_F32 ("parity mode") against a float64 torch
reference written out from the operation's formula.

Bars are written in units of the f32 unit roundoff EPS = 2^-24, relative to a per-element scale (the sum of the absolute
values of the terms that make up the result), and grow with the reduction length where there is one.  Every bar is checked
against bf16 in the same test: rounding the float64 reference's output (or, where the output is a near-cancellation, its
input) to bf16 must move it by more than the bar, so a kernel that rounds to bf16 anywhere on the f32 path fails.
Integer and index outputs are bit-exact; reductions are asserted deterministic (a second call is bit-identical)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -24
F64 = torch.float64


def ops():
    from ultravox_amd import ops as o
    return o


def lib():
    from ultravox_amd import _lib
    return _lib


def randn(*shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, device=DEV) * scale + shift


def close(got, ref, scale, bar, what, ref_bf=None):
    """max |got - ref| / scale <= bar, and bf16 rounding of the reference (ref_bf: the reference recomputed from bf16-rounded
    inputs) moves it by more than the bar."""
    ref = ref.detach().to(F64)
    scale = scale.detach().to(F64) + 1e-300
    probe = ref.to(torch.bfloat16).to(F64) if ref_bf is None else ref_bf.detach().to(F64)
    bf_err = ((probe - ref).abs() / scale).max().item()
    assert bf_err > bar, f"{what}: bar {bar:.3g} does not tell bf16 ({bf_err:.3g}) from f32"
    err = ((got.to(F64) - ref).abs() / scale).max().item()
    assert err <= bar, f"{what}: error {err:.3g} (x scale) over the f32 bar {bar:.3g} (bf16 would be {bf_err:.3g})"


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


# ------------------------------------------------------------------ uvx_gemm
def _gemm_ref(a, b, alpha=1.0, bias=None, act=0, res=None, res_mod=0, acc=None):
    z = alpha * (a.to(F64) @ b.to(F64).t())
    absz = abs(alpha) * (a.to(F64).abs() @ b.to(F64).abs().t())
    if bias is not None:
        z = z + bias.to(F64)
        absz = absz + bias.to(F64).abs()
    y, scale = (gelu64(z), 1.2 * absz) if act else (z, absz)
    if res is not None:
        r = res.to(F64)
        if res_mod:
            r = r[torch.arange(a.shape[0], device=a.device) % res_mod]
        y, scale = y + r, scale + r.abs()
    if acc is not None:
        y, scale = y + acc.to(F64), scale + acc.to(F64).abs()
    return y, scale


def _gemm_bar(K):
    return (2.0 * math.sqrt(K) + 4.0) * EPS


@pytest.mark.parametrize("M,N,K", [(1, 4, 16), (65, 252, 48), (333, 1028, 1040), (2049, 260, 4096), (64, 64, 16), (130, 72, 208)])
def test_f32_gemm_ragged_shapes_and_epilogues(M, N, K):
    """uvx_gemm: tiles cut by M / N / K, every epilogue."""
    torch.manual_seed(M * 7 + N + K)
    a, b = randn(M, K), randn(N, K, scale=0.5)
    bias, res = randn(N), randn(M, N)
    bar = _gemm_bar(K)
    y, s = _gemm_ref(a, b)
    close(ops().gemm(a, b), y, s, bar, "plain")
    y, s = _gemm_ref(a, b, alpha=0.37, bias=bias, act=1, res=res)
    close(ops().gemm(a, b, bias=bias, act="gelu", residual=res, alpha=0.37), y, s, bar, "alpha + bias + gelu + residual")
    mod = max(1, min(7, M))
    pos = randn(mod, N)
    y, s = _gemm_ref(a, b, bias=bias, res=pos, res_mod=mod)
    close(ops().gemm(a, b, bias=bias, residual=pos, res_mod=mod), y, s, bar, "res_mod")
    c0 = randn(M, N, scale=3.0)
    y, s = _gemm_ref(a, b, acc=c0)
    got = ops().gemm(a, b, out=c0.clone(), accumulate=True)
    close(got, y, s, bar, "accumulate")
    assert torch.equal(got, ops().gemm(a, b, out=c0.clone(), accumulate=True))


def test_f32_gemm_batched_strides_and_row_strided_a():
    """uvx_gemm through GemmDesc: batch strides, lda > K, ldc > N."""
    torch.manual_seed(3)
    L = lib()
    nb, M, N, K = 3, 70, 96, 80
    lda, ldc = K + 20, N + 4
    A = randn(nb, M + 1, lda)                  # batch stride (M + 1) * lda, rows lda > K apart
    B = randn(nb, N, K, scale=0.5)
    R = randn(nb, M, N)
    bias = randn(N)
    Cb = torch.full((nb, M, ldc), 7.0, device=DEV)
    d = L.GemmDesc()
    d.A, d.B, d.C, d.bias, d.residual = A.data_ptr(), B.data_ptr(), Cb.data_ptr(), bias.data_ptr(), R.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ldr = M, N, K, lda, K, ldc, N
    d.batch, d.stride_a, d.stride_b, d.stride_c, d.stride_r = nb, (M + 1) * lda, N * K, M * ldc, M * N
    d.alpha, d.act = 0.5, 1
    L.check(L.lib().uvx_gemm(L.stream_ptr(), L.F32, C.byref(d)), "uvx_gemm")
    for z in range(nb):
        y, s = _gemm_ref(A[z, :M, :K], B[z], alpha=0.5, bias=bias, act=1, res=R[z])
        close(Cb[z, :, :N], y, s, _gemm_bar(K), f"batch {z}")
    assert (Cb[:, :, N:] == 7.0).all()         # the row padding of C is not written


def test_f32_gemm_refuses_bf16_only_forms():
    """uvx_gemm / uvx_gemm_splitk: the bf16-only forms are refused in f32, never run silently."""
    L = lib()
    a, b = randn(32, 64), randn(64, 64)
    c2 = torch.empty(32, 64, device=DEV)
    for act in ("gelu_keep", "gelu_bwd"):
        with pytest.raises(L.UvxError, match="bf16 path only"):
            ops().gemm(a, b, act=act, c2=c2)
    with pytest.raises(L.UvxError, match="bf16 path only"):
        ops().gemm(a, b, b_kn=True)
    for ep in (1, 2):
        with pytest.raises(L.UvxError, match="bf16 only"):
            ops().gemm(a, b, epilogue=ep, c2=torch.empty(32, 128, device=DEV))
        with pytest.raises(L.UvxError, match="bf16 only"):
            ops().gemm_splitk(a, b, epilogue=ep, c2=torch.empty(32, 128, device=DEV))
    with pytest.raises(ValueError, match="multiple of 16"):
        ops().gemm(randn(8, 40), randn(8, 40))


@pytest.mark.parametrize("M,N,K", [(65, 4096, 1024), (316, 1028, 2048)])
def test_f32_gemm_splitk_equals_plain_gemm(M, N, K):
    """uvx_gemm_splitk in f32 (workspace lent, any force_split) is uvx_gemm bit for bit."""
    torch.manual_seed(M)
    a, b, bias = randn(M, K), randn(N, K, scale=0.5), randn(N)
    want = ops().gemm(a, b, bias=bias)
    for s in (0, 1, 4):
        got = ops().gemm_splitk(a, b, bias=bias, force_split=s)
        assert torch.equal(got, want), s
    y, sc = _gemm_ref(a, b, bias=bias)
    close(want, y, sc, _gemm_bar(K), "splitk")


def _rms64(x, w, eps, flavor):
    x = x.to(F64)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    weff = (1.0 + w.to(F64)) if flavor else w.to(F64)
    return x * r * weff, (x * r).abs() * weff.abs()


@pytest.mark.parametrize("M,K,flavor", [(1, 2048, 0), (2, 2560, 1), (17, 3584, 0), (40, 1024, 1)])
def test_f32_gemm_rmsnorm_is_rmsnorm_then_gemm(M, K, flavor):
    """uvx_gemm_rmsnorm in f32 runs uvx_rmsnorm (flavor 0 / Gemma 1 + w) into norm_out, then uvx_gemm."""
    torch.manual_seed(K + flavor)
    L = lib()
    N, eps = 264, 1e-6
    a, w, b = randn(M, K, scale=2.0), randn(K, scale=0.3), randn(N, K, scale=0.5)
    out = torch.empty(M, N, device=DEV)
    norm_out = torch.empty(M, K, device=DEV)
    d = L.GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.batch, d.alpha = M, N, K, K, K, N, 1, 1.0
    L.check(L.lib().uvx_gemm_rmsnorm(L.stream_ptr(), L.F32, C.byref(d), L.ptr(w), C.c_float(eps), flavor, L.ptr(norm_out)))
    yn, sn = _rms64(a, w, eps, flavor)
    nbar = 4 * (math.sqrt(K) + 4) * EPS
    close(norm_out, yn, sn, nbar, "norm")                               # rmsnorm_fwd_k<float>, Gemma's (1 + w) included
    if flavor == 0:
        assert torch.equal(norm_out, ops().rmsnorm(a, w, eps))
    assert torch.equal(out, ops().gemm(norm_out, b))                   # the two launches it stands for, bit for bit
    close(out, yn @ b.to(F64).t(), sn @ b.to(F64).abs().t(), _gemm_bar(K) + nbar, "norm + gemm")
    with pytest.raises(ValueError, match="norm_out"):
        L.check(L.lib().uvx_gemm_rmsnorm(L.stream_ptr(), L.F32, C.byref(d), L.ptr(w), C.c_float(eps), flavor, None))


# ------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows,cols", [(3, 8), (7, 384), (300, 1024), (33, 1280), (5, 5120)])
def test_f32_layernorm_fwd_bwd(rows, cols):
    """uvx_layernorm, uvx_layernorm_bwd (with and without dx_add)."""
    torch.manual_seed(rows + cols)
    eps = 1e-5
    x, w, b = randn(rows, cols, scale=2.0, shift=0.3), randn(cols), randn(cols)
    x64 = x.to(F64).requires_grad_(True)
    mu = x64.mean(-1, keepdim=True)
    xh = (x64 - mu) * torch.rsqrt((x64 - mu).pow(2).mean(-1, keepdim=True) + eps)
    y = xh * w.to(F64) + b.to(F64)
    bar = 4 * (math.sqrt(cols) + 4) * EPS
    close(ops().layernorm(x, w, b, eps), y, xh.abs() * w.to(F64).abs() + b.to(F64).abs(), bar, "layernorm")
    dy, add = randn(rows, cols), randn(rows, cols)
    y.backward(dy.to(F64))
    g = dy.to(F64) * w.to(F64)
    r = torch.rsqrt((x64 - mu).pow(2).mean(-1, keepdim=True) + eps).detach()
    xhd = xh.detach()
    s = r * (g.abs() + g.abs().mean(-1, keepdim=True) + xhd.abs() * (g * xhd).abs().mean(-1, keepdim=True))
    close(ops().layernorm_bwd(dy, x, w, eps), x64.grad, s, bar, "layernorm_bwd")
    close(ops().layernorm_bwd(dy, x, w, eps, dx_add=add), x64.grad + add.to(F64), s + add.to(F64).abs(), bar, "layernorm_bwd + dx_add")


@pytest.mark.parametrize("rows,cols", [(5, 8), (33, 2048), (19, 2560), (40, 3584), (3, 3840), (17, 5376), (21, 8192)])
def test_f32_rmsnorm_fwd_bwd(rows, cols):
    """uvx_rmsnorm, uvx_rmsnorm_bwd: dx only, dw only, both; rows not a multiple of the 16-row dw blocks."""
    torch.manual_seed(rows * cols)
    eps = 1e-6
    x, w = randn(rows, cols, scale=1.5), randn(cols, scale=0.2, shift=0.5)
    bar = 4 * (math.sqrt(cols) + 4) * EPS
    y, s = _rms64(x, w, eps, 0)
    close(ops().rmsnorm(x, w, eps), y, s, bar, "rmsnorm")
    x64, w64 = x.to(F64).requires_grad_(True), w.to(F64).requires_grad_(True)
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    dy = randn(rows, cols)
    (x64 * r * w64).backward(dy.to(F64))
    add = randn(rows, cols)
    gw = dy.to(F64) * w.to(F64)
    rd, xd = r.detach(), x.to(F64)
    sx = rd * gw.abs() + xd.abs() * rd.pow(3) * (gw * xd).abs().mean(-1, keepdim=True)
    sw = (dy.to(F64) * xd * rd).abs().sum(0)
    barw = 4 * (math.sqrt(cols) + math.sqrt(rows) + 4) * EPS
    dx, dw = ops().rmsnorm_bwd(dy, x, w, eps, dx_add=add, want_dw=True)
    close(dx, x64.grad + add.to(F64), sx + add.to(F64).abs(), bar, "dx + dx_add (with dw)")
    close(dw, w64.grad, sw, barw, "dw (with dx)")
    dx2, none = ops().rmsnorm_bwd(dy, x, w, eps)
    assert none is None
    close(dx2, x64.grad, sx, bar, "dx only")
    none, dw2 = ops().rmsnorm_bwd(dy, x, w, eps, want_dx=False, want_dw=True)
    assert none is None
    close(dw2, w64.grad, sw, barw, "dw only")
    for _ in range(2):                                                   # dw: a fixed summation order
        assert torch.equal(ops().rmsnorm_bwd(dy, x, w, eps, want_dx=False, want_dw=True)[1], dw2)
        assert torch.equal(ops().rmsnorm_bwd(dy, x, w, eps, dx_add=add, want_dw=True)[1], dw)


# ------------------------------------------------------------------ rotary / per-head norms
def _rope_table(T, D, theta=10000.0):
    inv = 1.0 / theta ** (torch.arange(0, D, 2, dtype=F64) / D)
    ang = torch.arange(T, dtype=F64)[:, None] * inv[None]
    cs = torch.stack([ang.cos(), ang.sin()], -1).float().to(DEV)        # [T, D/2, 2] f32, the layout of uvx_rope's cos_sin
    return cs


def _rope64(x, cs, T, H, D, sgn=1.0):
    """rotate_half form on heads 0..H-1 of x [rows, ld]; cos / sin are the f32 table values."""
    rows = x.shape[0]
    out = x.to(F64).clone()
    pos = torch.arange(rows, device=x.device) % T
    co = cs[pos, :, 0].to(F64)[:, None, :]
    si = cs[pos, :, 1].to(F64)[:, None, :] * sgn
    h = out[:, :H * D].view(rows, H, D)
    lo, hi = h[..., :D // 2].clone(), h[..., D // 2:].clone()
    scale = out.abs()
    sh = scale[:, :H * D].view(rows, H, D)
    sh[..., :D // 2] = lo.abs() * co.abs() + hi.abs() * si.abs()
    sh[..., D // 2:] = hi.abs() * co.abs() + lo.abs() * si.abs()
    h[..., :D // 2] = lo * co - hi * si
    h[..., D // 2:] = hi * co + lo * si
    return out, scale


@pytest.mark.parametrize("D", [64, 128, 256])
def test_f32_rope_forward_and_inverse(D):
    """uvx_rope forward, then inverse."""
    torch.manual_seed(D)
    B, T, H, ld = 2, 37, 3, 5 * D                      # 3 heads rotated, 2 untouched
    cs = _rope_table(T, D)
    x = randn(B * T, ld)
    x0 = x.clone()
    ops().rope_(x, cs, T, H, D)
    want, s = _rope64(x0, cs, T, H, D)
    close(x, want, s, 4 * EPS, "rope")
    assert torch.equal(x[:, H * D:], x0[:, H * D:])
    ops().rope_(x, cs, T, H, D, inverse=True)
    back, s2 = _rope64(x0, cs, T, H, D)            # R(-t) R(t) x = x (cos^2 + sin^2 of the f32 table: within an ulp of 1)
    close(x, x0, x0.to(F64).abs() + s2, 12 * EPS, "rope inverse after forward")


@pytest.mark.parametrize("D,flavor", [(128, 0), (128, 1), (256, 0), (256, 1), (64, 0)])
def test_f32_qk_norm_rope_and_backward(D, flavor):
    """uvx_qk_norm_rope (Qwen3 / Gemma-3 flavours, keep_raw), uvx_qk_norm_bwd."""
    torch.manual_seed(D + flavor)
    B, T, Hq, Hkv, eps = 2, 19, 4, 2, 1e-6
    ld = (Hq + 2 * Hkv) * D + 8
    qkv = randn(B * T, ld, scale=1.7)
    wq, wk = randn(D, scale=0.3, shift=0.8 * (1 - flavor)), randn(D, scale=0.3, shift=0.8 * (1 - flavor))
    cs = _rope_table(T, D, 1e6)
    x0 = qkv.clone()
    raw = ops().qk_norm_rope_(qkv, wq, wk, cs, T, Hq, Hkv, D, eps=eps, keep_raw=True, flavor=flavor)
    H = Hq + Hkv
    assert torch.equal(raw, x0[:, :H * D])                                      # keep_raw: the un-normalised rows, bit for bit
    assert torch.equal(qkv[:, H * D:], x0[:, H * D:])                          # v and the row padding untouched
    heads = x0[:, :H * D].to(F64).view(-1, H, D)
    w = torch.cat([wq[None].expand(Hq, D), wk[None].expand(Hkv, D)]).to(F64)
    r = torch.rsqrt(heads.pow(2).mean(-1, keepdim=True) + eps)
    weff = (1 + w) if flavor else w
    n = heads * r * weff
    ns = (heads * r).abs() * weff.abs()
    want, s = _rope64(n.reshape(-1, H * D), cs, T, H, D)
    _, s_n = _rope64(ns.reshape(-1, H * D), cs, T, H, D)
    close(qkv[:, :H * D], want, s_n, 4 * (math.sqrt(D) + 4) * EPS, "qk_norm_rope")
    # backward: gradient of the normalised (pre-rotary) rows -> gradient of the raw rows
    hr = heads.clone().requires_grad_(True)
    rr = torch.rsqrt(hr.pow(2).mean(-1, keepdim=True) + eps)
    dn = randn(B * T, ld)
    (hr * rr * weff).backward(dn[:, :H * D].to(F64).view(-1, H, D))
    g = dn[:, :H * D].to(F64).view(-1, H, D) * weff
    sx = r * g.abs() + heads.abs() * r.pow(3) * (g * heads).abs().mean(-1, keepdim=True)
    d = dn.clone()
    ops().qk_norm_bwd_(d, raw, wq, wk, Hq, Hkv, D, eps=eps, flavor=flavor)
    close(d[:, :H * D], hr.grad.reshape(-1, H * D), sx.reshape(-1, H * D), 4 * (math.sqrt(D) + 4) * EPS, "qk_norm_bwd")
    assert torch.equal(d[:, H * D:], dn[:, H * D:])


# ------------------------------------------------------------------ activations
@pytest.mark.parametrize("gate_first", [False, True])
def test_f32_swiglu_fwd_bwd(gate_first):
    """uvx_swiglu, uvx_swiglu_bwd in both half orders."""
    torch.manual_seed(int(gate_first))
    rows, half = 37, 1032
    x = randn(rows, 2 * half, scale=3.0)
    v64, g64 = (x[:, half:], x[:, :half]) if gate_first else (x[:, :half], x[:, half:])
    v64, g64 = v64.to(F64), g64.to(F64)
    sg = torch.sigmoid(g64)
    close(ops().swiglu(x, gate_first), g64 * sg * v64, (g64 * sg * v64).abs(), 16 * EPS, "swiglu")
    dout = randn(rows, half)
    d64 = dout.to(F64)
    din = ops().swiglu_bwd(dout, x, gate_first)
    dv, dg = (din[:, half:], din[:, :half]) if gate_first else (din[:, :half], din[:, half:])
    close(dv, d64 * g64 * sg, (d64 * g64 * sg).abs(), 16 * EPS, "d value")
    # silu' = s (1 + g (1 - s)): 1 - s is formed from the rounded s, so the bar is relative to s (1 + |g|)
    close(dg, d64 * v64 * sg * (1 + g64 * (1 - sg)), (d64 * v64).abs() * sg * (1 + g64.abs()), 16 * EPS, "d gate")


def test_f32_gelu_fwd_bwd_is_erf_gelu():
    """uvx_gelu, uvx_gelu_bwd: erf GELU and its exact derivative."""
    torch.manual_seed(12)
    n = 65536 + 8
    x = torch.cat([randn(n - 8, scale=3.0), torch.tensor([0.0, -0.0, 1e-20, -1e-20, 8.0, -8.0, 30.0, -30.0], device=DEV)])
    x64 = x.to(F64)
    erf = torch.erf(x64 / math.sqrt(2))
    cdf = 0.5 * (1 + erf)
    pdf = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
    # 1 + erf cancels for x << 0 and exp(-x^2 / 2) carries the rounding of x^2 / 2: the scales hold those terms in absolute value
    cdf_abs = 0.5 * (1 + erf.abs())
    close(ops().gelu(x), x64 * cdf, x64.abs() * cdf_abs, 16 * EPS, "gelu")
    dout = randn(n)
    d64 = dout.to(F64)
    close(ops().gelu_bwd(dout, x), d64 * (cdf + x64 * pdf), d64.abs() * (cdf_abs + x64.abs() * pdf * (1 + 0.5 * x64 * x64)), 16 * EPS,
          "gelu_bwd")
    # the exact erf GELU, not the tanh approximation: at x = 1 the two differ by 1.5e-4
    assert abs(ops().gelu(torch.ones(8, device=DEV))[0].item() - 0.8413447460685429) < 4e-7


# ------------------------------------------------------------------ attention
def _attn64(q, k, v, causal, block, scale, kv_start=None, kv_len=None, window=0):
    """float64 softmax(q k^T * scale + mask) v; -> o, lse (natural log), visible mask, sum_j p_j |v_j|."""
    B, T, Hq, D = q.shape
    Hkv = k.shape[2]
    qf, kf, vf = (t.to(F64).transpose(1, 2) for t in (q, k, v))
    kf, vf = kf.repeat_interleave(Hq // Hkv, 1), vf.repeat_interleave(Hq // Hkv, 1)
    s = qf @ kf.transpose(-1, -2) * scale
    i = torch.arange(T, device=q.device)
    ok = torch.ones(B, 1, T, T, dtype=torch.bool, device=q.device)
    if causal:
        ok = ok & (i[None, :] <= i[:, None])[None, None]
    if block:
        ok = ok & ((i[None, :] // block) <= (i[:, None] // block))[None, None]
    if window:
        ok = ok & (i[None, :] > i[:, None] - window)[None, None]
    if kv_len is not None:
        ok = ok & (i[None, None, None, :] < kv_len.view(-1, 1, 1, 1))
    if kv_start is not None:
        ok = ok & (i[None, None, None, :] >= kv_start.view(-1, 1, 1, 1))
    s = s.masked_fill(~ok, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.nan_to_num(torch.softmax(s, -1), 0.0)
    o = (p @ vf).transpose(1, 2).reshape(B, T, Hq * D)
    sv = (p @ vf.abs()).transpose(1, 2).reshape(B, T, Hq * D)
    return o, lse, ok.expand(B, Hq, T, T), sv


ATTN_CASES = [
    # D, B, Hq, Hkv, T, causal, block, window, scale, pad
    (64, 2, 4, 4, 17, False, 0, 0, None, "right"),
    (64, 1, 2, 2, 1500, False, 100, 0, None, "right"),               # Whisper: 30 s of frames, chunked block mask
    (64, 2, 2, 1, 333, False, 50, 0, None, "none"),
    (128, 3, 8, 1, 129, True, 0, 0, None, "both"),                 # GQA 8:1, left + right padding
    (128, 2, 4, 2, 333, True, 0, 64, None, "left"),                # sliding window
    (256, 2, 4, 2, 77, True, 0, 0, 256 ** -0.5 * 1.37, "both"),    # Gemma: head_dim 256, query_pre_attn_scalar != head_dim
    (256, 1, 2, 2, 1, True, 0, 0, None, "none"),
    (128, 1, 1, 1, 1500, True, 0, 0, None, "none"),
]


@pytest.mark.parametrize("D,B,Hq,Hkv,T,causal,block,window,scale,pad", ATTN_CASES)
def test_f32_attention_forward_backward(D, B, Hq, Hkv, T, causal, block, window, scale, pad):
    """uvx_attention_fwd (o and lse), uvx_attention_bwd; workspace from uvx_attention_ws_bytes."""
    torch.manual_seed(D + T + Hq)
    sc = D ** -0.5 if scale is None else scale
    q, k, v = randn(B, T, Hq, D), randn(B, T, Hkv, D), randn(B, T, Hkv, D)
    do = randn(B, T, Hq * D)
    kv_start = kv_len = None
    if pad in ("left", "both"):
        kv_start = torch.tensor([(7 * b) % max(T // 3, 1) for b in range(B)], device=DEV, dtype=torch.int32)
        kv_start[-1] = max(T // 3, 0)
    if pad in ("right", "both"):
        kv_len = torch.tensor([T - (11 * b) % max(T // 3, 1) for b in range(B)], device=DEV, dtype=torch.int32)
        kv_len[0] = T - T // 4
    o, lse = ops().attention(q, k, v, causal=causal, block=block, scale=sc, kv_start=kv_start, kv_len=kv_len, window=window)
    qr, kr, vr = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    ref, lse_ref, ok, sv = _attn64(qr, kr, vr, causal, block, sc, kv_start, kv_len, window)
    rows = ok.any(-1)                                                   # [B, Hq, T]: query rows that see a key
    rows_o = rows.transpose(1, 2).repeat_interleave(D, -1).reshape(B, T, Hq * D)
    assert rows.any()
    bar = 4 * (math.sqrt(D) + math.sqrt(T) + 4) * EPS
    close(o[rows_o], ref.detach()[rows_o], sv.detach()[rows_o], bar, "o")
    lse_nat = lse.to(F64) * math.log(2.0)                              # log2-domain in the ABI
    close(lse_nat[rows], lse_ref.detach()[rows], lse_ref.detach()[rows].abs() + sc * math.sqrt(D) * 4, bar, "lse")
    dq, dk, dv = ops().attention_bwd(q, k, v, o, lse, do, causal=causal, block=block, scale=sc, kv_start=kv_start, kv_len=kv_len,
                                     window=window)
    (ref * rows_o).backward(do.to(F64) * rows_o)
    gbar = 16 * (math.sqrt(D) + math.sqrt(T) + 4) * EPS
    # the size of the terms of dq / dk (scale * dO.V * K): the bar for a gradient that is exactly zero (one visible key: softmax is 1)
    floor = sc * do.norm(dim=-1).max().item() * v.norm(dim=-1).max().item() * max(q.abs().max().item(), k.abs().max().item())
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        if name == "dq":
            m = rows.transpose(1, 2)[..., None].expand_as(got)
            got, want = got * m, want * m
        if want.abs().max().item() == 0:
            assert got.abs().max().item() <= gbar * floor, name
            continue
        # norm-wise per tensor: max error over the largest gradient entry
        close(got, want, torch.full_like(want, want.abs().max().item()), gbar, name)
    # keys no query sees get exactly zero gradient
    seen = ok.any(2).any(1)                                             # [B, T] keys visible to some query
    assert (dk[~seen] == 0).all() and (dv[~seen] == 0).all()
    again = ops().attention_bwd(q, k, v, o, lse, do, causal=causal, block=block, scale=sc, kv_start=kv_start, kv_len=kv_len, window=window)
    assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), again))


# ------------------------------------------------------------------ losses
def _ce_call(logits, labels, dl, B, T, V, ld, grad_scale=1.0):
    L = lib()
    loss = torch.zeros(1, device=DEV)
    scratch = torch.empty(2 + B * T, device=DEV)
    L.check(L.lib().uvx_ce_loss(L.stream_ptr(), L.F32, L.ptr(logits), L.ptr(labels), L.ptr(loss), L.ptr(dl), B, T, V, ld,
                                C.c_float(grad_scale), L.ptr(scratch)), "uvx_ce_loss")
    return loss[0]


def _ce64(x, labels, V, grad_scale):
    """shifted causal-LM mean CE; labels outside [0, V) count as ignored.  -> loss, grad, loss scale, grad scale, lse, valid"""
    B, T, _ = x.shape
    tgt = F.pad(labels, (0, 1), value=-100)[:, 1:]
    valid = (tgt >= 0) & (tgt < V)
    x64 = x.to(F64)
    lse = torch.logsumexp(x64, -1)
    t = tgt.clamp(0, V - 1)
    xt = x64.gather(-1, t[..., None])[..., 0]
    n = valid.sum().item()
    loss = ((lse - xt) * valid).sum() / n
    loss_scale = ((lse.abs() + xt.abs()) * valid).sum() / n
    p = torch.exp(x64 - lse[..., None])
    onehot = F.one_hot(t, V).to(F64)
    g = grad_scale / n
    grad = (p - onehot) * g * valid[..., None]
    return loss, grad, loss_scale, (p + onehot) * abs(g) + 1e-300, lse, valid


@pytest.mark.parametrize("V,pad,shift", [(32000, 0, 0.0), (128256, 64, 1e4), (151936, 0, -1e4), (262144, 8, 0.0)])
def test_f32_ce_loss(V, pad, shift):
    """uvx_ce_loss: padded row stride, large logit offsets, ignored and out-of-range labels, grad_scale, in place."""
    torch.manual_seed(V % 1000)
    B, T = 2, 5
    ld = V + pad
    full = randn(B, T, ld, scale=2.0, shift=shift)
    x = full[..., :V]
    labels = torch.randint(0, V, (B, T), device=DEV)
    labels[0, 1] = -100
    labels[0, 2] = V                     # out of range: ignored like -100, not counted
    labels[1, 3] = -7
    labels[1, 1] = int(x[1, 0].argmax())  # the label is the row's maximum
    xb = x.to(torch.bfloat16)
    for gs in (1.0, 0.25):
        loss64, g64, ls, gsc, lse, valid = _ce64(x, labels, V, gs)
        lossb, gb, *_ = _ce64(xb.float(), labels, V, gs)
        dl = torch.full((B, T, ld), 5.0, device=DEV)
        loss = _ce_call(full, labels, dl, B, T, V, ld, gs)
        bar_loss = (16 + 4 * math.sqrt(V / 2048)) * EPS
        close(loss.reshape(1), loss64.reshape(1), ls.reshape(1), bar_loss, "loss", ref_bf=lossb.reshape(1))
        # p = exp(x - lse): the f32 lse and x - lse are rounded at the magnitude of the logits
        bar_g = (16 + 4 * math.sqrt(V / 2048) + 4 * lse.abs().max().item() + 2 * x.abs().max().item()) * EPS
        close(dl[..., :V], g64, gsc, bar_g, "dlogits", ref_bf=gb if shift else None)
        assert (dl[..., :V][~valid] == 0).all() and (dl[..., V:] == 5.0).all()   # ignored rows: exact zeros; the row padding untouched
        dl2 = torch.empty_like(dl)
        assert torch.equal(_ce_call(full, labels, dl2, B, T, V, ld, gs), loss)
        assert torch.equal(dl2[..., :V], dl[..., :V])
        inp = full.clone()                                            # in place over the logits
        assert torch.equal(_ce_call(inp, labels, inp, B, T, V, ld, gs), loss)
        assert torch.equal(inp[..., :V], dl[..., :V]) and torch.equal(inp[..., V:], full[..., V:])
    # nothing to score: NaN (torch's mean over an empty set), all-zero gradient
    dl = torch.full((B, T, ld), 5.0, device=DEV)
    none = torch.full_like(labels, -100)
    none[0, 3] = V + 3
    assert math.isnan(_ce_call(full, none, dl, B, T, V, ld).item())
    assert (dl[..., :V] == 0).all()


def _kl64(s, t, pair_row, pair_w, tau, gs):
    ls = torch.log_softmax(s.to(F64) / tau, -1)
    lt = torch.log_softmax(t.to(F64) / tau, -1)
    R = s.shape[0]
    loss = torch.zeros((), dtype=F64, device=s.device)
    lscale = torch.zeros((), dtype=F64, device=s.device)
    grad = torch.zeros_like(ls)
    gscale = torch.zeros_like(ls)
    for slot in range(2):
        idx = pair_row[slot].long()
        has = idx >= 0
        w = torch.where(has, pair_w[slot].to(F64), torch.zeros((), dtype=F64, device=s.device))
        lti = lt[idx.clamp(min=0)]
        pt = lti.exp()
        loss = loss + (w * (pt * (lti - ls)).sum(-1)).sum()
        lscale = lscale + (w.abs() * (pt * (lti.abs() + ls.abs())).sum(-1)).sum()
        grad = grad + w[:, None] * (ls.exp() - pt) * gs / tau
        gscale = gscale + w.abs()[:, None] * (ls.exp() + pt) * abs(gs) / tau
    return loss, grad, lscale, gscale


@pytest.mark.parametrize("V,tau", [(32000, 2.0), (151936, 0.7)])
def test_f32_kl_loss(V, tau):
    """uvx_kl_loss: temperature, two different teacher rows, one slot, no partner, aliasing."""
    torch.manual_seed(V % 997)
    R, Rt = 7, 5
    s, t = randn(R, V, scale=3.0), randn(Rt, V, scale=3.0, shift=1.0)
    pair_row = torch.tensor([[0, 1, -1, 2, -1, 4, 3],          # slot 0
                             [3, 1, 2, -1, -1, 0, 3]],         # slot 1: rows 0 / 5 pair with a DIFFERENT teacher row, 1 / 6 the same
                            device=DEV, dtype=torch.int32)
    pair_w = torch.rand(2, R, device=DEV) + 0.2
    gs = 0.6
    loss64, g64, ls, gsc = _kl64(s, t, pair_row, pair_w, tau, gs)
    lossb, gb, *_ = _kl64(s.bfloat16().float(), t.bfloat16().float(), pair_row, pair_w, tau, gs)
    loss, dl = ops().kl_loss(s, t, pair_row, pair_w, tau, grad_scale=gs)
    close(loss.reshape(1), loss64.reshape(1), ls.reshape(1), (16 + 4 * math.sqrt(V / 2048)) * EPS, "kl loss", ref_bf=lossb.reshape(1))
    mag = max((s.abs().max().item() + 1) / tau, (t.abs().max().item() + 1) / tau) + math.log(V)
    close(dl, g64, gsc, (16 + 4 * math.sqrt(V / 2048) + 6 * mag) * EPS, "kl grad")
    assert (dl[4] == 0).all()                                          # no partner: an exact-zero gradient
    loss2, dl2 = ops().kl_loss(s, t, pair_row, pair_w, tau, grad_scale=gs)
    assert torch.equal(loss2, loss) and torch.equal(dl2, dl)
    inp = s.clone()                                                    # dlogits may alias the student logits
    L = lib()
    lo = torch.zeros(1, device=DEV)
    scratch = torch.empty(R, device=DEV)
    L.check(L.lib().uvx_kl_loss(L.stream_ptr(), L.F32, L.ptr(inp), L.ptr(t), L.ptr(pair_row), L.ptr(pair_w), L.ptr(lo), L.ptr(inp),
                                C.c_int64(R), V, V, V, C.c_float(tau), C.c_float(gs), L.ptr(scratch)), "uvx_kl_loss")
    assert torch.equal(lo, loss.reshape(1)) and torch.equal(inp, dl)


# ------------------------------------------------------------------ merge / argmax / greedy bookkeeping
def test_f32_embed_merge_and_backward_are_bit_exact():
    """uvx_embed_merge, uvx_merge_embeds_bwd with an f32 config: overlap and clipping."""
    from oracle.reference_cpu import merge_ref
    L = lib()
    torch.manual_seed(21)
    B, T, D, Na, n_items, V = 3, 50, 72, 12, 5, 100
    table = randn(V, D)
    ids = torch.randint(0, V, (B, T), device=DEV)
    audio = randn(n_items, Na, D)
    start = torch.tensor([3, 10, 0, 45, 20], device=DEV)            # item 1 overlaps item 0; item 3 clipped by len
    tok_len = torch.tensor([12, 9, 7, 5, 0], device=DEV, dtype=torch.int32)
    bsz = torch.tensor([2, 2, 1], device=DEV)
    cfg = L.Config()
    cfg.dtype, cfg.llm_d, cfg.vocab = L.F32, D, V
    out = torch.empty(B, T, D, device=DEV)
    scratch = torch.empty(B * T + n_items, device=DEV, dtype=torch.int32)
    L.check(L.lib().uvx_embed_merge(L.stream_ptr(), C.byref(cfg), L.ptr(table), L.ptr(ids), L.ptr(audio), L.ptr(bsz), L.ptr(start),
                                    L.ptr(tok_len), B, T, n_items, Na, L.ptr(out), L.ptr(scratch)))
    want = merge_ref(F.embedding(ids, table).cpu(), audio.cpu(), start.cpu(), tok_len.cpu(), bsz.cpu())
    assert torch.equal(out.cpu(), want)
    g = randn(B, T, D)
    da = torch.full_like(audio, 3.0)
    L.check(L.lib().uvx_merge_embeds_bwd(L.stream_ptr(), C.byref(cfg), L.ptr(g), L.ptr(start), L.ptr(tok_len), B, T, n_items, Na,
                                         L.ptr(da), L.ptr(scratch)))
    a_req = audio.cpu().to(F64).requires_grad_(True)
    merge_ref(torch.zeros(B, T, D, dtype=F64), a_req, start.cpu(), tok_len.cpu(), bsz.cpu()).backward(g.cpu().to(F64))
    assert torch.equal(da.cpu().to(F64), a_req.grad)


@pytest.mark.parametrize("V", [262144, 32003, 8, 1000])
def test_f32_argmax_ties_and_all_minus_inf(V):
    """uvx_argmax: torch.argmax semantics (lowest index on ties, 0 for a row of -inf)."""
    L = lib()
    torch.manual_seed(V % 101)
    rows = 6
    x = randn(rows, V)
    x[1, V // 3] = x[1, V - 1] = x[1].max() + 1.0          # tie: the lowest index wins
    x[2] = -float("inf")                                     # nothing above -inf: index 0
    x[3, :] = 0.5                                            # all equal: index 0
    x[4, V - 1] = 1e30                                       # last column
    x[5, 1] = x[5].max() + 2.0 ** -20                        # an f32-only margin (rounds away in bf16)
    out = torch.empty(rows, device=DEV, dtype=torch.int64)
    L.check(L.lib().uvx_argmax(L.stream_ptr(), L.F32, L.ptr(x), rows, V, L.ptr(out)), "uvx_argmax")
    want = torch.argmax(x.cpu(), -1)
    want[2] = 0
    assert torch.equal(out.cpu(), want)
    assert out[1].item() == V // 3 and out[4].item() == V - 1 and out[5].item() == 1


def test_f32_greedy_select_bookkeeping():
    """uvx_greedy_select: argmax, EOS, pad after finish, positions, running count."""
    L = lib()
    torch.manual_seed(5)
    B, V, stride, pad = 4, 131072 + 5, 20, 7
    x = randn(B, V)
    x[0, 11] = 50.0                                          # row 0 emits EOS 11 -> finished
    x[2, 99] = x[2, 100] = 60.0                              # tie -> 99
    eos = torch.tensor([11, 12], device=DEV)
    unfinished = torch.tensor([1, 1, 0, 1], device=DEV, dtype=torch.int32)   # row 2 finished earlier -> pad
    nxt = torch.full((B,), -1, device=DEV, dtype=torch.int64)
    seq = torch.full((B, stride), -1, device=DEV, dtype=torch.int64)
    pos0 = torch.tensor([5, 6, 7, 8], device=DEV, dtype=torch.int32)
    pos = torch.zeros(B, device=DEV, dtype=torch.int32)
    counter = torch.tensor([9, 0], device=DEV, dtype=torch.int32)     # slot 0: the previous step's count
    step, col = 3, 13
    L.check(L.lib().uvx_greedy_select(L.stream_ptr(), L.F32, L.ptr(x), B, V, L.ptr(eos), 2, C.c_int64(pad), L.ptr(unfinished),
                                      L.ptr(nxt), L.ptr(seq), C.c_int64(stride), C.c_int64(col), L.ptr(pos0), L.ptr(pos), step,
                                      L.ptr(counter)), "uvx_greedy_select")
    am = torch.argmax(x.cpu(), -1)
    want = torch.tensor([11, int(am[1]), pad, int(am[3])])
    assert torch.equal(nxt.cpu(), want)
    assert torch.equal(seq[:, col].cpu(), want) and (seq[:, :col] == -1).all() and (seq[:, col + 1:] == -1).all()
    still = [0, int(am[1]) not in (11, 12), 0, int(am[3]) not in (11, 12)]
    assert unfinished.cpu().tolist() == still
    assert pos.cpu().tolist() == [5 + step, 6 + step, 7 + step, 8 + step]
    assert counter.cpu().tolist() == [0, sum(still)]           # counter[step & 1] = rows still running; the other slot cleared
