"""Tensor-level wrappers over the single-op C-ABI entry points (PyTorch-ROCm tensors in/out).

These are plumbing for tests, benches and the host-side model code; all arithmetic happens in
libuvx.so.  Every wrapper raises if the library is missing — there is no fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import check, dtype_code, ptr, stream_ptr


def gemm(a: torch.Tensor, b: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, act: str = "none", out: Optional[torch.Tensor] = None,
         out_f32: bool = False, accumulate: bool = False, alpha: float = 1.0, res_mod: int = 0,
         epilogue: int = 0, c2: Optional[torch.Tensor] = None, b_kn: bool = False) -> torch.Tensor:
    """out[M,N] = act(alpha * a[M,K] @ b[N,K]^T + bias) + residual   (nn.Linear layout); b_kn: b is [K, N] and out = a @ b (the NN form)."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[0 if b_kn else 1]
    assert a.stride(1) == 1 and b.stride(1) == 1
    M, K = a.shape
    N = b.shape[1 if b_kn else 0]
    dt = dtype_code(a.dtype)
    if out is None:
        out = torch.empty((M, N), device=a.device,
                          dtype=torch.float32 if (out_f32 or dt == _lib.F32) else a.dtype)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.bias = 0 if bias is None else bias.data_ptr()
    d.residual = 0 if residual is None else residual.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = a.stride(0), b.stride(0), out.stride(0)
    d.ldr = 0 if residual is None else residual.stride(0)
    d.res_mod = res_mod
    d.batch = 1
    d.act = {"none": 0, "gelu": 1, "gelu_keep": 2, "gelu_bwd": 3}[act]      # 2 / 3: include/uvx.h uvx_gemm_desc_t.act (c2 = activation out / pre-activation in)
    d.out_f32 = int(out_f32)
    d.accumulate = int(accumulate)
    d.alpha = alpha
    d.epilogue = epilogue
    d.C2, d.ldc2 = (0, 0) if c2 is None else (c2.data_ptr(), c2.stride(0))
    d.b_kn = int(b_kn)
    check(_lib.lib().uvx_gemm(stream_ptr(), dt, C.byref(d)), "uvx_gemm")
    return out


def gemm_splitk(a: torch.Tensor, b: torch.Tensor, *, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                act: str = "none", epilogue: int = 0, c2: Optional[torch.Tensor] = None, alpha: float = 1.0, res_mod: int = 0,
                force_split: int = 0, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uvx_gemm_splitk: gemm() with split-K scratch (the prefill's few-hundred-row problems); force_split 0 = the cost model decides."""
    M, K = a.shape
    N = b.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=a.dtype)
    if workspace is None:
        workspace = torch.empty(int(_lib.lib().uvx_gemm_splitk_ws_bytes(M, N)), device=a.device, dtype=torch.uint8)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.bias = 0 if bias is None else bias.data_ptr()
    d.residual = 0 if residual is None else residual.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = a.stride(0), b.stride(0), out.stride(0)
    d.ldr = 0 if residual is None else residual.stride(0)
    d.res_mod, d.batch, d.alpha = res_mod, 1, alpha
    d.act = {"none": 0, "gelu": 1}[act]
    d.epilogue = epilogue
    d.C2, d.ldc2 = (0, 0) if c2 is None else (c2.data_ptr(), c2.stride(0))
    check(_lib.lib().uvx_gemm_splitk(stream_ptr(), dtype_code(a.dtype), C.byref(d), ptr(workspace), C.c_size_t(workspace.numel()),
                                     int(force_split)), "uvx_gemm_splitk")
    return out


def gemm_rmsnorm(a: torch.Tensor, norm_w: torch.Tensor, b: torch.Tensor, *, eps: float = 1e-5, flavor: int = 0,
                 bias: Optional[torch.Tensor] = None, epilogue: int = 0, c2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epilogue(RMSNorm(a; norm_w) @ b[N,K]^T + bias) through uvx_gemm_rmsnorm (the decode step's fused norm + GEMV)."""
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty((M, N), device=a.device, dtype=a.dtype)
    scratch = torch.empty_like(a)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.bias = 0 if bias is None else bias.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = a.stride(0), b.stride(0), out.stride(0)
    d.batch, d.alpha, d.epilogue = 1, 1.0, epilogue
    d.C2, d.ldc2 = (0, 0) if c2 is None else (c2.data_ptr(), c2.stride(0))
    check(_lib.lib().uvx_gemm_rmsnorm(stream_ptr(), dtype_code(a.dtype), C.byref(d), ptr(norm_w), C.c_float(eps), int(flavor), ptr(scratch)),
          "uvx_gemm_rmsnorm")
    return out


def _code(t: torch.Tensor) -> int:
    return dtype_code(t.dtype)


def layernorm(x, w, b, eps=1e-5):
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    check(_lib.lib().uvx_layernorm(stream_ptr(), _code(x), ptr(x), ptr(w), ptr(b), ptr(y), rows, x.shape[-1],
                                   C.c_float(eps)), "uvx_layernorm")
    return y


def rmsnorm(x, w, eps=1e-6):
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    check(_lib.lib().uvx_rmsnorm(stream_ptr(), _code(x), ptr(x), ptr(w), ptr(y), rows, x.shape[-1], C.c_float(eps)),
          "uvx_rmsnorm")
    return y


def rmsnorm_bwd(dy, x, w, eps=1e-6, dx_add=None, want_dx=True, want_dw=False):
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.zeros(cols, device=x.device, dtype=torch.float32) if want_dw else None
    check(_lib.lib().uvx_rmsnorm_bwd(stream_ptr(), _code(x), ptr(dy), ptr(x), ptr(w), ptr(dx_add), ptr(dx), ptr(dw),
                                     rows, cols, C.c_float(eps)), "uvx_rmsnorm_bwd")
    return dx, dw


def qk_norm_rope_(qkv, wq, wk, cos_sin, T, Hq, Hkv, head_dim, eps=1e-6, keep_raw=False, flavor=0):
    """Qwen3 q_norm / k_norm + RoPE in place on the q | k columns of qkv [rows, ld]; -> the raw q | k rows when keep_raw."""
    rows = qkv.numel() // qkv.shape[-1]
    raw = torch.empty(rows, (Hq + Hkv) * head_dim, device=qkv.device, dtype=qkv.dtype) if keep_raw else None
    check(_lib.lib().uvx_qk_norm_rope(stream_ptr(), _code(qkv), ptr(qkv), ptr(wq), ptr(wk), ptr(raw), ptr(cos_sin), rows, T, Hq, Hkv,
                                      head_dim, qkv.shape[-1], C.c_float(eps), flavor), "uvx_qk_norm_rope")
    return raw


def qk_norm_bwd_(d_qkv, raw, wq, wk, Hq, Hkv, head_dim, eps=1e-6, flavor=0):
    """In place on the q | k columns of d_qkv [rows, ld]: gradient of the normalised rows -> gradient of the raw rows."""
    rows = d_qkv.numel() // d_qkv.shape[-1]
    check(_lib.lib().uvx_qk_norm_bwd(stream_ptr(), _code(d_qkv), ptr(d_qkv), ptr(raw), ptr(wq), ptr(wk), rows, Hq, Hkv, head_dim,
                                     d_qkv.shape[-1], C.c_float(eps), flavor), "uvx_qk_norm_bwd")
    return d_qkv


def swiglu(x, gate_first=False):
    half = x.shape[-1] // 2
    out = torch.empty(*x.shape[:-1], half, device=x.device, dtype=x.dtype)
    check(_lib.lib().uvx_swiglu(stream_ptr(), _code(x), ptr(x), ptr(out), x.numel() // x.shape[-1], half,
                                int(gate_first)), "uvx_swiglu")
    return out


def swiglu_bwd(dout, x, gate_first=False):
    half = x.shape[-1] // 2
    din = torch.empty_like(x)
    check(_lib.lib().uvx_swiglu_bwd(stream_ptr(), _code(x), ptr(dout), ptr(x), ptr(din), x.numel() // x.shape[-1],
                                    half, int(gate_first)), "uvx_swiglu_bwd")
    return din


def rope_(x, cos_sin, T, n_heads, head_dim, inverse=False):
    """In place on x [rows, ld]: heads 0..n_heads-1 (contiguous from column 0) are rotated."""
    rows = x.numel() // x.shape[-1]
    check(_lib.lib().uvx_rope(stream_ptr(), _code(x), ptr(x), ptr(cos_sin), rows, T, n_heads, head_dim, x.shape[-1],
                              int(inverse)), "uvx_rope")
    return x


def _attn_desc(q, k, v, o, lse, causal, block, scale, kv_start, kv_len, window=0):
    B, T, Hq, D = q.shape
    d = _lib.AttnDesc()
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.lse = 0 if lse is None else lse.data_ptr()
    d.kv_start = 0 if kv_start is None else kv_start.data_ptr()
    d.kv_len = 0 if kv_len is None else kv_len.data_ptr()
    d.B, d.T, d.Hq, d.Hkv, d.D = B, T, Hq, k.shape[2], D
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(1), k.stride(1), v.stride(1), o.stride(1)
    d.causal, d.block, d.scale, d.window = int(causal), int(block), scale, int(window)
    return d


def attention(q, k, v, causal=False, block=0, scale=None, kv_start=None, kv_len=None, need_lse=True, window=0):
    """q [B,T,Hq,D], k/v [B,T,Hkv,D] (last two dims contiguous, token stride free) -> o [B,T,Hq*D], lse."""
    B, T, Hq, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty(B, T, Hq * D, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, Hq, T, device=q.device, dtype=torch.float32) if need_lse else None
    d = _attn_desc(q, k, v, o, lse, causal, block, scale, kv_start, kv_len, window)
    nb = _lib.lib().uvx_attention_ws_bytes(_code(q), C.byref(d), 0)
    ws = torch.empty(nb, device=q.device, dtype=torch.uint8)
    check(_lib.lib().uvx_attention_fwd(stream_ptr(), _code(q), C.byref(d), ptr(ws), C.c_size_t(nb)), "uvx_attention_fwd")
    return o, lse


def attention_bwd(q, k, v, o, lse, dout, causal=False, block=0, scale=None, kv_start=None, kv_len=None, window=0):
    B, T, Hq, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    d = _attn_desc(q, k, v, o, lse, causal, block, scale, kv_start, kv_len, window)
    d.dout, d.dq, d.dk, d.dv = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.lddq, d.lddk, d.lddv = dq.stride(1), dk.stride(1), dv.stride(1)
    nb = _lib.lib().uvx_attention_ws_bytes(_code(q), C.byref(d), 1)
    ws = torch.empty(nb, device=q.device, dtype=torch.uint8)
    check(_lib.lib().uvx_attention_bwd(stream_ptr(), _code(q), C.byref(d), ptr(ws), C.c_size_t(nb)), "uvx_attention_bwd")
    return dq, dk, dv


def ce_loss(logits, labels, want_grad=True, grad_scale=1.0, in_place=False):
    """logits [B,T,V], labels [B,T] int64 -> (loss f32 scalar tensor, dlogits or None)."""
    B, T, V = logits.shape
    loss = torch.zeros(1, device=logits.device, dtype=torch.float32)
    dl = (logits if in_place else torch.empty_like(logits)) if want_grad else None
    scratch = torch.empty(2 + B * T, device=logits.device, dtype=torch.float32)
    check(_lib.lib().uvx_ce_loss(stream_ptr(), _code(logits), ptr(logits), ptr(labels.contiguous()), ptr(loss), ptr(dl),
                                 B, T, V, logits.stride(1), C.c_float(grad_scale), ptr(scratch)), "uvx_ce_loss")
    return loss[0], dl


def kl_loss(student, teacher, pair_row, pair_w, temperature, want_grad=True, grad_scale=1.0):
    """student [R, V], teacher [Rt, V]; pair_row int32 [2, R], pair_w f32 [2, R] -> (loss, dlogits or None)."""
    R, V = student.shape
    loss = torch.zeros(1, device=student.device, dtype=torch.float32)
    dl = torch.empty_like(student) if want_grad else None
    scratch = torch.empty(R, device=student.device, dtype=torch.float32)
    check(_lib.lib().uvx_kl_loss(stream_ptr(), _code(student), ptr(student), ptr(teacher), ptr(pair_row.contiguous()),
                                 ptr(pair_w.contiguous()), ptr(loss), ptr(dl), C.c_int64(R), V, student.stride(0),
                                 teacher.stride(0), C.c_float(temperature), C.c_float(grad_scale), ptr(scratch)), "uvx_kl_loss")
    return loss[0], dl


def layernorm_bwd(dy, x, w, eps=1e-5, dx_add=None):
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    dx = torch.empty_like(x)
    check(_lib.lib().uvx_layernorm_bwd(stream_ptr(), _code(x), ptr(dy), ptr(x), ptr(w), ptr(dx_add), ptr(dx), rows, cols,
                                       C.c_float(eps)), "uvx_layernorm_bwd")
    return dx


def gelu(pre):
    out = torch.empty_like(pre)
    check(_lib.lib().uvx_gelu(stream_ptr(), _code(pre), ptr(pre), ptr(out), C.c_int64(pre.numel())), "uvx_gelu")
    return out


def gelu_bwd(dout, pre):
    din = torch.empty_like(pre)
    check(_lib.lib().uvx_gelu_bwd(stream_ptr(), _code(pre), ptr(dout), ptr(pre), ptr(din), C.c_int64(pre.numel())), "uvx_gelu_bwd")
    return din


def _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter):
    """The bookkeeping buffers of a select entry point, those that are not given created (every row unfinished, a one-column `sequences`, a zero
    counter): -> (their part of the returned dict, the argument tail from eos_ids to counter)."""
    B, dev = logits.shape[0], logits.device
    eos = torch.empty(0, device=dev, dtype=torch.int64) if eos_ids is None else eos_ids
    out = dict(tokens=torch.empty(B, device=dev, dtype=torch.int64),
               unfinished=torch.ones(B, device=dev, dtype=torch.int32) if unfinished is None else unfinished,
               sequences=torch.zeros(B, col + 1, device=dev, dtype=torch.int64) if sequences is None else sequences,
               positions=None if positions0 is None else torch.empty(B, device=dev, dtype=torch.int32),
               counter=torch.zeros(2, device=dev, dtype=torch.int32) if counter is None else counter)
    # (the 64-bit ones by type: uvx_greedy_select has no argtypes)
    tail = (ptr(eos), eos.numel(), C.c_int64(int(pad)), ptr(out["unfinished"]), ptr(out["tokens"]), ptr(out["sequences"]),
            C.c_int64(out["sequences"].stride(0)), C.c_int64(int(col)), ptr(positions0), ptr(out["positions"]), int(step), ptr(out["counter"]))
    return out, tail


def _check_seen(name, seen, B):
    if seen.dtype != torch.int32 or seen.dim() != 2 or seen.shape[0] != B or not seen.is_contiguous():      # (the kernel strides the rows by shape[1])
        raise ValueError(f"{name}: `seen` has to be a contiguous int32 [B, words] tensor, but is {seen.dtype} {tuple(seen.shape)} "
                         f"with strides {tuple(seen.stride())}")


def greedy_select(logits, *, eos_ids=None, pad=0, unfinished=None, sequences=None, col=0, positions0=None, step=0, counter=None):
    """uvx_greedy_select on a [B, V] logits matrix (include/uvx.h): -> dict(tokens int64 [B], unfinished int32 [B], sequences int64 [B, n],
    positions int32 [B] or None, counter int32 [2]).  Bookkeeping buffers that are not given are created: every row unfinished, a one-column
    `sequences`, a zero counter."""
    B, V = logits.shape
    logits = logits.contiguous()
    out, book = _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter)
    check(_lib.lib().uvx_greedy_select(stream_ptr(), _code(logits), ptr(logits), B, V, *book), "uvx_greedy_select")
    return out


def sample_select(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, min_keep=1, seed=0, offset=0, uniforms=None, want_probs=False,
                  eos_ids=None, pad=0, unfinished=None, sequences=None, col=0, positions0=None, step=0, counter=None):
    """uvx_sample_select on a [B, V] logits matrix (include/uvx.h): greedy_select's keywords and its dict, plus probs f32 [B, V] or None."""
    B, V = logits.shape
    logits = logits.contiguous()
    out, book = _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter)
    probs = torch.empty(B, V, device=logits.device, dtype=torch.float32) if want_probs else None
    check(_lib.lib().uvx_sample_select(stream_ptr(), _code(logits), ptr(logits), B, V, float(temperature), int(top_k), float(top_p), float(min_p),
                                       int(min_keep), int(seed), int(offset), ptr(uniforms), ptr(probs), *book), "uvx_sample_select")
    return dict(out, probs=probs)


def seen_words(V: int) -> int:
    """Words of one row of the `seen` bitmap of uvx_seen_mark / uvx_greedy_select_penalized: ceil(V / 32)."""
    return (int(V) + 31) // 32


def seen_mark(ids, V, seen=None):
    """uvx_seen_mark (include/uvx.h): ORs the bits of ids int64 [B, n] (unit stride along n, any row stride) into the bitmap `seen`
    (int32 [B, >= ceil(V / 32)], the kernel's uint32 words; a zeroed one is created if not given) -> seen."""
    B, n = ids.shape
    if ids.dtype != torch.int64 or (n > 1 and ids.stride(1) != 1):
        ids = ids.to(torch.int64).contiguous()
    if seen is None:
        seen = torch.zeros(B, seen_words(V), device=ids.device, dtype=torch.int32)
    check(_lib.lib().uvx_seen_mark(stream_ptr(), ptr(ids), ids.stride(0), B, n, int(V), ptr(seen), seen.shape[1]), "uvx_seen_mark")
    return seen


def greedy_select_penalized(logits, seen, penalty, *, want_scores=False, eos_ids=None, pad=0, unfinished=None, sequences=None, col=0, positions0=None,
                            step=0, counter=None):
    """uvx_greedy_select_penalized on a [B, V] logits matrix and its `seen` bitmap (int32 [B, words], updated in place): greedy_select's keywords
    and its dict, plus scores f32 [B, V] or None and `seen`."""
    B, V = logits.shape
    _check_seen("greedy_select_penalized", seen, B)
    logits = logits.contiguous()
    out, book = _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter)
    scores = torch.empty(B, V, device=logits.device, dtype=torch.float32) if want_scores else None
    check(_lib.lib().uvx_greedy_select_penalized(stream_ptr(), _code(logits), ptr(logits), B, V, float(penalty), ptr(seen), seen.shape[1], ptr(scores),
                                                 *book), "uvx_greedy_select_penalized")
    return dict(out, scores=scores, seen=seen)


def sample_select_penalized(logits, seen, penalty, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, min_keep=1, seed=0, offset=0, uniforms=None,
                            want_probs=False, eos_ids=None, pad=0, unfinished=None, sequences=None, col=0, positions0=None, step=0, counter=None):
    """uvx_sample_select_penalized on a [B, V] logits matrix and its `seen` bitmap (int32 [B, words], updated in place): sample_select's keywords
    and its dict, plus `seen`."""
    B, V = logits.shape
    _check_seen("sample_select_penalized", seen, B)
    logits = logits.contiguous()
    out, book = _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter)
    probs = torch.empty(B, V, device=logits.device, dtype=torch.float32) if want_probs else None
    check(_lib.lib().uvx_sample_select_penalized(stream_ptr(), _code(logits), ptr(logits), B, V, float(penalty), ptr(seen), seen.shape[1],
                                                 float(temperature), int(top_k), float(top_p), float(min_p), int(min_keep), int(seed), int(offset),
                                                 ptr(uniforms), ptr(probs), *book), "uvx_sample_select_penalized")
    return dict(out, probs=probs, seen=seen)


def ban_rules(device, *, ngram=0, bad_words=(), min_ids=(), forced_ids=(), suppress_ids=(), begin_ids=()):
    """The rules of the banned selectors on `device`: -> (uvx_ban_rules_t mirror, the tensors its pointers refer to - keep them alive with it).
    bad_words: a list of id lists, flattened to tokens + offsets (lone-EOS entries are the caller's to drop, as generation.ScoreProcessors does)."""
    def ids(v, dtype=torch.int64):
        return torch.tensor(list(map(int, v)), device=device, dtype=dtype) if len(v) else None
    offsets = [0]
    for w in bad_words:
        offsets.append(offsets[-1] + len(w))
    t = dict(bad_tokens=ids([t for w in bad_words for t in w]), bad_offsets=ids(offsets, torch.int32) if len(bad_words) else None, min_ids=ids(min_ids),
             forced_ids=ids(forced_ids), suppress_ids=ids(suppress_ids), begin_ids=ids(begin_ids))
    rules = _lib.BanRules(**{k: ptr(v) for k, v in t.items()}, ngram=int(ngram), n_bad=len(bad_words), n_bad_tokens=offsets[-1], n_min=len(min_ids),
                          n_forced=len(forced_ids), n_suppress=len(suppress_ids), n_begin=len(begin_ids))
    return rules, t


def _ban_args(name, logits, seen, rules, ban):
    B, V = logits.shape
    if seen is not None:
        _check_seen(name, seen, B)
    if ban is None:
        ban = torch.empty(B, seen_words(V), device=logits.device, dtype=torch.int32)
    _check_seen(name, ban, B)
    if isinstance(rules, tuple):
        rules = rules[0]
    return ban, (C.byref(rules),), (ptr(seen), 0 if seen is None else seen.shape[1])


def greedy_select_banned(logits, rules, flags=0, *, seen=None, penalty=1.0, ban=None, want_scores=False, eos_ids=None, pad=0, unfinished=None,
                         sequences=None, col=0, positions0=None, step=0, counter=None):
    """uvx_greedy_select_banned on a [B, V] logits matrix (include/uvx.h): rules from ban_rules(), flags the step's UVX_BAN_* word, `sequences` the
    rows the n-gram and bad-word rules read (columns below `col`); seen / penalty as greedy_select_penalized (None: no penalty); `ban` int32
    [B, words] (created if not given, rewritten by the launch).  greedy_select_penalized's dict plus `ban`."""
    B, V = logits.shape
    ban, rl, pen = _ban_args("greedy_select_banned", logits, seen, rules, ban)
    logits = logits.contiguous()
    out, book = _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter)
    scores = torch.empty(B, V, device=logits.device, dtype=torch.float32) if want_scores else None
    check(_lib.lib().uvx_greedy_select_banned(stream_ptr(), _code(logits), ptr(logits), B, V, float(penalty), *pen, ptr(scores), *rl, int(flags), ptr(ban),
                                              ban.shape[1], *book), "uvx_greedy_select_banned")
    return dict(out, scores=scores, seen=seen, ban=ban)


def sample_select_banned(logits, rules, flags=0, *, seen=None, penalty=1.0, ban=None, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, min_keep=1, seed=0,
                         offset=0, uniforms=None, want_probs=False, eos_ids=None, pad=0, unfinished=None, sequences=None, col=0, positions0=None, step=0,
                         counter=None):
    """uvx_sample_select_banned on a [B, V] logits matrix: greedy_select_banned's rule arguments, sample_select's keywords and its dict, plus
    `seen` and `ban`."""
    B, V = logits.shape
    ban, rl, pen = _ban_args("sample_select_banned", logits, seen, rules, ban)
    logits = logits.contiguous()
    out, book = _select_book(logits, eos_ids, pad, unfinished, sequences, col, positions0, step, counter)
    probs = torch.empty(B, V, device=logits.device, dtype=torch.float32) if want_probs else None
    check(_lib.lib().uvx_sample_select_banned(stream_ptr(), _code(logits), ptr(logits), B, V, float(penalty), *pen, float(temperature), int(top_k),
                                              float(top_p), float(min_p), int(min_keep), int(seed), int(offset), ptr(uniforms), ptr(probs), *rl, int(flags),
                                              ptr(ban), ban.shape[1], *book), "uvx_sample_select_banned")
    return dict(out, probs=probs, seen=seen, ban=ban)


# ---- polyphase resampling (uvx_resample_poly) ----
RESAMPLE_TILE = 256          # outputs of one row per block: TILE of csrc/resample.h (the tests put n_out on either side of it)
RESAMPLE_MAX_RATIO = 1024    # up and down are each at most this: MAX_RATIO of csrc/resample.h
_resample_taps = {}          # (up, down, device) -> (f32 taps on the device, half)


def design_resample_taps(up: int, down: int):
    """The low-pass filter scipy.signal.resample_poly designs by default, in numpy alone: with m = max(up, down) and half = 10 * m,
    firwin(2 * half + 1, 1 / m, window=("kaiser", 5.0)) * up.  -> (taps float64 [2 * half + 1], half); taps[half + t] is the weight at lag t."""
    import numpy as np

    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"design_resample_taps: up={up} and down={down} must be at least 1")
    m = max(up, down)
    half = 10 * m
    t = np.arange(-half, half + 1, dtype=np.float64)
    w = np.sinc(t / m) / m * np.kaiser(2 * half + 1, 5.0)
    return up * w / w.sum(), half


def resample_ratio(sample_rate: int, target_rate: int = 16000):
    """-> (up, down) of the reduced fraction target_rate / sample_rate; a ValueError that names the limit if the kernel is not built for it."""
    import math

    sample_rate = int(sample_rate)
    if sample_rate < 1:
        raise ValueError(f"sample rate {sample_rate} must be positive")
    g = math.gcd(target_rate, sample_rate)
    up, down = target_rate // g, sample_rate // g
    if max(up, down) > RESAMPLE_MAX_RATIO:
        raise ValueError(f"cannot resample {sample_rate} Hz to {target_rate} Hz on the device: the ratio {up}/{down} is beyond the kernel's limit of "
                         f"{RESAMPLE_MAX_RATIO} for either term (there is no other resampler behind it)")
    return up, down


def resample_taps_device(up: int, down: int, device):
    """design_resample_taps rounded once to f32, on `device`; cached per (up, down, device).  -> (taps, half)"""
    key = (int(up), int(down), str(torch.device(device)))
    if key not in _resample_taps:
        taps, half = design_resample_taps(up, down)
        _resample_taps[key] = (torch.from_numpy(taps.astype("float32")).to(device), half)
    return _resample_taps[key]


def resample_n_out(n: int, up: int, down: int) -> int:
    return -(-int(n) * int(up) // int(down))


def resample_poly(pcm, row_offset, n_in, up, down, *, max_n_in, taps=None, half=None, out=None, out_width=None):
    """uvx_resample_poly (include/uvx.h).  pcm: 1-D int16 or f32 device tensor holding every row; row_offset int64 [B] and n_in int32 [B] on the
    device; max_n_in: the host's copy of max(n_in).  taps / half default to the cached scipy-default design.  out: f32 [B, >= out_width] with unit
    stride along a row (created as [B, out_width] if not given); out_width defaults to the n_out of max_n_in.  -> out"""
    up, down = int(up), int(down)
    if max(up, down) > RESAMPLE_MAX_RATIO:
        raise ValueError(f"resample_poly: up={up} down={down} is beyond the kernel's limit of {RESAMPLE_MAX_RATIO} for either term")
    if pcm.dtype not in (torch.int16, torch.float32) or pcm.dim() != 1 or not pcm.is_contiguous():
        raise ValueError(f"resample_poly: pcm has to be a contiguous 1-D int16 or float32 tensor, but is {pcm.dtype} {tuple(pcm.shape)}")
    if row_offset.dtype != torch.int64 or n_in.dtype != torch.int32 or row_offset.shape != n_in.shape or n_in.dim() != 1:
        raise ValueError("resample_poly: row_offset has to be int64 [B] and n_in int32 [B]")
    B = n_in.shape[0]
    if B == 0:
        return torch.empty(0, int(out_width or 0), device=pcm.device, dtype=torch.float32) if out is None else out
    if taps is None:
        taps, half = resample_taps_device(up, down, pcm.device)
    if out_width is None:
        out_width = resample_n_out(max_n_in, up, down) if out is None else out.shape[1]
    if out is None:
        out = torch.empty(B, out_width, device=pcm.device, dtype=torch.float32)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < out_width or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"resample_poly: out has to be f32 [B, >= out_width] with unit stride along a row, but is {out.dtype} {tuple(out.shape)}")
    check(_lib.lib().uvx_resample_poly(stream_ptr(), 1 if pcm.dtype == torch.int16 else 0, ptr(pcm), ptr(row_offset), ptr(n_in), B, int(max_n_in),
                                       up, down, ptr(taps), int(half), ptr(out), out.stride(0) if B > 1 else max(out.stride(0), out.shape[1]),
                                       int(out_width)), "uvx_resample_poly")
    return out


# ---- raw-waveform normalisation (uvx_wave_norm) ----
WAVENORM_CHUNK = 16384       # samples of one row per partial (S1, S2) pair: CHUNK of csrc/wavenorm.h (the tests put n on either side of it)


def wave_norm(pcm, row_offset, n, *, max_n, normalize=True, padding_value=0.0, out=None, out_width=None):
    """uvx_wave_norm (include/uvx.h).  pcm: 1-D int16 or f32 device tensor holding every row (resample_poly's input layout); row_offset int64
    [B] and n int32 [B] on the device; max_n: the host's copy of max(n).  normalize=False converts and pads only.  out: f32 [B, >= out_width]
    with unit stride along a row, not overlapping pcm (created as [B, out_width] if not given); out_width defaults to max_n.  The workspace
    is allocated here.  -> out"""
    if pcm.dtype not in (torch.int16, torch.float32) or pcm.dim() != 1 or not pcm.is_contiguous():
        raise ValueError(f"wave_norm: pcm has to be a contiguous 1-D int16 or float32 tensor, but is {pcm.dtype} {tuple(pcm.shape)}")
    if row_offset.dtype != torch.int64 or n.dtype != torch.int32 or row_offset.shape != n.shape or n.dim() != 1:
        raise ValueError("wave_norm: row_offset has to be int64 [B] and n int32 [B]")
    B = n.shape[0]
    if B == 0:
        return torch.empty(0, int(out_width or 0), device=pcm.device, dtype=torch.float32) if out is None else out
    if out_width is None:
        out_width = int(max_n) if out is None or out.dim() != 2 else out.shape[1]
    if out is None:
        out = torch.empty(B, out_width, device=pcm.device, dtype=torch.float32)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < out_width or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"wave_norm: out has to be f32 [B, >= out_width] with unit stride along a row, but is {out.dtype} {tuple(out.shape)}")
    l = _lib.lib()
    ws_bytes = int(l.uvx_wave_norm_ws_bytes(B, int(max_n))) if normalize else 0
    ws = torch.empty(ws_bytes, device=pcm.device, dtype=torch.uint8) if ws_bytes else None
    check(l.uvx_wave_norm(stream_ptr(), 1 if pcm.dtype == torch.int16 else 0, ptr(pcm), ptr(row_offset), ptr(n), B, int(max_n), int(bool(normalize)),
                          float(padding_value), ptr(out), out.stride(0) if B > 1 else max(out.stride(0), out.shape[1]), int(out_width), ptr(ws),
                          ws_bytes), "uvx_wave_norm")
    return out


AUG_IIR_BLOCK = 256          # outputs one filter thread produces after its warm-up: BLOCK of csrc/aug.h
AUG_IIR_MAX_ORDER = 16       # MAX_ORDER of csrc/aug.h
AUG_FFT_LDS_SPAN = 4096      # complex elements of the noise transform held in LDS: LDS_SPAN of csrc/aug.h (M <= 2 * span needs no global pass)
AUG_NOISE_MAX_N = 1 << 21    # coloured noise: the longest row (2^MAX_LOG2_M of csrc/aug.h)
AUG_COLOURS = {"white": 0, "pink": 1, "brown": 2, "blue": 3, "violet": 4}


def _aug_layout(what, pcm, row_offset, n, max_n, out, out_width):
    """The argument checks and the output buffer the three uvx_aug_* wrappers share (wave_norm's layout).  -> (B, out, out_width, stride)"""
    if pcm.dtype not in (torch.int16, torch.float32) or pcm.dim() != 1 or not pcm.is_contiguous():
        raise ValueError(f"{what}: pcm has to be a contiguous 1-D int16 or float32 tensor, but is {pcm.dtype} {tuple(pcm.shape)}")
    if row_offset.dtype != torch.int64 or n.dtype != torch.int32 or row_offset.shape != n.shape or n.dim() != 1:
        raise ValueError(f"{what}: row_offset has to be int64 [B] and n int32 [B]")
    B = n.shape[0]
    if out_width is None:
        out_width = int(max_n) if out is None or out.dim() != 2 else out.shape[1]
    if out is None:
        out = torch.empty(B, out_width, device=pcm.device, dtype=torch.float32)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < out_width or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"{what}: out has to be f32 [B, >= out_width] with unit stride along a row, but is {out.dtype} {tuple(out.shape)}")
    return B, out, int(out_width), (out.stride(0) if B > 1 else max(out.stride(0), out.shape[1]))


def _aug_per_row(what, name, t, dtype, B, device):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=dtype).reshape(-1).to(device)
    if t.dtype != dtype or t.shape != (B,) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{what}: {name} has to be a contiguous {dtype} [B] tensor on the clips' device, but is {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def aug_gain(pcm, row_offset, n, gain, *, max_n, out=None, out_width=None):
    """uvx_aug_gain (include/uvx.h): out[b][i] = clip(x_i * gain[b], -1, 1), zero beyond n[b].  pcm, row_offset, n, max_n, out, out_width: as for
    wave_norm.  gain: f32 [B] (a device tensor, or host numbers that go up here).  -> out"""
    B, out, out_width, stride = _aug_layout("aug_gain", pcm, row_offset, n, max_n, out, out_width)
    if B == 0:
        return out
    gain = _aug_per_row("aug_gain", "gain", gain, torch.float32, B, pcm.device)
    check(_lib.lib().uvx_aug_gain(stream_ptr(), 1 if pcm.dtype == torch.int16 else 0, ptr(pcm), ptr(row_offset), ptr(n), B, int(max_n), ptr(gain),
                                  ptr(out), stride, out_width), "uvx_aug_gain")
    return out


def aug_iir(pcm, row_offset, n, b, a, warm, *, max_n, out=None, out_width=None):
    """uvx_aug_iir (include/uvx.h): scipy.signal.lfilter(b, a, x) per row by warm-up blocks.  b, a: f64 [order + 1] device tensors with a[0] == 1
    (the caller normalises); warm: the look-back in samples (ultravox_amd.aug.iir_warm_len).  -> out"""
    B, out, out_width, stride = _aug_layout("aug_iir", pcm, row_offset, n, max_n, out, out_width)
    if b.dtype != torch.float64 or a.dtype != torch.float64 or b.dim() != 1 or b.shape != a.shape or b.device != pcm.device or a.device != pcm.device \
            or not (b.is_contiguous() and a.is_contiguous()):
        raise ValueError("aug_iir: b and a have to be contiguous float64 [order + 1] tensors on the clips' device")
    if B == 0:
        return out
    check(_lib.lib().uvx_aug_iir(stream_ptr(), 1 if pcm.dtype == torch.int16 else 0, ptr(pcm), ptr(row_offset), ptr(n), B, int(max_n), ptr(b), ptr(a),
                                 b.shape[0] - 1, int(warm), ptr(out), stride, out_width), "uvx_aug_iir")
    return out


def aug_noise(pcm, row_offset, n, noise_ratio, *, colour, seed, offset, max_n, out=None, out_width=None):
    """uvx_aug_noise (include/uvx.h): adds noise of `colour` (a name of AUG_COLOURS or its number) at noise_ratio[b] = 10^(-snr_db / 10) times the
    row's own power.  noise_ratio: f64 [B] (a device tensor, or host numbers that go up here).  The workspace is allocated here.  -> out"""
    colour = AUG_COLOURS[colour] if isinstance(colour, str) else int(colour)
    B, out, out_width, stride = _aug_layout("aug_noise", pcm, row_offset, n, max_n, out, out_width)
    if B == 0:
        return out
    noise_ratio = _aug_per_row("aug_noise", "noise_ratio", noise_ratio, torch.float64, B, pcm.device)
    l = _lib.lib()
    ws_bytes = int(l.uvx_aug_noise_ws_bytes(B, int(max_n), colour))
    ws = torch.empty(ws_bytes, device=pcm.device, dtype=torch.uint8) if ws_bytes else None
    check(l.uvx_aug_noise(stream_ptr(), 1 if pcm.dtype == torch.int16 else 0, ptr(pcm), ptr(row_offset), ptr(n), B, int(max_n), colour,
                          ptr(noise_ratio), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(out), stride, out_width, ptr(ws), ws_bytes),
          "uvx_aug_noise")
    return out
