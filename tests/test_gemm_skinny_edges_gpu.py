"""The few-row bf16 GEMM kernels (ultravox_amd/csrc/gemm_skinny.hip: the row-streaming kernel, the fragment-load and the LDS-staged MFMA kernels, and the
two fused-RMSNorm prologues of uvx_gemm_rmsnorm) at their row, column and K-span edges, element by element against the float64 reference of
gemm_edge_util.py / gemm_skinny_edge_util.py.  Every case goes through uvx_gemm (uvx_gemm_rmsnorm) with the variant left automatic; the
profiler's record proves the path (200 = the few-row kernels, 201 / 202 = the fused row / staged kernel, below 100 = a tile), and
gemm_skinny_edge_util.served_by - the dispatcher restated, with the device's CU count - says which of the three kernels that was.

Every operand sits inside a larger buffer of canaries: padding, rows after M, columns after N (where the clamped weight rows would land) and
the space around come back bit for bit, inputs and norm weights included; a second call from the same buffers is bit-identical; every output
is finite; families S / Sb are BIT-EQUAL to the exact chain in every output without a transcendental (their sums are exact in any order: the
v_dot2 chains and the butterfly included); families R and G stay within the bars, the fused cases with the tippable activations' term.
test_gemm_skinny_edges_cpu.py shows that an f32 restatement of each kernel's summation order stays within these bars and that every
off-by-one of the index arithmetic breaks them.

Largest error seen on an MI355X, in bar units per kernel and output kind, with the case and family (the restatement's figures are in
test_gemm_skinny_edges_cpu.py):
  rows    plain 0.988 rows-1x4092x64, G            bias 0.977 rows-1x4092x64-r0, G          alpha 0.995 rows-2x24572x192, R
          bias_gelu 0.899 rows-1x24572x192-r0, G   bias_res 0.964 rows-1x24572x192, G       res_mod 0.964 rows-1x24572x192, G
          bias_gelu_res 0.952 rows-2x24572x192, G  ep1 0.939 ld-2x96x576 (ldc2 + 4), R      ep1.C2 0.532 ld-2x96x576 (ldc2 + 12), G
  frag    plain 0.995 frag-3x16388x64, R           bias 0.971 frag-15x16x192, G             alpha 0.953 frag-16x16x64, R
          bias_gelu 0.933 frag-15x16404x64, G      bias_res 0.973 frag-3x16388x64, G        res_mod 0.975 frag-15x16404x64, G
          bias_gelu_res 0.773 ld-15x36x576, G      ep1 0.960 frag-16x96x576, R              ep1.C2 0.655 frag-16x96x576, G
  staged  plain 0.957 staged-33x36x2048, G         bias 0.952 staged-33x36x2048, G          alpha 0.956 staged-49x20x6144, R
          bias_gelu 0.775 staged-17x20x2048, G     bias_res 0.959 staged-17x16388x2048, G   res_mod 0.881 staged-31x36x4096, G
          bias_gelu_res 0.703 staged-16x36x6144, G ep1 0.962 staged-33x96x2048, G           ep1.C2 0.597 ld-33x96x2048, G
  fused row kernel (201)     plain 0.990 fused_rows-1x4092x576-f0, R    bias 0.977 fused_rows-2x36x8192-f1-small, R   bias_res 0.920 fused_rows-2x4092x64-f1-small, G
                             ep1 0.947 fused_rows-1x96x576-f1, G        ep1.C2 0.489 fused_rows-1x96x576-f1, G
  fused staged kernel (202)  plain 0.894 fused_staged-15x20x4096-f1, R  bias 0.970 fused_staged-3x16388x2048-f1, G    bias_gelu 0.407 fused_staged-16x20x2048-f1, G
                             bias_res 0.761 fused_staged-16x20x4096-f0, G   ep1 0.988 fused_staged-15x96x2048-f1, R   ep1.C2 0.576 fused_staged-15x96x2048-f1, R
Every kind equals the restatement's figure to three digits (the CPU test counts the fused cases with the kernel whose prologue they run): the
error is the bf16 roundings', neither the summation order nor the hardware exp shows at this scale.  Bit-equality, every canary, the second
call and the path (200 / 201 / 202 / a tile) held in all 122 tests; the launch at M = 2, K = 16384 - 64 KiB of dynamic LDS beside the 2 KiB of
static reduction arrays - is accepted (a work-group of gfx950 may take up to 160 KiB) and within its bars.  At 256 CUs N = 4 is one block of
SIXTEEN weight rows (no balance gain from eight: the 5 % rule keeps the larger block), all clamped to row 3; 8 rows per block start at N = 12.
"""
import contextlib
import ctypes as C

import pytest
import torch

import gemm_edge_util as U
import gemm_skinny_edge_util as S
from gemm_edge_util import HEAD
from gemm_skinny_edge_util import CASES, case_id, families, make_problem, with_form

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from ultravox_amd import _lib as L
    return L


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _desc(p):
    g, b = p.g, p.buf
    at = lambda name: b[name].data_ptr() + HEAD * b[name].element_size() if name in b else 0
    d = _lib().GemmDesc()
    d.A, d.B, d.C, d.bias, d.residual, d.C2 = at("A"), at("B"), at("C"), at("bias"), at("R"), at("C2")
    d.M, d.N, d.K = g["M"], g["N"], g["K"]
    d.lda, d.ldb, d.ldc, d.ldr, d.ldc2 = g["lda"], g["ldb"], g["ldc"], g["ldr"] if g["Mr"] else 0, g["ldc2"] if g["W2"] else 0
    d.res_mod, d.batch = g["res_mod"], 1
    d.act, d.out_f32, d.accumulate, d.alpha = g["act"], 0, 0, g["alpha"]
    d.epilogue, d.b_kn = g["epi"], 0
    return d


def _records():
    """the profiler's GEMM records since uvx_prof_begin -> [(M, N, K, batch, variant)]; ends the region"""
    L = _lib().lib()
    buf, tot = (C.c_double * (6 * 16))(), (C.c_double * 12)()
    n = L.uvx_prof_records(buf, 16)
    L.uvx_prof_end(tot, 3)
    return [tuple(int(buf[i * 6 + j]) for j in range(5)) for i in range(n)]


def _launch(p, norm_out=None):
    L = _lib()
    d = _desc(p)
    if S.fused(p.c):
        w = p.buf["W"].data_ptr() + HEAD * 2
        L.check(L.lib().uvx_gemm_rmsnorm(L.stream_ptr(), L.BF16, C.byref(d), C.c_void_p(w), C.c_float(S.NORM_EPS), p.c["flavor"], L.ptr(norm_out)), "uvx_gemm_rmsnorm")
    else:
        L.check(L.lib().uvx_gemm(L.stream_ptr(), L.BF16, C.byref(d)), "uvx_gemm")


def _held(p, what):
    """Two calls from the same initial buffers: bit-identical; the first one against the reference (and the exact chain).  -> the first call's records"""
    outs = p.outputs()
    first = {k: v.clone() for k, v in p.buf.items()}
    norm_out = torch.empty(p.g["M"] * p.g["K"], device=DEV, dtype=torch.bfloat16) if S.fused(p.c) else None
    _lib().lib().uvx_prof_begin()
    try:
        _launch(p, norm_out)
    finally:
        recs = _records()
    got = {k: p.buf[k].clone() for k in outs}
    for k in outs:
        p.buf[k].copy_(first[k])
    _launch(p, norm_out)
    for k in outs:
        assert torch.equal(U.output_bits(p.buf[k]), U.output_bits(got[k])), f"{what}: the second call's {k} differs"
        p.buf[k].copy_(first[k])
    for k, v in p.buf.items():                       # inputs, norm weights, their padding and canaries are read only
        assert k in outs or torch.equal(U.output_bits(v), U.output_bits(first[k])), f"{what}: the call wrote into {k}"
    exact = S.kernel_images(p, S.operands(p)) if S.biteq_outputs(p) else None
    ref = S.reference(p)
    if S.fused(p.c):
        assert p.tips[0] <= S.TIP_CAP, f"{what}: {p.tips[0]:.2e} of the activations are tippable"
    res = U.compare(p, ref, got, exact)
    print(f"EDGE {what}: " + "  ".join(f"{S.kind(p, k)} {r['worst']:.3f}" for k, r in res.items()))
    U.assert_ok(p, res, what)
    if p.c.get("zero_row") is not None and p.c["kind"] == "bias":      # a row of zeros: rstd = eps^-1/2 is finite and the output is the bias itself
        g = p.g
        row = got["C"][HEAD + p.c["zero_row"] * g["ldc"]:][:g["N"]]
        assert torch.equal(U.output_bits(row), U.output_bits(p.buf["bias"][HEAD:HEAD + g["N"]])), f"{what}: the all-zero row is not the bias"
    return recs


def _off_by_8_bytes(p):
    """C, C2, bias and residual 8 bytes off a 16-byte boundary: the loosest alignment the MFMA epilogues' 8-byte vector accesses admit"""
    buf = {}
    for k, v in p.buf.items():
        if k in ("C", "C2", "bias", "R"):
            moved = torch.empty(v.numel() + 8, dtype=v.dtype, device=v.device)[4:4 + v.numel()]
            assert moved.data_ptr() % 16 == 8
            buf[k] = moved.copy_(v)
        else:
            buf[k] = v
    q = U.Problem(p.c, p.family, p.g, buf)
    q.tips = None
    return q


def _for_device(c):
    """The case as listed where the device has the CU count the list was laid out for; otherwise the nearest N that keeps the row kernel's block
    height - and a ragged last block - under this device's count."""
    s = S.kernel_of(c)
    if _cus() == S.CUS or s is None or s[0] != "rows" or c["forms"] == ("ep1",):
        return c
    for n in range(c["N"], 8 * c["N"] + 64, 4):
        if S.rows_per_block(n, False, _cus()) == s[3] and (n % s[3] or not c["N"] % s[3]):
            return dict(c, N=n)
    pytest.fail(f"{case_id(c)}: no N with {s[3]} weight rows per block on {_cus()} CUs")


def _run(c, second=None):
    """every form and family of a case under its options; the record says which entry served it -> nothing"""
    c = _for_device(c)
    o4, o24, o26 = c.get("opt4", 1), c.get("opt24", 0), c.get("opt26")
    O = _lib().Option
    with contextlib.ExitStack() as options:      # the old values come back whatever happens inside
        for key, v in ((O.SKINNY_GEMM, o4), (O.SKINNY_RMSNORM_STAGED, o24), (O.GEMV_ROWS_IN_FLIGHT, o26)):
            if v is not None:
                options.enter_context(_lib().option(key, v))
        for form in c["forms"]:
            cf = with_form(c, form)
            sw = form == "ep1"
            if S.fused(c):
                code, s = S.fused_by(c["M"], c["N"], c["K"], o4, o24, o26 or 0, sw, _cus())
            else:
                s = S.served_by(c["M"], c["N"], c["K"], o4, o26 or 0, sw, _cus())
                code = 200 if s != "tiled" else 0
            assert s == (S.kernel_of(cf, _cus()) or "tiled")
            for fam in families(cf, form):
                p = make_problem(cf, fam, DEV)
                what = f"{case_id(c)} {form} family {fam} [{' '.join(str(x) for x in s) if s != 'tiled' else s}]"
                recs = _held(p, what)
                assert len(recs) == 1, f"{what}: {recs}"
                assert (recs[0][4] == code) if code else (recs[0][4] < 100), f"{what}: meant for {code or 'a tile'}, the record says {recs}"
                if second:
                    second(p, what)


def _group(name):
    return [c for c in CASES if c["group"] == name]


@pytest.mark.parametrize("c", _group("rows"), ids=case_id)
def test_row_streaming_kernel_at_its_k_step_block_and_in_flight_edges(c):
    """gemv_rows_bf16_k, M = 1 and 2: one partial 512-step, a full one, a full one and eight lanes, the second k-step of a trip under its guard,
    37 K-tiles; 8, 16 and 32 weight rows per block, each with a ragged (clamped) last block; 2, 4, 8, 16 rows in flight; SwiGLU blocks."""
    _run(c)


@pytest.mark.parametrize("c", _group("frag"), ids=case_id)
def test_fragment_load_mfma_kernel_at_its_chunk_mapping_and_unroll_edges(c):
    """gemm_skinny_bf16_k<TILES, false>, M = 3, 15, 16 (and 1, 2, 16 with option 4 = 2): span and interleave mapping, idle waves, unrolled trips with
    and without a remainder at both widths, one and two column tiles with four columns of the last block's first or second tile."""
    _run(c)


@pytest.mark.parametrize("c", _group("staged"), ids=case_id)
def test_staged_mfma_kernel_at_its_step_and_row_tile_edges(c):
    """gemm_skinny_bf16_k<TILES, true, MT>: one, two and three 256-column steps per wave, one, two and four activation row tiles on either side of
    each tile's last row, ragged N, SwiGLU, the reduction array laid over the staging buffer."""
    _run(c)


@pytest.mark.parametrize("c", _group("boundary"), ids=case_id)
def test_dispatch_boundaries_are_held_to_the_same_reference_on_either_side(c):
    """(M = 64, K = 2048) and (M = 16, K = 2112) are the last few-row problems, M + 1 goes to a tile; option 4 = 0 sends one row to a tile."""
    _run(c)


@pytest.mark.parametrize("c", _group("ld"), ids=case_id)
def test_padded_leading_dimensions_and_8_byte_alignment(c):
    _run(c, lambda p, what: _held(_off_by_8_bytes(p), what + " operands 8 bytes off"))


@pytest.mark.parametrize("c", _group("fused_rows"), ids=case_id)
def test_fused_rmsnorm_prologue_of_the_row_kernel(c):
    """uvx_gemm_rmsnorm at M = 1, 2: K from one partial vector per thread to the 16384 of the prologue (at M = 2 the 64 KiB of dynamic LDS itself,
    beside the static reduction arrays), both flavors, a row of mean square 3 eps, a row of zeros; K = 16448 runs as two launches."""
    _run(c)


def _two_launches(p, what):
    """option 24 = 0: the same problem is bit-identical to RMSNorm and GEMM as two calls (flavor 0: uvx_rmsnorm + uvx_gemm; flavor 1, which is not
    among the single-op entry points: uvx_gemm on the normalised rows the entry point itself left in norm_out)"""
    L = _lib()
    g, outs = p.g, p.outputs()
    first = {k: p.buf[k].clone() for k in outs}
    norm_out = torch.empty(g["M"] * g["K"], device=DEV, dtype=torch.bfloat16)
    with L.option(L.Option.SKINNY_RMSNORM_STAGED, 0):
        L.lib().uvx_prof_begin()
        try:
            _launch(p, norm_out)
        finally:
            recs = _records()
    assert len(recs) == 1 and recs[0][4] == 200, f"{what}: option 24 = 0 is the two launches: {recs}"
    got = {k: p.buf[k].clone() for k in outs}
    for k in outs:
        p.buf[k].copy_(first[k])
    normed = norm_out
    if p.c["flavor"] == 0:
        normed = torch.empty_like(norm_out)
        L.check(L.lib().uvx_rmsnorm(L.stream_ptr(), L.BF16, C.c_void_p(p.buf["A"].data_ptr() + HEAD * 2), C.c_void_p(p.buf["W"].data_ptr() + HEAD * 2), L.ptr(normed),
                                    g["M"], g["K"], C.c_float(S.NORM_EPS)), "uvx_rmsnorm")
        assert torch.equal(U.output_bits(normed), U.output_bits(norm_out))
    d = _desc(p)
    d.A = normed.data_ptr()
    L.check(L.lib().uvx_gemm(L.stream_ptr(), L.BF16, C.byref(d)), "uvx_gemm")
    for k in outs:
        assert torch.equal(U.output_bits(p.buf[k]), U.output_bits(got[k])), f"{what}: {k} differs from the two launches"
        p.buf[k].copy_(first[k])
    res = U.compare(p, S.reference(p), got)
    print(f"EDGE {what} option 24 = 0: " + "  ".join(f"{S.kind(p, k)} {r['worst']:.3f}" for k, r in res.items()))
    U.assert_ok(p, res, what + " option 24 = 0")


@pytest.mark.parametrize("c", _group("fused_staged"), ids=case_id)
def test_fused_rmsnorm_prologue_of_the_staged_kernel(c):
    """uvx_gemm_rmsnorm at M = 3, 15, 16 with option 24 = 1: the norm inside the staged kernel (record 202), both flavors, one and two column tiles,
    a small and a zero row; with option 24 = 0 the two launches, bit for bit."""
    _run(c, _two_launches)
