"""The bf16 tiled GEMM (uvx_gemm / uvx_gemm_splitk, ultravox_amd/csrc/gemm.hip) at its tile, K and stride edges, element by element against the
float64 reference of gemm_edge_util.py: every product tile variant (0, the eight-phase family 11 / 15..19, the merged-phase 31..34, the
three-buffer 59 / 60, the 32 x 32 x 16 kernels 61 / 62) at M = 1, bm - 1, bm, bm + 1, 2 bm + 1, N on either side of a tile and N % 8 != 0, K
shorter than the pipelines and with odd tile counts; act 2 / 3 and both SwiGLU epilogues through launch_variant's reroutes; the NN form; every
leading dimension padded; the batched form as the conv stems, the grouped positional conv and the K-cut LM-head gradient call it; split-K with
2, 3, 5, 16 slabs of 5 and 37 K-tiles; and the tail-split launch with proof (the profiler's record) that the second launch happened.

Every operand sits inside a larger buffer full of canaries (NaN bit patterns): padding columns of every leading dimension, rows after M, the
gaps between batch slabs and the space before and after must come back bit for bit (inputs included); the padded-ld and NN cases run a
second time with C, C2, bias and residual 8 bytes off a 16-byte boundary; every output is finite; a second call is bit-identical;
family S / Sb is BIT-EQUAL to the exact chain in every output without a transcendental.  test_gemm_edges_cpu.py shows that a float64
restatement of the kernels stays within these bars and that every off-by-one of the index arithmetic breaks them.

splitk_reduce_norm_k (the reduce with the following RMSNorm fused in) is reached only through GemmDesc::norm_w, which no single-op entry point
sets (uvx_gemm_splitk leaves it null): it stays with the prefill tests.  A forced split that leaves a slab without a K-tile (16 slabs of 5
K-tiles) falls back to the unsplit launch, as pick_split documents: asserted from the profiler's record.

Largest error seen on an MI355X, in bar units per output kind, with the case and family it came from (the restatement's figures are in
test_gemm_edges_cpu.py; bit-equality and every canary held in all 240 tests):
  plain     0.995  tiles-v15-161x132x64, G                 bias      0.996  tiles-v19-127x520x192, R
  alpha     0.996  tiles-v31-257x252x64, R                 bias_gelu 0.933  tiles-v11-513x256x64, G
  bias_res  0.988  tiles-v33-161x260x192, G                res_mod   0.989  tail-auto-130x16544x128, G (tail split)
  f32       0.150  tiles-v11-256x520x320, R                f32_acc   0.177  tiles-v61-255x252x2368, R
  act2      0.996  second-v32-192x256x128, R               act2.C2   0.933  second-v31-256x256x128, G
  act3      0.954  second-v33-161x260x192, G               ep2       0.973  tail-auto-130x16544x128, G (tail split)
  ep1       0.996  second-v33-161x288x192, R               ep1.C2    0.833  tail-auto-130x16544x128, G (tail split)
The bf16 kinds equal the restatement's figures to three digits: the error is the bf16 roundings'.  Only the f32 outputs differ from it (0.15 /
0.18 against 0.08 / 0.10): the MFMA's own 32-term sum is not exact, the bar's accumulation term leaves it a factor of five.
Variants 61 / 62 on their aligned cases (N = 264) and their twins 31 / 34 return the same bits - measured at 37 K-tiles, 0 of 135 432
elements differ - so no result tells which MFMA shape ran; that these cases meet launch_variant's `plain` condition is by reading it."""
import ctypes as C

import pytest
import torch

import gemm_edge_util as U
from gemm_edge_util import CASES, HEAD, case_id, families, make_problem, with_form

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from ultravox_amd import _lib as L
    return L


def _desc(p):
    g, b = p.g, p.buf
    at = lambda name: b[name].data_ptr() + HEAD * b[name].element_size() if name in b else 0
    d = _lib().GemmDesc()
    d.A, d.B, d.C, d.bias, d.residual, d.C2 = at("A"), at("B"), at("C"), at("bias"), at("R"), at("C2")
    d.M, d.N, d.K = g["M"], g["N"], g["K"]
    d.lda, d.ldb, d.ldc, d.ldr, d.ldc2 = g["lda"], g["ldb"], g["ldc"], g["ldr"] if g["Mr"] else 0, g["ldc2"] if g["W2"] else 0
    d.res_mod, d.batch = g["res_mod"], g["Z"]
    d.stride_a, d.stride_b, d.stride_c, d.stride_r = g["sA"], g["sB"], g["sC"], g["sR"]
    d.act, d.out_f32, d.accumulate, d.alpha = g["act"], int(g["out_f32"]), int(g["accumulate"]), g["alpha"]
    d.epilogue, d.b_kn = g["epi"], int(g["nn"])
    return d


def _records():
    """the profiler's GEMM records since uvx_prof_begin -> [(M, N, K, batch, variant)]; ends the region"""
    L = _lib().lib()
    buf, tot = (C.c_double * (6 * 16))(), (C.c_double * 12)()
    n = L.uvx_prof_records(buf, 16)
    L.uvx_prof_end(tot, 3)
    return [tuple(int(buf[i * 6 + j]) for j in range(5)) for i in range(n)]


def _launch(p, ws=None):
    L = _lib()
    d = _desc(p)
    s = p.c.get("split", 0)
    if s:
        L.check(L.lib().uvx_gemm_splitk(L.stream_ptr(), L.BF16, C.byref(d), L.ptr(ws), C.c_size_t(ws.numel()), s), "uvx_gemm_splitk")
    else:
        L.check(L.lib().uvx_gemm(L.stream_ptr(), L.BF16, C.byref(d)), "uvx_gemm")


def _held(p, what, ws=None, records=False):
    """Two calls from the same initial buffers: bit-identical; the first one against the reference (and the exact chain).  -> records of the first"""
    outs = p.outputs()
    first = {k: v.clone() for k, v in p.buf.items()}
    if records:
        _lib().lib().uvx_prof_begin()
    try:
        _launch(p, ws)
    finally:
        recs = _records() if records else None
    got = {k: p.buf[k].clone() for k in outs}
    for k in outs:
        p.buf[k].copy_(first[k])
    _launch(p, ws)
    for k in outs:
        assert torch.equal(U.output_bits(p.buf[k]), U.output_bits(got[k])), f"{what}: the second call's {k} differs"
        p.buf[k].copy_(first[k])
    for k, v in p.buf.items():                       # inputs, their padding and canaries included, are read only
        assert k in outs or torch.equal(U.output_bits(v), U.output_bits(first[k])), f"{what}: the call wrote into {k}"
    exact = U.kernel_images(p, U.operands(p)) if U.biteq_outputs(p) else None
    res = U.compare(p, U.reference(p), got, exact)
    print(f"EDGE {what}: " + "  ".join(f"{U.kind(p, k)} {r['worst']:.3f}" for k, r in res.items()))
    U.assert_ok(p, res, what)
    return recs


def _off_by_8_bytes(p):
    """The same problem with every bf16 operand the kernels may take at 8-byte alignment (C, C2, bias, residual; A and B need 16 bytes for
    the LDS DMA) moved 8 bytes off its 16-byte boundary: the `(uintptr_t)p.C & 15` fallbacks of the epilogues instead of their 16-byte paths."""
    buf = {}
    for k, v in p.buf.items():
        if k in ("C", "C2", "bias", "R") and v.dtype == torch.bfloat16:
            moved = torch.empty(v.numel() + 8, dtype=v.dtype, device=v.device)[4:4 + v.numel()]
            assert moved.data_ptr() % 16 == 8
            buf[k] = moved.copy_(v)
        else:
            buf[k] = v
    return U.Problem(p.c, p.family, p.g, buf)


def _forced(c):
    class Forced:
        def __enter__(self_):
            _lib().lib().uvx_gemm_force_variant(-1 if c["variant"] is None else c["variant"])

        def __exit__(self_, *exc):
            _lib().lib().uvx_gemm_force_variant(-1)
    return Forced()


def _group(name):
    return [c for c in CASES if c["group"] == name]


def _plain_group(c):
    with _forced(c):
        for form in c["forms"]:
            cf = with_form(c, form)
            for fam in families(cf, form):
                p = make_problem(cf, fam, DEV)
                what = f"{case_id(c)} {form} family {fam}"
                if form == "ep2":
                    for v in c.get("opt2", (2,)):             # the fragment-layout (1) and the staged (2) form of the SwiGLU backward
                        with _lib().option(_lib().Option.SWIGLU_BWD_IN_DGRAD, v):
                            _held(p, f"{what} option 2 = {v}")
                else:
                    _held(p, what)
                if c["group"] in ("ld", "nn"):
                    _held(_off_by_8_bytes(p), what + " operands 8 bytes off")


@pytest.mark.parametrize("c", _group("tiles"), ids=case_id)
def test_every_product_tile_variant_at_its_tile_and_k_edges(c):
    _plain_group(c)


@pytest.mark.parametrize("c", _group("second"), ids=case_id)
def test_epilogues_with_a_second_operand_against_float64(c):
    """act 2 / act 3 on their own builds (0, 32..34) and through launch_variant's reroutes (31, 11, 15..19, 59..62); epilogue 1 / 2 on every
    family of tiles, epilogue 2 in its fragment-layout and its staged form."""
    _plain_group(c)


@pytest.mark.parametrize("c", _group("nn"), ids=case_id)
def test_nn_form_with_padded_ldb(c):
    _plain_group(c)


@pytest.mark.parametrize("c", _group("ld"), ids=case_id)
def test_padded_leading_dimensions(c):
    _plain_group(c)


@pytest.mark.parametrize("c", _group("batched"), ids=case_id)
def test_batched_form_as_the_project_calls_it(c):
    _plain_group(c)


@pytest.mark.parametrize("c", _group("splitk"), ids=case_id)
def test_split_k_slab_ranges_and_reduce_epilogues(c):
    """uvx_gemm_splitk with a forced factor on every tile the dispatcher serves split (pick_split takes a forced eight-phase tile too): the
    record's variant is 300 + tile and its batch the factor; 16 slabs of 5 K-tiles is the documented fallback to one unsplit launch."""
    L = _lib()
    s, nk, v = c["split"], c["K"] // 64, c["variant"]
    with _forced(c):
        for form in c["forms"]:
            cf = with_form(c, form)
            for fam in families(cf, form):
                p = make_problem(cf, fam, DEV)
                ws = torch.empty(int(L.lib().uvx_gemm_splitk_ws_bytes(c["M"], c["N"])), device=DEV, dtype=torch.uint8)
                recs = _held(p, f"{case_id(c)} {form} family {fam}", ws, records=True)
                assert len(recs) == 1, recs
                if nk >= s:
                    assert recs[0][3] == s and recs[0][4] == 300 + v, recs
                else:
                    assert recs[0][3] == 1 and recs[0][4] == v, recs


@pytest.mark.parametrize("form", _group("tail")[0]["forms"])
def test_tail_split_second_launch_offsets(form):
    """260 tiles of 128 x 128 at K = 128: with the threshold moved (option 10) the last 160 columns go to a second launch whose B, bias,
    residual, C and C2 are offset by hand.  The profiler's record proves the path (variant field >= 100); the same problem with the tail
    split switched off is held to the same reference."""
    L = _lib().lib()
    c = with_form(_group("tail")[0], form)
    for fam in families(c, form):
        p = make_problem(c, fam, DEV)
        what = f"{case_id(c)} {form} family {fam}"
        try:
            with _lib().option(_lib().Option.TAIL_SPLIT_PCT, 190):
                L.uvx_gemm_force_variant(-1)
                recs = _held(p, what + " tail split", records=True)
                # 100 + tile 0: 128-column panels, so the cut is at 128 whole panels = column 16384, the n_main of the CPU mutation proof
                assert len(recs) == 1 and recs[0][4] == 100, f"{what}: the tail launch did not happen: {recs}"
                assert c["n_main"] == (256 // -(-c["M"] // 128)) * 128
                L.uvx_gemm_force_variant(-2)
                recs = _held(p, what + " tail split off", records=True)
                assert len(recs) == 1 and recs[0][4] < 100, recs
        finally:
            L.uvx_gemm_force_variant(-1)
