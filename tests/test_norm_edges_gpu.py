"""The bf16 norm kernels (ultravox_amd/csrc/norms.hip: the wave, register-resident, two-pass and block kernels of LayerNorm and RMSNorm and their
backwards; elementwise.hip: qk_norm_rope_k, qk_norm_bwd_k) at their dispatch, row and column edges, element by element against the float64
reference of norm_edge_util.py.  Every case goes through the public ABI: uvx_layernorm, uvx_layernorm_bwd (with and without dx_add), uvx_rmsnorm,
uvx_rmsnorm_bwd (dx, dx + dx_add, dw, dx + dw), uvx_qk_norm_rope (flavors 0 and 1, with and without raw), uvx_qk_norm_bwd (flavors 0 and 1), and the
row norm of either flavor as uvx_gemm_rmsnorm runs it at M = 3 with option 24 left at 0 (read from norm_out; flavor 0 bit-equal to uvx_rmsnorm).
norm_edge_util.served_by - the dispatchers restated - says which instantiation a case runs; test_norm_edges_cpu.py shows that the case list
reaches all of them, that an f32 restatement of each kernel stays within the bars and that every off-by-one breaks them.

Per case, family (R, P with one run per edge vector, Z) and output: every element within its bar of the reference and finite; against the
restatement at most 1 % of the elements differ in their bf16 bits and none by more than one bf16 ulp (two for the RoPE outputs; the f32 dw by its
bar only); every operand sits in a buffer of canaries - the space around, the rows after `rows`, the pad and v columns of the strided per-head
rows, the inputs and the weights come back bit for bit; a second call is bit-identical (dw: three calls); the forced two-pass form (option 18)
of every register case and the flavor-0 norm_out are bit-identical to the default; a rejected shape raises ValueError and writes nothing, zero
rows write nothing; RMSNorm of an all-zero row is exactly 0.  (Flavor 0 rounds twice: where x rstd lies within 2^-20 of a rounding boundary the kernel
and the restatement may round it apart with nothing wrong, and a weight of mantissa m turns that into up to two ulps of the output.  With general
weights everywhere the first run showed exactly this, 23 of 2 M elements of rms-512x4096, R, at up to 2.00 ulp; the inputs - not the cap - were
changed: the weight of such a column is a power of two, norm_edge_util._decide_inner_rounding.)

Not reachable through the ABI and left to the model-level tests (test_model_gpu.py, test_gemma_gpu.py, test_gemma3_gpu.py, test_qwen_gpu.py,
test_prefix_skip_gpu.py): rows_dev, resid, dw_part (the blocked weight gradient and rmsnorm_dw_reduce_k), RowSkip, and flavor 1 of the row backward.

Largest error seen on an MI355X, in bar units per kernel and output, with the case and family (P: its edge vector); beside it the restatement's
figure from test_norm_edges_cpu.py (profiles/norm_edges.txt holds the same table):
  kernel                          output  MI355X  restatement  case, family (P: its edge vector)
  layernorm_fwd_wave_k            y       0.998   0.998        ln-4x512, R
  layernorm_fwd_k                 y       0.998   0.998        ln-5x504, P 62
  layernorm_bwd_k                 dx      0.999   0.999        ln_bwd-5x8, Z
  rmsnorm_fwd_wave_k              y       0.999   0.999        rms-9x512, R
  rmsnorm_fwd_wave_k, flavor 1    y       0.998   0.998        gemma-3x512-f1, Z
  rmsnorm_fwd_reg_k               y       0.998   0.998        rms-5x504, R (restatement: rms-4x1544, R)
  rmsnorm_fwd_reg_k, flavor 1     y       0.997   0.997        gemma-3x576-f1, Z
  rmsnorm_fwd_k                   y       0.998   0.998        rms-513x4096, P 256
  rmsnorm_fwd_k, flavor 1         y       0.994   0.994        gemma-3x8256-f1, P 512
  rmsnorm_bwd_k                   dx      0.998   0.998        rms_bwd-1x8-dx_add, P 0 (restatement: rms_bwd-17x8-dx_add, R)
  rmsnorm_bwd_k                   dw      0.995   0.995        rms_bwd-1x4096-dx_dw, P 255
  qk_norm_rope_k                  qk      0.975   0.975        qk-d64-h5x1-f1-raw, Z
  qk_norm_rope_k                  raw     0       0            a copy, bit for bit
  qk_norm_bwd_k                   dqk     0.999   0.999        qk_bwd-d64-h5x1-f0, P (0, 7)
Every figure equals the restatement's to three digits: the error is the bf16 roundings' (a bar is the SUM of the half ulps on a path, and among
thousands of elements one comes within a part in a thousand of all of them at once); neither the summation order, the fma contraction nor the
hardware rsqrt shows at this scale.  Against the restatement the largest share of elements with other bf16 bits was 7.4e-3 (one element of the
136 of rms_bwd-17x8-dx, P 0), 2e-3 and less on every output of more than a thousand elements, never more than one ulp; every canary, the second
(dw: third) call, the forced two-pass form and the flavor-0 norm_out held bit for bit in all 1814 runs of the 267 tests (10 s).  No kernel had
to be changed.
"""
import ctypes as C

import pytest
import torch

import norm_edge_util as N
from norm_edge_util import FAMILIES, HEAD, case_id, cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAIL = 72                  # canary elements after every operand; an output has two more rows of them in front of that
WORST = {}                 # (kernel, output) -> (bar units, case, family, variant): printed by every test, collected into profiles/norm_edges.txt


def _lib():
    from ultravox_amd import _lib as L
    return L


def _canaries(shape, dtype=torch.bfloat16):
    if dtype == torch.bfloat16:
        return torch.full(shape, N.CANARY16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


class Run:
    """the operands of one launch inside their canary buffers"""

    def __init__(self, c, inp):
        self.c, self.inp, self.buf, self.view, self.outs = c, inp, {}, {}, []
        for k, v in inp.items():
            self.buf[k], self.view[k] = N.guarded(v, TAIL)

    def output(self, name, shape, dtype=torch.bfloat16, zero=False):
        t = torch.zeros(shape, dtype=dtype, device=DEV) if zero else _canaries(shape, dtype)
        self.buf[name], self.view[name] = N.guarded(t, 2 * shape[-1] + TAIL)
        self.outs.append(name)

    def in_place(self, name):
        """an operand that the call rewrites"""
        self.outs.append(name)

    def p(self, name):
        return C.c_void_p(self.view[name].data_ptr()) if name in self.view else C.c_void_p(0)


def _launch(r):
    L, c = _lib(), r.c
    lib, st, e, rows, cols = L.lib(), L.stream_ptr(), c["entry"], c["rows"], c["cols"]
    if e == "rms":
        L.check(lib.uvx_rmsnorm(st, L.BF16, r.p("x"), r.p("w"), r.p("y"), rows, cols, C.c_float(N.RMS_EPS)), "uvx_rmsnorm")
    elif e == "ln":
        L.check(lib.uvx_layernorm(st, L.BF16, r.p("x"), r.p("w"), r.p("b"), r.p("y"), rows, cols, C.c_float(N.LN_EPS)), "uvx_layernorm")
    elif e == "ln_bwd":
        L.check(lib.uvx_layernorm_bwd(st, L.BF16, r.p("dy"), r.p("x"), r.p("w"), r.p("add"), r.p("dx"), rows, cols, C.c_float(N.LN_EPS)), "uvx_layernorm_bwd")
    elif e == "rms_bwd":
        L.check(lib.uvx_rmsnorm_bwd(st, L.BF16, r.p("dy"), r.p("x"), r.p("w"), r.p("add"), r.p("dx"), r.p("dw"), rows, cols, C.c_float(N.RMS_EPS)), "uvx_rmsnorm_bwd")
    elif e == "gemma":
        d = L.GemmDesc()
        d.A, d.B, d.C = r.view["x"].data_ptr(), r.view["B"].data_ptr(), r.view["C"].data_ptr()
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.batch, d.alpha = rows, 8, cols, cols, cols, 8, 1, 1.0
        L.check(lib.uvx_gemm_rmsnorm(st, L.BF16, C.byref(d), r.p("w"), C.c_float(N.RMS_EPS), c["flavor"], r.p("y")), "uvx_gemm_rmsnorm")
    elif e == "qk":
        L.check(lib.uvx_qk_norm_rope(st, L.BF16, r.p("qkv"), r.p("wq"), r.p("wk"), r.p("raw"), r.p("cs"), rows, c["T"], c["Hq"], c["Hkv"], cols, c["ld"],
                                     C.c_float(N.RMS_EPS), c["flavor"]), "uvx_qk_norm_rope")
    else:
        L.check(lib.uvx_qk_norm_bwd(st, L.BF16, r.p("dqkv"), r.p("raw"), r.p("wq"), r.p("wk"), rows, c["Hq"], c["Hkv"], cols, c["ld"], C.c_float(N.RMS_EPS),
                                    c["flavor"]), "uvx_qk_norm_bwd")


def _prepare(c, inp):
    """-> (Run, {reference output name: (buffer name, columns)})"""
    e, rows, cols = c["entry"], c["rows"], c["cols"]
    r = Run(c, inp)
    if e in ("rms", "ln", "gemma"):
        r.output("y", (rows, cols))
        if e == "gemma":
            r.output("C", (rows, 8))
        return r, {"y": ("y", cols)}
    if e == "ln_bwd":
        r.output("dx", (rows, cols))
        return r, {"dx": ("dx", cols)}
    if e == "rms_bwd":
        m = {}
        if c["mode"] != "dw":
            r.output("dx", (rows, cols))
            m["dx"] = ("dx", cols)
        if c["mode"] in ("dw", "dx_dw"):
            r.output("dw", (cols,), torch.float32, zero=True)      # the kernel adds into dw: the caller zeroes it
            m["dw"] = ("dw", cols)
        return r, m
    qk = (c["Hq"] + c["Hkv"]) * cols
    name = "qkv" if e == "qk" else "dqkv"
    r.view[name][:, c["ld"] - 8:] = _canaries((rows, 8))           # the pad of every strided row
    r.in_place(name)
    m = {"qk" if e == "qk" else "dqk": (name, qk)}
    if c.get("raw"):
        r.output("raw", (rows, qk))
        m["raw"] = ("raw", qk)
    return r, m


def _held(c, fam, variant):
    """one run of a case: the launch against reference, restatement and canaries; a second launch (dw: a third) bit for bit; the forced two-pass form"""
    what = f"{case_id(c)} family {fam}{'' if variant is None else ' ' + str(variant)}"
    inp = N.make_inputs(c, fam, variant, DEV)
    r, outs = _prepare(c, inp)
    inp = {k: r.view[k].clone() for k in inp}                      # (the pad canaries of the strided rows included)
    ref, re = N.reference(c, inp), N.restatement(c, inp)
    first = {k: v.clone() for k, v in r.buf.items()}

    def once():
        for k in r.outs:
            r.buf[k].copy_(first[k])
        _launch(r)
        return {k: v.clone() for k, v in r.buf.items()}

    after = once()
    for n in range(2 if "dw" in outs else 1):
        again = once()
        for k in r.outs:
            assert torch.equal(N.bits(again[k]), N.bits(after[k])), f"{what}: call {n + 2} differs in {k}"
    kern = N.served_by(c["entry"], c["rows"], c["cols"], 0, c.get("mode"))
    if kern[0] == "rmsnorm_fwd_reg_k":
        with _lib().option(_lib().Option.RMSNORM_TWO_PASS, 1):
            forced = once()
        assert torch.equal(N.bits(forced["y"]), N.bits(after["y"])), f"{what}: the two-pass kernel differs from the register kernel"
    for k, v in after.items():                                     # read-only operands and every canary
        if k not in r.outs:
            assert torch.equal(N.bits(v), N.bits(first[k])), f"{what}: the call wrote into {k}"
    for k in r.outs:                                               # the space around every output, the rows after `rows` among it
        n_el = r.view[k].numel()
        outside = torch.ones(after[k].numel(), dtype=torch.bool, device=DEV)
        outside[HEAD:HEAD + n_el] = False
        assert torch.equal(N.bits(after[k])[outside], N.bits(first[k])[outside]), f"{what}: canaries around {k} are overwritten"
    line = []
    for name, (bname, ncols) in outs.items():
        n_el = r.view[bname].numel()
        got_full = after[bname][HEAD:HEAD + n_el].view(r.view[bname].shape)
        was_full = first[bname][HEAD:HEAD + n_el].view(r.view[bname].shape)
        got = got_full
        if got_full.dim() == 2 and ncols != got_full.shape[1]:     # in place on the q | k columns: v and the pad stay
            assert torch.equal(N.bits(got_full[:, ncols:]), N.bits(was_full[:, ncols:])), f"{what}: the v columns or the pad of {bname} are overwritten"
            got = got_full[:, :ncols]
        val, noise = ref[name][0], ref[name][2]
        got = got.reshape(val.shape)
        assert torch.isfinite(got).all(), f"{what}: {name} is not finite"
        u = N.bar_units(got, ref[name])
        key = (kern[0] + (" flavor 1" if c.get("flavor") and c["entry"] == "gemma" else ""), name)
        if u > WORST.get(key, (0.0,))[0]:
            WORST[key] = (u, case_id(c), fam, variant)
        line.append(f"{name} {u:.3f}")
        assert u <= 1.0, f"{what}: {name} at {u:.3f} bars"
        if name != "dw":
            share, ulps = N.flips(got, re[name], noise, ref[name][3] if len(ref[name]) > 3 else None)
            line.append(f"(flips {share:.1e}, {ulps:.2f} ulp)")
            assert share <= 0.01 and ulps <= (2.0 if name == "qk" else 1.0), f"{what}: {name} against the restatement: {share:.2e} of the elements differ, by up to {ulps:.2f} ulp"
    if fam == "Z" and c["entry"] in ("rms", "gemma"):
        assert not N.bits(after["y"][HEAD:][:c["rows"] * c["cols"]].view(c["rows"], -1)[-1]).to(torch.int32).bitwise_and(0x7FFF).any(), f"{what}: the all-zero row is not 0"
    print(f"NORM-EDGE {what} [{' '.join(str(x) for x in kern)}]: " + " ".join(line))
    return r, after


def _run(c, extra=None):
    for fam in FAMILIES:
        for v in N.variants(c, fam):
            r, after = _held(c, fam, v)
            if extra:
                extra(r, after)
    for (kern, out), (u, cid, fam, v) in sorted(WORST.items()):
        print(f"NORM-EDGE-WORST {kern} {out} {u:.3f} {cid}, {fam} {'' if v is None else v}")


@pytest.mark.parametrize("c", cases("rms"), ids=case_id)
def test_rmsnorm_forward_at_its_wave_register_and_two_pass_edges(c):
    """uvx_rmsnorm: rmsnorm_fwd_wave_k<1, 2, 4> with a partial last block of four rows, rmsnorm_fwd_reg_k<bf16, 1, 2, 4> from one active lane to every sweep
    exactly full and one vector into the next, rmsnorm_fwd_k past 8192 columns and past 512 rows; every register case again as the two-pass kernel."""
    _run(c)


@pytest.mark.parametrize("c", cases("rms_bwd"), ids=case_id)
def test_rmsnorm_backward_in_every_mode_at_its_vector_count_edges(c):
    """uvx_rmsnorm_bwd: rmsnorm_bwd_k<.., MV = 1, 2, 6> on both sides of 2048 and 4096 columns and at the 12288 limit; the register-cached path (dx,
    dx + dx_add) and the reloading one with the single-block weight gradient (dw, dx + dw), whose sum is the same bits in three calls."""
    _run(c)


@pytest.mark.parametrize("c", cases("ln"), ids=case_id)
def test_layernorm_forward_wave_and_block_kernels(c):
    """uvx_layernorm: layernorm_fwd_wave_k<1, 2, 4, 8> with one to nine rows (four per block), layernorm_fwd_k with 64 to 256 threads."""
    _run(c)


@pytest.mark.parametrize("c", cases("ln_bwd"), ids=case_id)
def test_layernorm_backward_with_and_without_dx_add(c):
    _run(c)


def _flavor0_is_uvx_rmsnorm(r, after):
    if r.c["flavor"] == 0:
        L = _lib()
        y = torch.empty_like(r.view["x"])
        L.check(L.lib().uvx_rmsnorm(L.stream_ptr(), L.BF16, r.p("x"), r.p("w"), L.ptr(y), r.c["rows"], r.c["cols"], C.c_float(N.RMS_EPS)), "uvx_rmsnorm")
        assert torch.equal(N.bits(y).reshape(-1), N.bits(after["y"][HEAD:HEAD + y.numel()])), f"{case_id(r.c)}: norm_out differs from uvx_rmsnorm"
    assert torch.isfinite(after["C"][HEAD:HEAD + 3 * 8]).all()


@pytest.mark.parametrize("c", cases("gemma"), ids=case_id)
def test_row_norm_of_either_flavor_inside_uvx_gemm_rmsnorm(c):
    """uvx_gemm_rmsnorm at M = 3, N = 8 (option 24 = 0: rmsnorm_fwd(flavor) into norm_out, then the GEMM): one K for each forward form; the Gemma flavor
    against the reference, flavor 0 bit-equal to uvx_rmsnorm as well."""
    _run(c, _flavor0_is_uvx_rmsnorm)


@pytest.mark.parametrize("c", cases("qk"), ids=case_id)
def test_per_head_norm_and_rope_on_strided_rows(c):
    """uvx_qk_norm_rope: D / 16 lanes per head (4, 8, 16), q and k heads with their own weights, positions row % T wrapping twice over a table of exactly
    T rows, rows strided by ld with v columns and a pad behind them, a partial last block."""
    _run(c)


@pytest.mark.parametrize("c", cases("qk_bwd"), ids=case_id)
def test_per_head_norm_backward_on_strided_rows(c):
    _run(c)


def _reject(c, inp, untouched, **change):
    r, _ = _prepare(c, inp)
    r.c = dict(c, **change)
    first = {k: v.clone() for k, v in r.buf.items()}
    if untouched == "raises":
        with pytest.raises(ValueError):
            _launch(r)
    else:
        _launch(r)
    torch.cuda.synchronize()
    for k, v in r.buf.items():
        assert torch.equal(N.bits(v), N.bits(first[k])), f"{case_id(r.c)}: a rejected or empty call wrote into {k}"


def test_rejected_shapes_raise_and_zero_rows_write_nothing():
    """cols % 8 != 0 in every row-norm entry point, 12296 columns in the RMSNorm backward, head_dim 96, ld % 8 != 0: ValueError, every buffer intact;
    rows == 0: a no-op.  (The buffers are those of a valid 2-row problem of 16 columns, larger than anything the rejected shape names.)"""
    row = [dict(entry="rms", rows=2, cols=16), dict(entry="ln", rows=2, cols=16), dict(entry="ln_bwd", rows=2, cols=16, add=True)]
    row += [dict(entry="rms_bwd", rows=2, cols=16, mode=m) for m in N.RMS_BWD_MODES]
    for c in row:
        c["seed"] = 5
        inp = N.make_inputs(c, "R", None, DEV)
        assert N.served_by(c["entry"], 1, N.REJECTED_COLS, 0, c.get("mode")) == "rejected"
        _reject(c, inp, "raises", rows=1, cols=N.REJECTED_COLS)
        _reject(c, inp, "noop", rows=0)
    big = dict(entry="rms_bwd", rows=1, cols=N.MAX_BWD_COLS + 8, seed=6)
    for m in N.RMS_BWD_MODES:
        c = dict(big, mode=m)
        assert N.served_by("rms_bwd", 1, c["cols"], 0, m) == "rejected"
        _reject(c, N.make_inputs(c, "R", None, DEV), "raises")
    for e in ("qk", "qk_bwd"):
        c = dict(entry=e, rows=15, cols=128, Hq=3, Hkv=2, T=5, ld=7 * 128 + 8, flavor=0, raw=True, seed=7)
        inp = N.make_inputs(c, "R", None, DEV)
        _reject(c, inp, "raises", cols=96)                         # (3 + 2) heads of 96 fit inside the rows of 128-wide heads
        _reject(c, inp, "raises", ld=c["ld"] - 4)
        _reject(c, inp, "noop", rows=0)
