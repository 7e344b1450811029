"""The wav2vec2 stem on the GPU (ultravox_amd/csrc/wav2vec2.hip: w2v_im2col0_k, w2v_gn_partial_k / w2v_gn_final_k / w2v_gn_gelu_k, the conv layers as GEMMs
on the strided view, w2v_pos_pack_k, the per-clip batched GEMM over the groups, w2v_pos_finish_k; frames() and carve() around them) through
uvx_wav2vec2_fwd at ZERO encoder layers, frame by frame against the float64 reference of w2v_stem_util.py, in f32 parity mode and in bf16.
test_w2v_stem_cpu.py shows that the two CPU stand-ins stay inside the bars and that each of the 34 moved boundaries breaks them by a factor of 2 at least.

The call goes through _lib itself: operands from pack_wav2vec2, W2vConfig and W2vWeights filled here, a one-element EncLayer array (the entry refuses a
null pointer even at zero layers), workspace and output owned by the test.

Per case, family (R, E) and form of input_values (f32 into either tower, bf16 into a bf16 tower; both must give the same bits, the bf16 tower rounding
f32 samples as torch does): every frame within the bar and finite, with a line for the worst frame and where it is; input_values sit between NaN
canaries and come back bit for bit; the rows behind the B Tn d output elements keep their canaries; the workspace is filled with 0xFF bytes before the
call (w2v_pos_pack_k must write its own padding) and the result with a zeroed workspace, and of a second call, is bit-identical; at B = 3 other
samples in clip 1 leave the outputs of clips 0 and 2 bit-identical.  uvx_wav2vec2_frames equals the conv-stack formula from L = 380 to 1100 (-1 below
400); L = 399 raises the shape error that names the receptive field and a workspace one byte short of uvx_wav2vec2_ws_bytes the workspace error,
both with nothing written.

Measured on an MI355X (profiles/w2v_stem_edges.txt holds the same figures), largest per-frame distance in bar units per precision:
  f32    0.292 bars  (1.366e-06 against 4.673e-06)  std-L400-B3, R, clip 0 frame 0
  bf16   0.553 bars  (1.773e-02 against 3.206e-02)  std-L5200-B3, R, clip 0 frame 6      (most bf16 cases sit at 0.48 .. 0.52: torch's own distance)
The group-norm family with a conv bias of 10 .. 30 spreads (gnbias-L9000-B3, T0 = 1799, f32) decided the suspicion about w2v_gn_final_k:
  E[x^2] - mean^2 over f32 chunk sums   R 3.19 bars (4.251e-05 against 1.333e-05)   E 4.21 bars (8.345e-05 against 1.983e-05)
      relative error of rstd on the biased channels, read out of the workspace: R 5.7e-05, E 1.2e-04 (a CPU emulation of that order: 5.7e-05, 1.1e-04)
  per-chunk mean and squared deviations R 0.128 bars (1.700e-06)                    E 0.101 bars (1.996e-06); rstd: R 7.2e-08, E 1.9e-07
so w2v_gn_partial_k now walks its chunk twice (a rough mean, then the deviations from it) and w2v_gn_final_k merges (count, mean, M2) in double.  Sums
of deviations from the chunk's FIRST row - the cheaper form - fail on family E, whose first frames are spikes (CPU emulation: rstd off by 2.6e-04 on
channels without any offset).  With the old statistics every other case held: f32 at most 0.310 bars (std-L5520-B3, R), bf16 0.546 (std-L5200-B3, R).
The second defect these tests met: the workspace check compared against the carved bytes, 256 fewer than uvx_wav2vec2_ws_bytes reports, so a
workspace one byte short was accepted; the entry points now ask for what the size function reports.  All 88 tests: 3.4 s.
"""
import ctypes as C

import pytest
import torch

import w2v_stem_util as U
from w2v_stem_util import FAMILIES, case_id

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEAD = 64                  # canary elements in front of input_values and of the output
TAIL_ROWS = 2              # canary rows of d elements behind the output
D = 128
WORST = {}                 # precision -> (bar units, distance, bar, case, family, clip, frame): printed by every test, collected into profiles/w2v_stem_edges.txt
_TOWERS = {}


def _lib():
    from ultravox_amd import _lib as L
    return L


class Tower:
    """the packed operands of one configuration and family on the device, with the structs that point at them"""

    def __init__(self, c, fam, precision):
        from ultravox_amd.weights import pack_wav2vec2
        L = _lib()
        self.cfg, dt = U.config(c), U.tdtype(precision)
        a = self.cfg.audio_config
        self.e = e = pack_wav2vec2(U.state_dict(c, fam, precision), self.cfg, dt, DEV)
        wc = L.W2vConfig()
        wc.dtype, wc.n_conv, wc.conv_dim = L.dtype_code(dt), len(a.conv_kernel), a.conv_dim[0]
        for i, (k, s) in enumerate(zip(a.conv_kernel, a.conv_stride)):
            wc.conv_kernel[i], wc.conv_stride[i] = k, s
        wc.d, wc.heads, wc.ffn, wc.layers = a.d_model, a.encoder_attention_heads, a.encoder_ffn_dim, 0
        wc.pos_k, wc.pos_groups, wc.ln_eps = a.num_conv_pos_embeddings, a.num_conv_pos_embedding_groups, a.layer_norm_eps
        wc.feat_norm_layer, wc.conv_bias, wc.stable_ln = int(a.feat_extract_norm == "layer"), int(a.conv_bias), int(a.do_stable_layer_norm)
        ww = L.W2vWeights()
        for n in ("conv0_w", "gn_w", "gn_b", "fp_ln_w", "fp_ln_b", "fp_w", "fp_b", "pos_w", "pos_b", "ln_w", "ln_b"):
            setattr(ww, n, 0 if e[n] is None else e[n].data_ptr())
        for name in ("conv_w", "conv_b", "conv_ln_w", "conv_ln_b"):
            for i, t in enumerate(e[name]):
                getattr(ww, name)[i] = 0 if t is None else t.data_ptr()
        self.layers = (L.EncLayer * 1)()              # zero layers: never read, but the entry refuses a null array
        ww.layers = self.layers
        self.wc, self.ww, self.dtype = wc, ww, dt

    def frames(self, n):
        return _lib().lib().uvx_wav2vec2_frames(C.byref(self.wc), n)

    def ws_bytes(self, B, n):
        return _lib().lib().uvx_wav2vec2_ws_bytes(C.byref(self.wc), B, n)

    def forward(self, x, out, ws, ws_bytes=None, B=None, n=None):
        """x [B, L] f32 or bf16 on the device, out: the first element of the output, ws: a byte tensor"""
        L = _lib()
        B, n = (x.shape[0] if B is None else B), (x.shape[1] if n is None else n)
        L.check(L.lib().uvx_wav2vec2_fwd(L.stream_ptr(), C.byref(self.wc), C.byref(self.ww), L.ptr(x), int(x.dtype == torch.float32), B, n, L.ptr(out),
                                         L.ptr(ws), C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes)), "uvx_wav2vec2_fwd")


def _tower(c, fam, precision):
    key = (c["kernel"], c["pos_k"], c["groups"], c["norm"], c["bias"], c["stable"], c["name"] == "gnbias", fam, precision)
    if key not in _TOWERS:
        _TOWERS[key] = Tower(c, fam, precision)
    return _TOWERS[key]


def _nan_canaries(n, dtype):
    if dtype == torch.bfloat16:
        return torch.full((n,), 0x7F91, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return torch.full((n,), float("nan"), dtype=dtype, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded_input(x):
    """x [B, L] on the host -> (the flat buffer: HEAD NaNs, the samples, HEAD NaNs; the [B, L] view of the samples)"""
    buf = _nan_canaries(2 * HEAD + x.numel(), x.dtype)
    view = buf[HEAD:HEAD + x.numel()].view(x.shape)
    view.copy_(x)
    return buf, view


def _call(tower, c, x, poison=0xFF, ws=None):
    """one forward inside canaries -> (the [B, Tn, d] result, a clone; the workspace)"""
    B, Tn, n_out = c["B"], c["T"][-1], c["B"] * c["T"][-1] * D
    xbuf, xv = _guarded_input(x)
    before = xbuf.clone()
    obuf = _nan_canaries(HEAD + n_out + TAIL_ROWS * D, tower.dtype)
    guard = _bits(obuf).clone()
    if ws is None:
        ws = torch.full((tower.ws_bytes(B, c["L"]),), poison, dtype=torch.uint8, device=DEV)
    tower.forward(xv, obuf[HEAD:], ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(xbuf), _bits(before)), "input_values or their canaries were written"
    after = _bits(obuf)
    assert torch.equal(after[:HEAD], guard[:HEAD]) and torch.equal(after[HEAD + n_out:], guard[HEAD + n_out:]), "the canaries around the output were written"
    return obuf[HEAD:HEAD + n_out].view(B, Tn, D).clone(), ws


def _held(c, fam, precision):
    what = f"{case_id(c)} family {fam} {precision}"
    cfg, sd, x, want, stand, bar = U.prepared(c, fam, precision)
    tower = _tower(c, fam, precision)
    assert tower.frames(c["L"]) == c["T"][-1], what
    first = None
    for form in U.input_forms(precision):
        got, ws = _call(tower, c, U.wave_in(c, fam, form))
        assert torch.isfinite(got).all(), f"{what}: not finite with {form} input_values"
        if first is None:
            first = got
            dist = U.frame_dist(got.cpu(), want)
            w, b, t = U.worst(dist)
            print(f"W2V-STEM {what}: worst frame {w:.3e} = {w / bar:.3f} bars (bar {bar:.3e}, stand-in {stand.max().item():.3e}) at clip {b} frame {t} of {c['T'][-1]}")
            if w / bar > WORST.get(precision, (0.0,))[0] and c["name"] != "gnbias":
                WORST[precision] = (w / bar, w, bar, case_id(c), fam, b, t)
            if c["name"] == "gnbias":
                WORST["gnbias " + fam] = (w / bar, w, bar, case_id(c), fam, b, t)
            assert w <= bar, f"{what}: clip {b} frame {t} at {w:.3e}, {w / bar:.2f} bars"
            again, _ = _call(tower, c, U.wave_in(c, fam, form), ws=ws)                   # the workspace as the first call left it
            assert torch.equal(_bits(again), _bits(got)), f"{what}: a second call differs"
            zeroed, _ = _call(tower, c, U.wave_in(c, fam, form), poison=0)
            assert torch.equal(_bits(zeroed), _bits(got)), f"{what}: the result depends on what the workspace held"
        else:
            assert torch.equal(_bits(got), _bits(first)), f"{what}: bf16 input_values and f32 input_values give other bits"
    if c["B"] == 3:
        other = U.wave_in(c, fam, torch.float32, alt=True)
        assert torch.equal(other[0], U.wave_in(c, fam, torch.float32)[0]) and not torch.equal(other[1], U.wave_in(c, fam, torch.float32)[1])
        leak, _ = _call(tower, c, other)
        assert torch.isfinite(leak).all(), what
        assert not torch.equal(_bits(leak[1]), _bits(first[1])), f"{what}: clip 1 did not change with its samples"
        for b in (0, 2):
            assert torch.equal(_bits(leak[b]), _bits(first[b])), f"{what}: clip {b} changed with clip 1's samples"


def _run(c, precision):
    for fam in FAMILIES:
        _held(c, fam, precision)
    for k, (u, w, bar, cid, fam, b, t) in sorted(WORST.items()):
        print(f"W2V-STEM-WORST {k}: {u:.3f} bars ({w:.3e} against {bar:.3e}) {cid}, {fam}, clip {b} frame {t}")


@pytest.mark.parametrize("c", U.cases("f32"), ids=case_id)
def test_stem_in_f32_parity_mode_frame_by_frame(c):
    """f32 mode: 8 x torch's f32 distance to float64 per frame - the place for the index arithmetic of this file's kernels; the group-norm family with
    a conv bias of 10 .. 30 spreads decides whether w2v_gn_final_k's E[x^2] - mean^2 holds"""
    _run(c, "f32")


@pytest.mark.parametrize("c", U.cases("bf16"), ids=case_id)
def test_stem_in_bf16_frame_by_frame_with_either_input_form(c):
    """bf16: 2 x torch's module-by-module bf16 distance per frame - what only the bf16 dispatch does: the few-row kernels on the strided, overlapping
    rows of a short single clip (lda != K, act = 1), the tiled conv layout with a batch"""
    _run(c, "bf16")


def test_frame_count_from_380_to_1100():
    tower = _tower(U.CASES[0], "R", "f32")
    for n in range(380, 1101):
        assert tower.frames(n) == (-1 if n < 400 else (n - 400) // 320 + 1), n
        assert (tower.ws_bytes(1, n) > 256) == (n >= 400), n


@pytest.mark.parametrize("precision", U.PRECISIONS)
def test_error_paths_return_before_anything_is_launched(precision):
    """L = 399: the shape error naming the receptive field; a workspace one byte short of uvx_wav2vec2_ws_bytes: the workspace error - the output and the
    workspace keep every byte"""
    c = next(c for c in U.CASES if c["name"] == "std" and c["L"] == 720 and c["B"] == 3)
    tower = _tower(c, "R", precision)
    x = U.wave_in(c, "R", torch.float32).to(DEV)
    need = tower.ws_bytes(3, 720)
    out = _nan_canaries(3 * 2 * D + TAIL_ROWS * D, tower.dtype)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    guard = _bits(out).clone()
    with pytest.raises(ValueError, match="receptive field"):
        tower.forward(x, out, ws, B=3, n=399)              # (the buffers are those of the valid 720-sample problem)
    with pytest.raises(_lib().UvxError, match="workspace") as err:
        tower.forward(x, out, ws, ws_bytes=need - 1)
    assert not isinstance(err.value, ValueError)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), guard) and bool((ws == 0xA5).all())
    tower.forward(x, out, ws)                               # the same buffers at their full size: accepted
    torch.cuda.synchronize()
    assert torch.isfinite(out[:3 * 2 * D]).all()
