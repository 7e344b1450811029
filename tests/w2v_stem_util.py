"""The wav2vec2 stem (ultravox_amd/csrc/wav2vec2.hip below the encoder layers: w2v_im2col0_k, the GroupNorm over time, the six conv layers as GEMMs on
a strided view, the feature projection, w2v_pos_pack_k / the per-clip batched GEMM / w2v_pos_finish_k) frame by frame against float64 at its length
edges: the case list, the input families, the float64 reference, the two CPU stand-ins for a correct kernel, the mutants and the per-frame metric.
test_w2v_stem_cpu.py proves the harness on the stand-ins and the mutants; test_w2v_stem_gpu.py holds uvx_wav2vec2_fwd to it.

Every case has ZERO encoder layers: uvx_wav2vec2_fwd then returns encoder.layer_norm(h + gelu(pos_conv(h))) in both layer forms, h the feature
projection's output - the stem alone, one LayerNorm behind it.  conv_dim 64, d 128, at most 3 clips of 9000 samples.

Reference: oracle.reference_cpu.wav2vec2_encoder_ref in float64 on exactly the values the device sees - weights and inputs rounded to the tower's dtype
first, then widened (the weight-norm fold of the positional conv in the tower's dtype, as pack_wav2vec2 folds it).  `stem64` restates the same
arithmetic with every boundary as a parameter; unmutated it equals the oracle to 1e-11 (test_w2v_stem_cpu.py), and each mutant is stem64 with exactly
one boundary moved.

Metric: per clip and frame, ||got - want||_2 / ||want||_2 over the d columns.

Bars: per case, family and precision, a margin times the largest per-frame distance of the matching CPU stand-in to float64 - f32: 8 x torch's f32
evaluation of the oracle (gemm_f32.hip and the GroupNorm pass sum in other orders than torch); bf16: 2 x torch's module-by-module bf16 evaluation
(same rounding points; the accumulation order and gelu_fast differ).  Neither is measured against a kernel.  CEILING holds what the bars may be at
most: a property of the inputs, asserted on the CPU.

Families: R - normalised noise, random_state_dict's weights; E - noise of 2^-6 under spikes in the first and the last k0 samples of every clip (the
last samples of clip b and the first of clip b + 1 are neighbours in memory) and in the sample under the last tap of the last frame, placed before the
normalisation; the weights of E have a large last tap in every conv layer, large first and last taps in the positional conv, and positional weights
and biases that differ strongly from group to group."""
import functools

import torch
import torch.nn.functional as F

F64 = torch.float64
P = "audio_tower."
STD_KERNEL, STD_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
GN_ROWS = 512                                  # wav2vec2.hip: time rows per GroupNorm partial block
FAMILIES = ("R", "E")
PRECISIONS = ("f32", "bf16")
MARGIN = {"f32": 8.0, "bf16": 2.0}
# what a bar may be at most (stand-in distances measured on the CPU: f32 at most 1.4e-6 per frame, bf16 at most 2.0e-2): far below every mutant.
# The conv-bias case may have four times that: under offsets of 10 .. 30 spreads torch's own f32 evaluation is up to 2.5e-6 from float64
CEILING = {"f32": 2e-5, "bf16": 5e-2}
TEXT_SMALL = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=64, eos_token_id=2)


def frames_of(L, kernel=STD_KERNEL, stride=STD_STRIDE, ceil=False):
    """the conv-stack formula: frames after every layer, or None where a layer's input is shorter than its kernel"""
    T, n = [], int(L)
    for k, s in zip(kernel, stride):
        if n < k:
            return None
        n = (-(-(n - k) // s) if ceil else (n - k) // s) + 1
        T.append(n)
    return T


def _length_for(Tn, kernel, stride, slack):
    """the shortest L that gives Tn frames, plus `slack` samples (still Tn frames)"""
    L = next(L for L in range(1, 100000) if (frames_of(L, kernel, stride) or [0])[-1] == Tn)
    assert frames_of(L + slack, kernel, stride)[-1] == Tn
    return L + slack


# ------------------------------------------------------------------ cases
def _cases():
    out = []
    std = dict(kernel=STD_KERNEL, stride=STD_STRIDE, pos_k=16, groups=4, norm="group", bias=False, stable=False, precisions=PRECISIONS)
    for L in (400, 719, 720, 2569, 2570, 2640, 2960, 5129, 5130, 5200, 5520, 9000):
        out += [dict(std, name="std", L=L, B=B) for B in (1, 3)]
    two = dict(std, kernel=(10, 3), stride=(5, 2), groups=2)
    for pos_k in (15, 16):
        for Tn, slack in ((1, 7), (7, 0), (8, 3), (128, 7), (129, 0)):
            L = _length_for(Tn, two["kernel"], two["stride"], slack)
            out += [dict(two, name="two", L=L, B=B, pos_k=pos_k) for B in ((1, 3) if Tn <= 8 else (3,))]
    out += [dict(std, name="layer", L=L, B=3, norm="layer", bias=True, stable=True) for L in (720, 5520)]
    out.append(dict(std, name="gnbias", L=9000, B=3, bias=True, stable=True, precisions=("f32",)))
    for i, c in enumerate(out):
        c["T"] = frames_of(c["L"], c["kernel"], c["stride"])
        c["seed"] = 131 * i + c["L"]
    return out


def case_id(c):
    return f"{c['name']}-L{c['L']}-B{c['B']}" + (f"-k{c['pos_k']}" if c["name"] == "two" else "")


CASES = _cases()


def cases(precision):
    return [c for c in CASES if precision in c["precisions"]]


def tdtype(precision):
    return torch.float32 if precision == "f32" else torch.bfloat16


@functools.lru_cache(maxsize=None)
def _config(kernel, stride, pos_k, groups, norm, bias, stable):
    from ultravox_amd.config import UltravoxConfig
    audio = {"model_type": "wav2vec2", "hidden_size": 128, "num_hidden_layers": 0, "num_attention_heads": 2, "intermediate_size": 256,
             "conv_dim": [64] * len(kernel), "conv_kernel": list(kernel), "conv_stride": list(stride), "num_conv_pos_embeddings": pos_k,
             "num_conv_pos_embedding_groups": groups, "feat_extract_norm": norm, "conv_bias": bias, "do_stable_layer_norm": stable}
    return UltravoxConfig(audio_config=audio, text_config=TEXT_SMALL, hidden_size=256, projector_ln_mid=True)


def config(c):
    return _config(c["kernel"], c["stride"], c["pos_k"], c["groups"], c["norm"], c["bias"], c["stable"])


# ------------------------------------------------------------------ inputs
def _normalize(pcm):
    return (pcm - pcm.mean(-1, keepdim=True)) / torch.sqrt(pcm.var(-1, unbiased=False, keepdim=True) + 1e-7)


def _spike_positions(c):
    """the first and the last k0 samples of a clip and the sample under the last tap of the last frame"""
    L, k0 = c["L"], c["kernel"][0]
    rf, hop = 1, 1
    for k, s in zip(c["kernel"], c["stride"]):
        rf, hop = rf + (k - 1) * hop, hop * s
    last_tap = hop * (c["T"][-1] - 1) + rf - 1
    assert last_tap < L
    return sorted({*range(min(k0, L)), *range(L - k0, L), last_tap})


def make_wave(c, family, alt=False):
    """[B, L] float64 zero-mean, unit-variance clips; alt: other values in clip 1 (the leak check), clips 0 and 2 unchanged"""
    g = torch.Generator().manual_seed(c["seed"] * 7 + FAMILIES.index(family))
    B, L = c["B"], c["L"]
    if family == "R":
        x = 0.1 * torch.randn(B, L, generator=g, dtype=F64) + 0.01
    else:
        x = 2.0 ** -6 * torch.randn(B, L, generator=g, dtype=F64)
        pos = _spike_positions(c)
        amp = 0.25 + 0.75 * torch.rand(B, len(pos), generator=g, dtype=F64)
        sign = 1.0 - 2.0 * torch.randint(0, 2, (B, len(pos)), generator=g).to(F64)
        # (clip b's spikes are (1 + b) / 2 times clip 0's: the clips' noise-to-spike ratios, and with them their GroupNorm statistics, differ)
        x[:, pos] = amp * sign * (0.5 + 0.5 * torch.arange(B, dtype=F64)[:, None])
    if alt:
        g2 = torch.Generator().manual_seed(c["seed"] * 7 + 5)
        x[1] = 0.3 * torch.randn(L, generator=g2, dtype=F64) - 0.02
    return _normalize(x)


@functools.lru_cache(maxsize=None)
def _weights(cfg_key, seed, family, bias_case):
    """the audio tower's float32 state dict of a case"""
    from ultravox_amd.weights import random_state_dict
    cfg = _config(*cfg_key)
    a = cfg.audio_config
    sd = {k: v for k, v in random_state_dict(cfg, seed=seed).items() if k.startswith(P)}
    g = torch.Generator().manual_seed(seed + 17)
    if family == "E":
        for i in range(len(a.conv_kernel)):
            sd[P + f"feature_extractor.conv_layers.{i}.conv.weight"][:, :, -1] *= 2.0
        C0, C1 = P + "encoder.pos_conv_embed.conv.parametrizations.weight.original0", P + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
        G, d = a.num_conv_pos_embedding_groups, a.d_model
        scale = (0.5 + 1.5 * torch.arange(G) / max(G - 1, 1)).repeat_interleave(d // G)      # group g's rows: 0.5 .. 2 times the drawn ones
        sd[C1] = sd[C1] * scale[:, None, None]
        gain = sd[C1].float().norm(dim=(0, 1), keepdim=True) * 1.1
        gain[..., 0] *= 3.0
        gain[..., -1] *= 3.0
        sd[C0] = gain
        sd[P + "encoder.pos_conv_embed.conv.bias"] = (0.2 * torch.randn(d, generator=g) + 0.5 * (torch.arange(d) // (d // G)).float() - 0.5)
    if bias_case is not None:
        # conv 0's bias: on every fourth channel an offset of 10 .. 30 times the channel's spread over time, the spread taken from the case's own
        # clips (the largest of the clips' spreads, so that 10.5 .. 12.5 is the SMALLEST ratio among them; family E's quieter clips reach 30;
        # test_w2v_stem_cpu.py measures the ratio per clip)
        w0, b0 = sd[P + "feature_extractor.conv_layers.0.conv.weight"], sd[P + "feature_extractor.conv_layers.0.conv.bias"]
        c = CASES[bias_case]
        spread = F.conv1d(make_wave(c, family).float()[:, None], w0, None, stride=c["stride"][0]).std(-1).amax(0)
        ratio = torch.linspace(10.5, 12.5, b0.shape[0] // 4)
        b0[::4] = ratio * spread[::4] * (1.0 - 2.0 * (torch.arange(ratio.numel()) % 2))
    return sd


def state_dict(c, family, precision):
    """the tower's weights as the device sees them: tensors of the tower's dtype"""
    key = (c["kernel"], c["stride"], c["pos_k"], c["groups"], c["norm"], c["bias"], c["stable"])
    sd = _weights(key, 100 + len(c["kernel"]) + c["pos_k"], family, CASES.index(c) if c["name"] == "gnbias" else None)
    return {k: v.to(tdtype(precision)) for k, v in sd.items()}


def wave(c, family, precision, alt=False):
    """input_values as the device sees them: rounded to the tower's dtype (f32 input_values into a bf16 tower are rounded by w2v_im2col0_k), in f32"""
    return make_wave(c, family, alt).float().to(tdtype(precision)).float()      # (through f32 first, as wave_in's bf16 form: one rounding sequence)


def input_forms(precision):
    """the dtypes input_values come in: f32 into either tower (unrounded: a bf16 tower rounds them itself), bf16 into a bf16 tower"""
    return (torch.float32,) if precision == "f32" else (torch.float32, torch.bfloat16)


def wave_in(c, family, form, alt=False):
    return make_wave(c, family, alt).float().to(form)


# ------------------------------------------------------------------ the float64 reference, with its boundaries as parameters
MUTANTS = ("conv0_from_1", "clip_stride_plus", "clip_stride_minus", "conv0_taps", "gn_rows_minus_1", "gn_whole_chunks", "gn_prev_clip",
           *(f"conv{i}_{m}" for i in range(1, 7) for m in ("from_1", "taps", "clip_stride")),
           "frames_ceil", "pos_pad_plus", "pos_pad_minus", "pos_taps", "pos_drop_first", "pos_next_group_channels", "pos_group0_weights",
           "pos_bias_wrong_group", "no_residual")


def touches(mut, c):
    """whether the mutant has a meaning on the case"""
    n = len(c["kernel"])
    if mut.startswith("conv") and mut[4] != "0":
        i = int(mut[4])
        return i < n and (c["B"] > 1 or not mut.endswith("clip_stride"))
    if mut in ("clip_stride_plus", "clip_stride_minus", "gn_prev_clip"):
        return c["B"] > 1 and (c["norm"] == "group" or not mut.startswith("gn"))
    if mut in ("gn_rows_minus_1", "gn_whole_chunks"):
        return c["norm"] == "group" and (mut == "gn_rows_minus_1" or (c["T"][0] > GN_ROWS and c["T"][0] % GN_ROWS != 0))
    if mut == "frames_ceil":
        return frames_of(c["L"], c["kernel"], c["stride"], ceil=True) != c["T"]
    if mut == "pos_drop_first":
        return c["pos_k"] % 2 == 0
    return True


def _conv_rows(flat, w, bias, B, T_out, clip_stride, step, first, taps):
    """flat [rows, Cin] (rows of all clips, back to back), w [Cout, Cin, k]: out[b, t] = bias + sum over j < taps of w[:, :, j] . flat[b clip_stride +
    step t + first + j]; rows past the end read as zero"""
    need = (B - 1) * clip_stride + step * (T_out - 1) + first + taps
    if need > flat.shape[0]:
        flat = torch.cat((flat, flat.new_zeros(need - flat.shape[0], flat.shape[1])))
    idx = (torch.arange(B)[:, None, None] * clip_stride + step * torch.arange(T_out)[None, :, None] + first + torch.arange(taps)[None, None, :])
    out = torch.einsum("btjc,ocj->bto", flat[idx], w[:, :, :taps])
    return out if bias is None else out + bias


def stem64(sd, cfg, x, mut=None):
    """wav2vec2_encoder_ref at zero layers in float64, written over rows of a flat buffer as the kernels walk them.  sd: tensors of the tower's dtype;
    x [B, L] the values the device sees.  mut: one of MUTANTS -> [B, Tn, d] (frames_ceil: the first B Tn d elements of the longer result, which is
    what the caller's buffer would hold)"""
    a = cfg.audio_config
    W = lambda k: sd[P + k].to(F64)
    is_ = lambda m: mut == m
    kernel, stride = list(a.conv_kernel), list(a.conv_stride)
    B, L = x.shape
    T_true = frames_of(L, kernel, stride)
    T = frames_of(L, kernel, stride, ceil=is_("frames_ceil"))
    layer_norm = a.feat_extract_norm == "layer"
    Cc = a.conv_dim[0]
    gelu = lambda t: F.gelu(t)
    h = x.to(F64).reshape(-1, 1)
    prev = L
    for i, (k, s) in enumerate(zip(kernel, stride)):
        bias = W(f"feature_extractor.conv_layers.{i}.conv.bias") if a.conv_bias else None
        w = W(f"feature_extractor.conv_layers.{i}.conv.weight")
        name = f"conv{i}_"
        clip = prev
        if i == 0:
            clip += 1 if is_("clip_stride_plus") else -1 if is_("clip_stride_minus") else 0
        elif is_(name + "clip_stride"):
            clip -= 1
        taps = k - 1 if (is_(name + "taps") or (i == 0 and is_("conv0_taps"))) else k
        first = 1 if is_(name + "from_1") else 0
        y = _conv_rows(h, w, bias, B, T[i], clip, s, first, taps)                 # [B, T_i, C]
        if layer_norm:
            y = F.layer_norm(y, (Cc,), W(f"feature_extractor.conv_layers.{i}.layer_norm.weight"), W(f"feature_extractor.conv_layers.{i}.layer_norm.bias"), 1e-5)
        elif i == 0:
            rows = T[0] - 1 if is_("gn_rows_minus_1") else T[0] // GN_ROWS * GN_ROWS if is_("gn_whole_chunks") else T[0]
            mean = y[:, :rows].mean(1, keepdim=True)
            var = (y[:, :rows] - mean).pow(2).mean(1, keepdim=True)
            if is_("gn_prev_clip"):
                mean, var = mean.roll(1, 0), var.roll(1, 0)
            y = (y - mean) / torch.sqrt(var + 1e-5) * W("feature_extractor.conv_layers.0.layer_norm.weight") + W("feature_extractor.conv_layers.0.layer_norm.bias")
        h = gelu(y).reshape(-1, Cc)
        prev = T[i]
    Tn, d = T[-1], a.d_model
    h = F.layer_norm(h, (Cc,), W("feature_projection.layer_norm.weight"), W("feature_projection.layer_norm.bias"), a.layer_norm_eps)
    h = F.linear(h, W("feature_projection.projection.weight"), W("feature_projection.projection.bias")).reshape(B, Tn, d)
    K, G = a.num_conv_pos_embeddings, a.num_conv_pos_embedding_groups
    dg = d // G
    from oracle.reference_cpu import pos_conv_weight_ref
    wp = pos_conv_weight_ref(sd, P).to(F64).reshape(G, dg, dg, K)                 # [g][out][in][tap]
    bp = W("encoder.pos_conv_embed.conv.bias").reshape(G, dg)
    pad = K // 2 + (1 if is_("pos_pad_plus") else -1 if is_("pos_pad_minus") else 0)
    shift = 1 if is_("pos_drop_first") else 0                                     # even K: torch computes Tn + 1 frames and drops the LAST
    taps = K - 1 if is_("pos_taps") else K
    hp = torch.zeros(B, Tn + 2 * K + 2, d, dtype=F64)
    hp[:, K + 1:K + 1 + Tn] = h
    hg = hp.reshape(B, -1, G, dg)
    if is_("pos_next_group_channels"):
        hg = hg.roll(-1, 2)
    if is_("pos_group0_weights"):
        wp = wp[:1].expand(G, -1, -1, -1)
    if is_("pos_bias_wrong_group"):
        bp = bp.roll(-1, 0)
    idx = torch.arange(Tn)[:, None] + torch.arange(taps)[None, :] + (K + 1 - pad + shift)       # frame t, tap j reads h[t + j - pad]
    pos = torch.einsum("btjgc,gocj->btgo", hg[:, idx], wp[..., :taps]) + bp
    pos = gelu(pos).reshape(B, Tn, d)
    h = pos if is_("no_residual") else h + pos
    out = F.layer_norm(h, (d,), W("encoder.layer_norm.weight"), W("encoder.layer_norm.bias"), a.layer_norm_eps)
    if T != T_true:
        out = out.reshape(-1)[:B * T_true[-1] * d].reshape(B, T_true[-1], d)
    return out


# ------------------------------------------------------------------ reference, stand-ins, bars
def oracle(sd, cfg, x, dtype):
    """oracle.reference_cpu.wav2vec2_encoder_ref evaluated in `dtype` (module by module: every tensor it makes has that dtype) -> float64"""
    from oracle.reference_cpu import wav2vec2_encoder_ref
    with torch.no_grad():
        return wav2vec2_encoder_ref(sd, cfg, x.to(dtype)).to(F64)


def frame_dist(got, want):
    """[B, Tn]: ||got - want||_2 / ||want||_2 over the columns; inf where got is not finite"""
    got, want = got.to(F64), want.to(F64)
    e = (got - want).norm(dim=-1) / want.norm(dim=-1)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def worst(dist):
    """(largest distance, clip, frame)"""
    i = int(dist.reshape(-1).argmax())
    return dist.reshape(-1)[i].item(), i // dist.shape[1], i % dist.shape[1]


@functools.lru_cache(maxsize=None)
def _prepared(i, family, precision):
    c = CASES[i]
    cfg, sd, x = config(c), state_dict(c, family, precision), wave(c, family, precision)
    want = oracle(sd, cfg, x, F64)
    stand = frame_dist(oracle(sd, cfg, x, tdtype(precision)), want)
    return cfg, sd, x, want, stand, MARGIN[precision] * stand.max().item()


def prepared(c, family, precision):
    """-> (config, state dict in the tower's dtype, input_values [B, L] f32 holding values of the tower's dtype, the float64 reference [B, Tn, d], the
    stand-in's per-frame distance to it, the bar).  Computed once per process and shared: do not write into any of it"""
    return _prepared(CASES.index(c), family, precision)
