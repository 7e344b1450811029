"""The harness of test_w2v_stem_gpu.py, proven without a GPU (w2v_stem_util.py):

1. the case list sits on the edges it is meant for: the standard stack's lengths on their frame counts (Tn 1, 1, 2; T0 512 / 513 and 1024 / 1025 on
   either side of a GroupNorm chunk; Tn 8 / 9 around pos_k / 2; Tn 16 / 17 around the few-row GEMM kernels' last M), the two-conv stack on
   Tn 1, 7, 8, 128, 129 with an odd and an even positional kernel, and with one clip every conv layer of a short clip has at most 16 rows and one batch -
   the shape gemm_skinny_applicable sends to the weight-streaming kernels;
2. stem64 - the reference written over flat rows, every boundary a parameter - equals oracle.reference_cpu.wav2vec2_encoder_ref in float64 to 1e-11;
3. both stand-ins (torch's f32 and torch's module-by-module bf16 evaluation of the oracle) give bars that are positive, finite and under
   w2v_stem_util.CEILING in every case and family - f32 bars 1.5e-6 .. 1.1e-5 (the conv-bias case, whose ceiling is four times the others': 1.3e-5
   and 2.0e-5, torch's own f32 loss under an offset of 10 .. 30 spreads), bf16 bars 9.7e-3 .. 3.9e-2 - and every frame of a stand-in is inside its bar;
4. every mutant - the float64 reference with exactly one boundary moved - exceeds TWICE the bar of each precision on at least one frame of at least
   one case.  Measured over all cases: the weakest are gn_whole_chunks, 37 bars in bf16 (std-L2640-B3, E) and 2.0e5 bars in f32, and
   pos_bias_wrong_group, 41 bars and 2.0e5; every other mutant reaches 59 .. 154 bars in bf16;
5. AudioConfig.feat_extract_output_length and processing._wav2vec2_frames agree with the conv-stack formula for every L from 380 to 1100."""
import pytest
import torch

import w2v_stem_util as U
from w2v_stem_util import CASES, FAMILIES, MUTANTS, PRECISIONS, case_id


def test_case_list_sits_on_its_edges():
    std = {c["L"]: c["T"] for c in CASES if c["name"] == "std"}
    assert {L: T[-1] for L, T in std.items()} == {400: 1, 719: 1, 720: 2, 2569: 7, 2570: 7, 2640: 8, 2960: 9, 5129: 15, 5130: 15, 5200: 16, 5520: 17, 9000: 27}
    assert {L: std[L][0] for L in (2569, 2570, 5129, 5130)} == {2569: 512, 2570: 513, 5129: 1024, 5130: 1025}
    for L, T in std.items():
        assert T[-1] == (L - 400) // 320 + 1 and T[0] == (L - 10) // 5 + 1
        assert {c["B"] for c in CASES if c["name"] == "std" and c["L"] == L} == {1, 3}
    for k in (15, 16):
        two = [c for c in CASES if c["name"] == "two" and c["pos_k"] == k]
        assert {c["T"][-1] for c in two} == {1, 7, 8, 128, 129} and all(c["kernel"] == (10, 3) and c["groups"] == 2 for c in two)
        assert (k * (128 // 2)) % 64 == 0
    # B = 1 and every conv layer from some layer on at 16 rows or fewer: the few-row dispatch (M <= 16, batch <= 1, K = k C a multiple of 32)
    short = [c for c in CASES if c["B"] == 1 and c["T"][-1] <= 16]
    assert {c["T"][-1] for c in short} >= {1, 2, 7, 8, 15, 16} and all((k * 64) % 32 == 0 for c in short for k in c["kernel"][1:])
    assert any(c["T"][-1] == 17 and c["B"] == 1 for c in CASES)
    layer = [c for c in CASES if c["name"] == "layer"]
    assert [(c["L"], c["B"], c["norm"], c["bias"], c["stable"]) for c in layer] == [(720, 3, "layer", True, True), (5520, 3, "layer", True, True)]
    (gb,) = [c for c in CASES if c["name"] == "gnbias"]
    assert (gb["L"], gb["B"], gb["norm"], gb["bias"], gb["precisions"]) == (9000, 3, "group", True, ("f32",))
    assert all(c["B"] <= 3 and c["L"] <= 9000 and U.config(c).audio_config.encoder_layers == 0 for c in CASES)
    assert len({case_id(c) for c in CASES}) == len(CASES)


def test_conv_bias_case_has_offsets_of_10_to_30_spreads():
    """the group-norm family with conv_bias: the first conv layer's output, per clip and channel, has |mean over time| / std over time of 10 .. 30 on a
    quarter of the channels (one or two (clip, channel) pairs of family E just above 30) - the input of the GroupNorm pass whose variance is under suspicion"""
    (c,) = [c for c in CASES if c["name"] == "gnbias"]
    for fam in FAMILIES:
        cfg, sd, x, *_ = U.prepared(c, fam, "f32")
        w = sd[U.P + "feature_extractor.conv_layers.0.conv.weight"].to(U.F64)
        y = torch.nn.functional.conv1d(x.to(U.F64)[:, None], w, sd[U.P + "feature_extractor.conv_layers.0.conv.bias"].to(U.F64), stride=5)
        ratio = y.mean(-1).abs() / y.std(-1)
        assert y.shape[-1] == 1799
        big = ratio[:, ::4]
        print(f"W2V-STEM gnbias {fam}: offset / spread on the biased channels {big.min().item():.1f} .. {big.max().item():.1f}")
        assert big.min() >= 10.0 and big.max() <= 32.0 and (big <= 30.0).float().mean() >= 0.95 and ratio[:, 1::4].max() < 1.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stand_ins_stay_inside_their_bars_and_the_restated_reference_is_the_oracle(precision):
    lo, hi = float("inf"), 0.0
    for c in U.cases(precision):
        for fam in FAMILIES:
            cfg, sd, x, want, stand, bar = U.prepared(c, fam, precision)
            assert want.shape == (c["B"], c["T"][-1], 128) and want.dtype == U.F64 and torch.isfinite(want).all()
            assert all(v.dtype == U.tdtype(precision) for v in sd.values()) and torch.equal(x, x.to(U.tdtype(precision)).float())
            what = f"{case_id(c)} family {fam} {precision}"
            assert U.frame_dist(U.stem64(sd, cfg, x), want).max().item() < 1e-11, what
            assert torch.isfinite(stand).all() and 0.0 < bar <= U.CEILING[precision] * (4.0 if c["name"] == "gnbias" else 1.0), f"{what}: bar {bar:.3e}"
            assert stand.max().item() <= bar, what
            if c["name"] != "gnbias":
                lo, hi = min(lo, bar), max(hi, bar)
            # the other precision's stand-in is no stand-in for this one: torch's bf16 evaluation is far outside the f32 bars
            if precision == "f32" and c["L"] == 720:
                rough = U.frame_dist(U.oracle({k: v.bfloat16() for k, v in sd.items()}, cfg, x.bfloat16(), torch.bfloat16), want)
                assert rough.min().item() > 100 * bar, what
    print(f"W2V-STEM {precision} bars {lo:.2e} .. {hi:.2e}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mut", MUTANTS)
def test_every_mutant_exceeds_twice_the_bar(mut, precision):
    touched = [c for c in U.cases(precision) if U.touches(mut, c)]
    assert touched, f"{mut}: no case it has a meaning on"
    best = (0.0, None)
    for c in sorted(touched, key=lambda c: c["L"] * c["B"]):
        for fam in ("E", "R"):
            cfg, sd, x, want, stand, bar = U.prepared(c, fam, precision)
            got = U.stem64(sd, cfg, x, mut)
            assert got.shape == want.shape
            u = U.frame_dist(got, want).max().item() / bar
            if u > best[0]:
                best = (u, f"{case_id(c)}, {fam}")
        if best[0] >= 2.0:
            break
    print(f"W2V-STEM mutant {mut} {precision}: {best[0]:.3g} bars at {best[1]}")
    assert best[0] >= 2.0, f"{mut} ({precision}): at most {best[0]:.3g} bars ({best[1]})"


def test_frame_count_formulas_agree_from_380_to_1100():
    from ultravox_amd.processing import _wav2vec2_frames
    a = U.config(CASES[0]).audio_config
    for L in range(380, 1101):
        T = U.frames_of(L)
        if L < 400:
            assert T is None and a.feat_extract_output_length(L) <= 0 and _wav2vec2_frames(L) <= 0, L
        else:
            assert T[-1] == (L - 400) // 320 + 1 == a.feat_extract_output_length(L) == _wav2vec2_frames(L), L
